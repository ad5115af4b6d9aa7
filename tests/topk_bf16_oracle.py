"""The numpy oracle of recommend(scan_dtype='bf16') (arx_topk_bf16.h, arx/topk.py): round-to-nearest-even bf16, the
approximate scores of the filter, its one-sided test, and filter-then-rescore as a whole.  Pure numpy; shared by the CPU
and the GPU tests."""
import numpy as np


def bf16_bits(x):
    """uint16 bit patterns of the round-to-nearest-even bf16 of float32 x (ties to the even 8-bit significand; a NaN
    becomes the quiet NaN 0x7fc0)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[np.isnan(x)] = 0x7fc0
    return r


def bf16_round(x):
    """float32 values of the bf16 roundings of x."""
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def approx_dot(U, P):
    """[B, V] float32: bf16(U) . bf16(P)^T with every product exact (8 x 8 significand bits) and the sum kept in
    float32, one term after the other -- what the matrix pipe computes up to the order of its adds."""
    Ub, Pb = bf16_round(U), bf16_round(P)
    acc = np.zeros((Ub.shape[0], Pb.shape[0]), dtype=np.float32)
    for j in range(Ub.shape[1]):
        acc = (acc + Ub[:, j:j + 1] * Pb[None, :, j]).astype(np.float32)     # (the product is exact in float32)
    return acc


def exact_dot(U, P):
    return np.asarray(U, dtype=np.float64) @ np.asarray(P, dtype=np.float64).T


def norms(X):
    return np.sqrt((np.asarray(X, dtype=np.float64) ** 2).sum(1))


def two_below(t):
    """the float32 two steps below each finite t (what the kernel compares against); infinities stay."""
    t = np.asarray(t, dtype=np.float32)
    lo = np.nextafter(np.nextafter(t, np.float32(-np.inf)), np.float32(-np.inf))
    return np.where(np.isfinite(t), lo, t).astype(np.float32)


def widened(U, P, bias, coeff, approx=None):
    """[B, V] float64: v~ + coeff |u| |p| with v~ = float32(approx + bias) -- the left side of the filter's test, the
    margin in float64 from the exact norms (the device rounds both norms up: its margin is never smaller)."""
    a = approx_dot(U, P) if approx is None else approx
    v = a if bias is None else (a + np.asarray(bias, dtype=np.float32)[None, :]).astype(np.float32)
    return v.astype(np.float64) + coeff * norms(U)[:, None] * norms(P)[None, :], v


def survivors(U, P, bias, thr, coeff, eligible=None):
    """bool [B, V]: the columns whose widened logit beats thr[r] (float32) in float64 arithmetic, and eligible."""
    w, _ = widened(U, P, bias, coeff)
    s = w > np.asarray(thr, dtype=np.float64)[:, None]
    return s if eligible is None else s & eligible


def topk_rows(scores, k):
    """(values [B, k], ids int64 [B, k]) by (score desc, column asc); (-inf, -1) where fewer than k are above -inf."""
    B, V = scores.shape
    vals = np.full((B, k), -np.inf, dtype=scores.dtype)
    ids = np.full((B, k), -1, dtype=np.int64)
    col = np.arange(V)
    for r in range(B):
        o = np.lexsort((col, -scores[r].astype(np.float64)))[:k]
        vals[r, :len(o)], ids[r, :len(o)] = scores[r, o], o
    ids[np.isneginf(vals)] = -1
    return vals, ids


def filter_then_rescore(U, P, bias, k, n0, coeff, eligible=None):
    """The whole scheme in numpy: the first n0 columns scored exactly (float64) give every row its threshold (the
    k-th best eligible, -inf with fewer), the tail passes the bf16 filter widened by coeff, the survivors are
    re-scored exactly, top-k of the union.  Returns (values, ids, number of tail survivors per row)."""
    ex = exact_dot(U, P)
    if bias is not None:
        ex = ex + np.asarray(bias, dtype=np.float64)[None, :]
    if eligible is not None:
        ex = np.where(eligible, ex, -np.inf)
    first = ex[:, :n0]
    thr = np.sort(first, axis=1)[:, ::-1][:, k - 1]
    s = survivors(U, P[n0:], None if bias is None else np.asarray(bias)[n0:], thr.astype(np.float32), coeff,
                  None if eligible is None else eligible[:, n0:])
    kept = np.full(ex.shape, -np.inf)
    kept[:, :n0] = first
    kept[:, n0:] = np.where(s, ex[:, n0:], -np.inf)
    v, i = topk_rows(kept, k)
    return v, i, s.sum(1)


def exact_topk(U, P, bias, k, eligible=None):
    ex = exact_dot(U, P)
    if bias is not None:
        ex = ex + np.asarray(bias, dtype=np.float64)[None, :]
    if eligible is not None:
        ex = np.where(eligible, ex, -np.inf)
    return topk_rows(ex, k) + (ex,)


def dyadic(rng, B, V, d):
    """U [B, d], P [V, d]: multiples of 2^-3 in [-2, 2]; b [V]: multiples of 2^-6 in [-1, 1] -- every product and every
    sum is exact in bf16 and in float32 alike, in any order."""
    U = (rng.integers(-16, 17, size=(B, d)) / 8.0).astype(np.float32)
    P = (rng.integers(-16, 17, size=(V, d)) / 8.0).astype(np.float32)
    b = (rng.integers(-64, 65, size=V) / 64.0).astype(np.float32)
    return U, P, b
