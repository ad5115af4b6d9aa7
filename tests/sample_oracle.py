"""The numpy oracle of the sampled recommend (include/arx_sample.h), shared by the CPU and GPU tests.

The noise is a pure function of (seed, row, column): row_words / bits restate the hash with numpy's wrapping unsigned
arithmetic, gumbel64 the two logarithms in float64.  The GPU tests rank the DEVICE's own logits plus the DEVICE's own
noise: key = float32(float64(tau) * float64(g) + float64(v)) (the product of two float32 is exact in float64, so this is
fmaf unless the float64 sum lands within 2^-29 of a float32 rounding boundary), ineligible and excluded columns at
-inf, a stable sort by (-key, column), the first k, -inf entries -> index -1.
"""
import itertools

import numpy as np

import tags_oracle as T

M64 = (1 << 64) - 1


def row_words(seed, row):
    """(b0, b1) of one noise row, python ints."""
    z = (int(seed) * 0x9E3779B97F4A7C15 + (int(row) + 1) * 0xD1B54A32D192ED03) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    z = z ^ (z >> 31)
    return z & 0xffffffff, z >> 32


def bits(seed, rows, cols):
    """The hash x, uint32 [len(rows), len(cols)]; m = x >> 9 is the draw."""
    w = np.array([row_words(seed, r) for r in rows], dtype=np.uint64).reshape(-1, 2)
    with np.errstate(over='ignore'):
        x = (np.asarray(cols, dtype=np.uint32)[None, :] + w[:, 0:1].astype(np.uint32)).astype(np.uint32)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x ^= w[:, 1:2].astype(np.uint32)
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def u_of(x, dtype=np.float64):
    """u = (m + 0.5) 2^-23: exact in float32 and float64."""
    return ((x >> np.uint32(9)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -23)


def m_of_u(u):
    """the 23 bits back out of a u (exact)"""
    return np.round(np.asarray(u, dtype=np.float64) * 2.0 ** 23 - 0.5).astype(np.int64)


def m_of_g(g):
    """The 23 bits behind a float32 g: m read off u = exp(-exp(-g)), then the nearest in float64 g of m - 1, m, m + 1."""
    g = np.asarray(g, dtype=np.float64)
    m0 = m_of_u(np.exp(-np.exp(-g)))
    cand = np.clip(m0[..., None] + np.array([-1, 0, 1]), 0, 2 ** 23 - 1)
    g64 = -np.log(-np.log((cand.astype(np.float64) + 0.5) * 2.0 ** -23))
    return np.take_along_axis(cand, np.abs(g64 - g[..., None]).argmin(-1)[..., None], -1)[..., 0]


def recoverable(x):
    """Where m_of_g must give m back: the nearer neighbour of m lies more than 2 e off in g, e = 4 x the error of a
    correctly rounded float32 evaluation (half an ulp at t = -log u, carried through the second logarithm as 1 / t,
    and half an ulp at g)."""
    m = (x >> np.uint32(9)).astype(np.int64)
    g_of = lambda mm: -np.log(-np.log((mm.astype(np.float64) + 0.5) * 2.0 ** -23))
    ulp = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)
    g, t = g_of(m), -np.log((m + 0.5) * 2.0 ** -23)
    e = 4 * (ulp(g) / 2 + ulp(t) / 2 / t)
    lo, hi = np.clip(m - 1, 0, 2 ** 23 - 1), np.clip(m + 1, 0, 2 ** 23 - 1)
    half = np.minimum(np.abs(g_of(lo) - g), np.abs(g_of(hi) - g)) / 2
    return half > e


def gumbel64(x):
    return -np.log(-np.log(u_of(x, np.float64)))


def gumbel32(x):
    """numpy's own float32 evaluation of the formula"""
    return -np.log(-np.log(u_of(x, np.float32)))


def keys(x, g, tau):
    """x [B, V] float32 (masked logits), g [B, V] float32 noise, tau [B] float32 -> float32 keys."""
    with np.errstate(invalid='ignore'):
        k = (tau.astype(np.float64)[:, None] * g.astype(np.float64) + x.astype(np.float64)).astype(np.float32)
    k[np.isneginf(x)] = -np.inf
    return k


def strip_bound(key, score):
    """|stripped value - score| <= 2^-23 (|key| + |score|): one rounding at the key, one at the difference."""
    return 2.0 ** -23 * (np.abs(key.astype(np.float64)) + np.abs(score.astype(np.float64)))


def sample_topk(logits, g, tau, k, tags=None, want_any=None, want_all=None, ex_lists=None):
    """-> (key values [B, k], scores [B, k], indices [B, k] int64 in selection order, keys [B, V])."""
    x = T.masked(logits, tags, want_any, want_all, ex_lists)
    ky = keys(x, g, np.asarray(tau, dtype=np.float32))
    kv, ki = T.topk(ky, k)
    sc = np.where(ki >= 0, np.take_along_axis(x, np.maximum(ki, 0), 1), -np.inf).astype(np.float32)
    return kv, sc, ki, ky


def close_rows(ky, kv, sc, k):
    """Rows whose k-th and (k + 1)-th keys are closer than the strip bound of the k-th (the rows the id comparison
    may leave out)."""
    B, V = ky.shape
    if k >= V:
        return np.zeros(B, dtype=bool)
    nxt = -np.partition(-ky, k, axis=1)[:, k]
    with np.errstate(invalid='ignore'):
        gap = kv[:, k - 1].astype(np.float64) - nxt.astype(np.float64)
        bound = strip_bound(kv[:, k - 1], sc[:, k - 1])
    return np.isfinite(gap) & np.isfinite(bound) & (gap < bound)


# ---- the law: Plackett-Luce
def pl_inclusion(scores, tau, k):
    """P(item in the first k draws) of sequential sampling without replacement from softmax(scores / tau)."""
    w = np.exp(np.asarray(scores, dtype=np.float64) / tau)
    n = len(w)
    inc = np.zeros(n)
    for perm in itertools.permutations(range(n), k):
        p, rest = 1.0, w.sum()
        for i in perm:
            p *= w[i] / rest
            rest -= w[i]
        inc[list(perm)] += p
    return inc


def law_stats(ids, scores, tau, k=3):
    """ids [rows, >= k] draws in selection order -> (chi^2 of the first pick against softmax(scores / tau), the
    largest |count - expected| / sigma of the top-k inclusion counts)."""
    rows, n = ids.shape[0], len(scores)
    p = np.exp(np.asarray(scores, dtype=np.float64) / tau)
    p /= p.sum()
    first = np.bincount(ids[:, 0], minlength=n).astype(np.float64)
    chi2 = float((((first - rows * p) ** 2) / (rows * p)).sum())
    inc = pl_inclusion(scores, tau, k)
    cnt = np.bincount(ids[:, :k].reshape(-1), minlength=n).astype(np.float64)
    z = np.abs(cnt - rows * inc) / np.sqrt(rows * inc * (1 - inc))
    return chi2, float(z.max())


def oracle_draws(seed, rows, scores, tau, k):
    """The float64 restatement's own draws for equal rows of `scores`: ids [rows, k] in selection order."""
    g = gumbel64(bits(seed, range(rows), range(len(scores))))
    ky = np.asarray(scores, dtype=np.float64)[None, :] + tau * g
    return np.argsort(-ky, axis=1, kind='stable')[:, :k]
