"""Oracles and data of the similar_items tests (cosine nearest neighbours over the full item vocabulary).

EXACT DATA: row r holds +-2^e_r (e_r in {-1, 0, 1, 2}) on exactly 16 or 64 positions and zeros elsewhere, so its norm is
4 * 2^e_r or 8 * 2^e_r, its inverse norm a power of two, its unit row +-1/4 or +-1/8 on the support, and every cosine a
sum of at most 64 dyadic terms of one magnitude scaled by a power of two: exact in float32 in ANY summation order.  Ties
are therefore real ties and the kernels compare with the float64 oracle bit for bit (test_similar_abi_cpu.py checks
that a float32 numpy evaluation of the formula and the float64 one agree on this data).  The special rows: a
duplicate, a 2x and a -1x multiple of row 0 (cosine exactly 1, 1, -1: scale invariance and the tie rule), one all-zero
row (cosine 0 with everything, also as a query), and a duplicate at the far end of the table."""
import numpy as np

KEY_NONE = 0x7FFFFFFF


def exact_table(rng, n, d):
    assert d >= 16
    E = np.zeros((n, d), dtype=np.float32)
    for r in range(n):
        m = 64 if d >= 64 and rng.random() < 0.5 else 16
        pos = rng.choice(d, size=m, replace=False)
        E[r, pos] = rng.choice([-1.0, 1.0], size=m) * 2.0 ** int(rng.integers(-1, 3))
    if n >= 8:
        E[1] = E[0]
        E[2] = 2.0 * E[0]
        E[3] = -E[0]
        E[4] = 0.0
        E[n - 1] = E[5]
    return E


ZERO_ROW = 4          # of exact_table(n >= 8)


def inv_norm64(E):
    s = (E.astype(np.float64) ** 2).sum(1)
    with np.errstate(divide='ignore'):
        return np.where(s > 0, 1.0 / np.sqrt(s), 0.0)


def cos64(Q, E):
    """[len(Q), len(E)] float64 cosines of the rows of Q with the rows of E; 0 where either is a zero row."""
    q = Q.astype(np.float64) * inv_norm64(Q)[:, None]
    return (q @ E.astype(np.float64).T) * inv_norm64(E)[None, :] + 0.0


def cos32(Q, E):
    """The same formula evaluated in float32 the way the kernels state it: f32 sums of squares, 1 / sqrt, the unit
    query rows, an f32 dot, times the column's inverse norm, + 0."""
    def inv(X):
        s = (X * X).sum(1, dtype=np.float32)
        with np.errstate(divide='ignore'):
            return np.where(s > 0, np.float32(1.0) / np.sqrt(s, dtype=np.float32), np.float32(0.0)).astype(np.float32)
    q = (Q * inv(Q)[:, None]).astype(np.float32)
    return ((q @ E.T).astype(np.float32) * inv(E)[None, :] + np.float32(0.0)).astype(np.float32)


def topk_cos(C, k, self_ids=None):
    """(values float64 [B, k], ids int64 [B, k]) by (cosine desc, id asc) over the columns of C; self_ids[r] (>= 0)
    is left out of row r; (-inf, -1) where fewer than k columns are left."""
    B, V = C.shape
    x = C.astype(np.float64).copy()
    if self_ids is not None:
        for r, s in enumerate(self_ids):
            if 0 <= s < V:
                x[r, int(s)] = -np.inf
    vals = np.full((B, k), -np.inf)
    ids = np.full((B, k), -1, dtype=np.int64)
    for r in range(B):
        o = np.lexsort((np.arange(V), -x[r]))[:k]
        vals[r, :len(o)], ids[r, :len(o)] = x[r, o], o
    ids[np.isneginf(vals)] = -1
    return vals, ids


def cos_atol(d):
    """The float32 running-error bound of a cosine formed as the kernels form it, u = 2^-24: each inverse norm carries
    (d / 2 + 2) u (a length-d sum of squares, halved by the square root, + the root and the division), the unit query
    row one more rounding, the length-d dot of a unit row with a row of norm n at most d u n, the scale one rounding:
    2 (d / 2 + 2) + d + 2 = 2 d + 6 <= 2 (d + 4) roundings.  (Twice this was granted at first; the kernels stay far
    inside: the largest error seen on an MI355X is 4.8e-7 at d = 128, where this bound is 1.6e-5.)"""
    return 2.0 * (d + 4) * 2.0 ** -24


def check_random(got_ids, got_vals, C64, k, self_ids, atol):
    """The random-data rule: every returned id has a float64 cosine within atol of its returned value and at least the
    oracle's k-th value - atol, is no duplicate and is not the query itself.  Returns the largest value error."""
    B = C64.shape[0]
    want_v, _ = topk_cos(C64, k, self_ids)
    worst = 0.0
    for r in range(B):
        ids = np.asarray(got_ids[r], dtype=np.int64)
        assert (ids >= 0).all() and (ids < C64.shape[1]).all(), (r, ids)
        assert len(set(ids.tolist())) == len(ids), ("duplicate id", r, ids)
        if self_ids is not None:
            assert int(self_ids[r]) not in set(ids.tolist()), ("the query itself", r)
        err = np.abs(C64[r, ids] - np.asarray(got_vals[r], dtype=np.float64))
        worst = max(worst, float(err.max()))
        assert (err <= atol).all(), (r, float(err.max()), atol)
        assert (C64[r, ids] >= want_v[r, k - 1] - atol).all(), (r, C64[r, ids], want_v[r, k - 1])
        assert (np.diff(np.asarray(got_vals[r], dtype=np.float64)) <= 0).all(), ("not descending", r)
    return worst
