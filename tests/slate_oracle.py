"""The float64 oracle of score_items (arx_slate.h, arx/slate.py): the scores of a per-row candidate slate and their
order.  Pure numpy; shared by the CPU and the GPU tests."""
import numpy as np

KEY_NONE = 0x7FFFFFFF


def scores(U, P, b, cand):
    """[B, C] float64: U[r] . P[c] + b[c] for c = cand[r, j] in [0, V), -inf outside (b may be None)."""
    U, P = np.asarray(U, dtype=np.float64), np.asarray(P, dtype=np.float64)
    cand = np.asarray(cand).astype(np.int64)
    V = P.shape[0]
    ok = (cand >= 0) & (cand < V)
    c = np.where(ok, cand, 0)
    s = np.einsum('rd,rjd->rj', U, P[c]) if V else np.zeros(cand.shape)
    if b is not None and V:
        s = s + np.asarray(b, dtype=np.float64)[c]
    return np.where(ok, s, -np.inf)


def abs_scores(U, P, b, cand):
    """[B, C] float64: sum_i |u_i p_i| + |b| of every live slot (0 elsewhere) -- the scale of the float32 dot's bound."""
    bb = None if b is None else np.abs(np.asarray(b, dtype=np.float64))
    s = scores(np.abs(np.asarray(U, dtype=np.float64)), np.abs(np.asarray(P, dtype=np.float64)), bb, cand)
    return np.where(np.isneginf(s), 0.0, s)


def bound(d):
    """|got - ref| <= bound(d) * (sum_i |u_i p_i| + |b|): a float32 dot of d terms plus the bias, in any order, with
    or without FMA."""
    return 2.0 * (d + 1) * 2.0 ** -24


def order(sc, cand, k):
    """(ids int32 [B, k], values [B, k] of sc's dtype): slots by (score desc, slot asc), the first k; (-1, -inf) where
    a row has fewer than k slots above -inf."""
    sc, cand = np.asarray(sc), np.asarray(cand)
    B, C = sc.shape
    ids = np.full((B, k), -1, dtype=np.int32)
    vals = np.full((B, k), -np.inf, dtype=sc.dtype)
    slot = np.arange(C)
    for r in range(B):
        o = np.lexsort((slot, -sc[r].astype(np.float64)))[:k]
        vals[r, :len(o)] = sc[r, o]
        ids[r, :len(o)] = cand[r, o]
    ids[np.isneginf(vals)] = -1
    return ids, vals


def dyadic(rng, B, V, d):
    """U [B, d], P [V, d] with entries k / 2 and b [V] with entries k / 4: every score is exact in float32."""
    U = (rng.integers(-2, 3, size=(B, d)) / 2.0).astype(np.float32)
    P = (rng.integers(-2, 3, size=(V, d)) / 2.0).astype(np.float32)
    b = (rng.integers(-4, 5, size=V) / 4.0).astype(np.float32)
    return U, P, b


def slate(rng, B, C, V):
    """int32 [B, C] drawn from [-1, V + 2) with some ARX_KEY_NONE; with more than one row the last is all -1, and
    slot 0 of the first row is always live."""
    cand = rng.integers(-1, V + 2, size=(B, C)).astype(np.int32)
    cand[rng.random((B, C)) < 0.05] = KEY_NONE
    if B > 1:
        cand[B - 1] = -1
    cand[0, 0] = V - 1
    if C >= 4:
        cand[0, 1:4] = [V, KEY_NONE, -2]
    return cand
