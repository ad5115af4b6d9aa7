"""The float64 oracle of score_items(sample_temperature=) (include/arx_slate_sample.h): which slots of a scored slate
compete, the order of their Gumbel keys, and the log-probability of every pick given the picks before it.  Pure numpy;
shared by the CPU and the GPU tests.

The GPU tests hand in the DEVICE's own scores and the DEVICE's own noise (arx_topk_gumbel_add with tau = 1 over a zero
matrix, indexed by candidate id): key = float32(float64(tau) * float64(g) + float64(s)) (sample_oracle.keys states why
that is fmaf), tau == 0: key = s.  Keys are compared through arx_topk's order-preserving image (-0 below +0).
"""
import itertools

import numpy as np

import sample_oracle as SM


def image(key):
    """float32 -> uint32, larger float <-> larger unsigned (topk.hip ord_key)."""
    b = np.ascontiguousarray(key, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def competitors(cand_row, s_row):
    """bool [C]: live (id >= 0 and a finite score) and no lower-numbered live slot with the same id."""
    cand_row = np.asarray(cand_row).astype(np.int64)
    with np.errstate(invalid='ignore'):
        live = (cand_row >= 0) & np.isfinite(np.asarray(s_row, dtype=np.float64))
    comp = np.zeros(len(cand_row), dtype=bool)
    idx = np.nonzero(live)[0]
    comp[idx[np.unique(cand_row[idx], return_index=True)[1]]] = True       # (the first slot of every id)
    return comp


def keys(s_row, g_row, tau):
    """float32 keys of one row (every slot; the caller masks)."""
    s_row = np.asarray(s_row, dtype=np.float32)
    if tau == 0:
        return s_row.copy()
    with np.errstate(invalid='ignore', over='ignore'):
        return (np.float64(np.float32(tau)) * np.asarray(g_row, dtype=np.float64) + s_row.astype(np.float64)) \
            .astype(np.float32)


def select(cand, scores, g, tau, k):
    """cand int [B, C], scores float32 [B, C], g [B, C] the noise of every slot's item, tau [B] ->
    (ids int32 [B, k], values float32 [B, k], pos int32 [B, k]) in selection order, (-1, -inf, -1) past the last
    competitor."""
    cand, scores = np.asarray(cand), np.asarray(scores, dtype=np.float32)
    B, C = cand.shape
    ids = np.full((B, k), -1, dtype=np.int32)
    vals = np.full((B, k), -np.inf, dtype=np.float32)
    pos = np.full((B, k), -1, dtype=np.int32)
    slot = np.arange(C)
    for r in range(B):
        comp = competitors(cand[r], scores[r])
        img = image(keys(scores[r], g[r], float(tau[r]))).astype(np.int64)
        o = np.lexsort((slot, -img))
        o = o[comp[o]][:k]
        ids[r, :len(o)] = cand[r, o]
        vals[r, :len(o)] = scores[r, o]
        pos[r, :len(o)] = o
    return ids, vals, pos


def logprob(cand, scores, tau, pos):
    """float64 [B, k]: for the picks pos (slots in selection order, -1: none) the log-probability of pick t given the
    picks before it, over the row's competitors, a = s / tau in float64; 0 where tau == 0 and where pos < 0.  Every
    remaining mass is summed from what is left (never total minus picked): the log-sum-exp of the competitors that are
    never picked, then one pick after the other joined from the last to the first (np.logaddexp re-centres every
    join on its larger term)."""
    cand, scores, pos = np.asarray(cand), np.asarray(scores, dtype=np.float32), np.asarray(pos)
    B, k = pos.shape
    out = np.zeros((B, k), dtype=np.float64)
    for r in range(B):
        t_r = float(np.float32(tau[r]))
        n = int((pos[r] >= 0).sum())
        assert (pos[r, :n] >= 0).all(), "row %d: a real pick after a missing one" % r
        if t_r == 0 or n == 0:
            continue
        left = competitors(cand[r], scores[r])
        picks = pos[r, :n].astype(np.int64)
        assert left[picks].all() and len(np.unique(picks)) == n, "row %d: a pick that does not compete, or twice" % r
        left[picks] = False
        a = scores[r].astype(np.float64) / t_r
        rest = a[left]
        base = rest.max() + np.log(np.exp(rest - rest.max()).sum()) if len(rest) else -np.inf
        mass = np.logaddexp.accumulate(np.concatenate([[base], a[picks][::-1]]))[1:][::-1]
        out[r, :n] = a[picks] - mass
    return out


def tolerance(cand, scores, tau, lp, C):
    """[B, k]: 2^-20 (1 + (smax - smin) / tau) + 2^-22 |logp| + C 2^-24, smax / smin over the row's live scores."""
    scores = np.asarray(scores, dtype=np.float32)
    B = scores.shape[0]
    tol = np.zeros(np.shape(lp), dtype=np.float64)
    for r in range(B):
        t_r = float(np.float32(tau[r]))
        comp = competitors(np.asarray(cand)[r], scores[r])
        if t_r == 0 or not comp.any():
            continue
        s = scores[r][comp].astype(np.float64)
        tol[r] = 2.0 ** -20 * (1.0 + (s.max() - s.min()) / t_r) + 2.0 ** -22 * np.abs(lp[r]) + C * 2.0 ** -24
    return tol


def noise64(seed, rows, cand):
    """The float64 restatement's own noise of every slot: g [B, C] (0 where the id is negative)."""
    cand = np.asarray(cand)
    g = np.zeros(cand.shape, dtype=np.float64)
    for i, r in enumerate(rows):
        ok = cand[i] >= 0
        g[i, ok] = SM.gumbel64(SM.bits(seed, [r], cand[i, ok].astype(np.uint32)))[0]
    return g


def pair_chi2(ids, lp, items, exact_logp):
    """The law statistic: the chi^2 of the ordered-pair counts of ids [rows, 2] over `items` against
    rows * exp(logp[0] + logp[1]), the propensity REPORTED with the draw (lp [rows, 2]; the mean over the rows that drew
    the pair); a pair nobody drew reports nothing and takes exact_logp[(a, b)].  -> (chi2, cells, smallest expected)."""
    rows = ids.shape[0]
    chi2, cells, small = 0.0, 0, np.inf
    for a, b in itertools.permutations(items, 2):
        hit = (ids[:, 0] == a) & (ids[:, 1] == b)
        n = int(hit.sum())
        e = rows * np.exp(lp[hit].sum(axis=1).mean() if n else exact_logp[(a, b)])
        chi2 += (n - e) ** 2 / e
        cells += 1
        small = min(small, e)
    return float(chi2), cells, float(small)


def exact_pairs(items, scores, tau):
    """{(a, b): log P(first a, then b)} of Plackett-Luce over distinct items."""
    w = np.exp(np.asarray(scores, dtype=np.float64) / tau)
    W = w.sum()
    return {(items[i], items[j]): float(np.log(w[i] / W) + np.log(w[j] / (W - w[i])))
            for i, j in itertools.permutations(range(len(items)), 2)}
