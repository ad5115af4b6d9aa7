"""The float64 oracle of list_logprob (include/arx_list_logp.h): the reason code of every entry of a given list and the
log-probability of the list under the sampling policy -- written as "clean the list, call the oracle of the draw's
propensities (tests/recommend_logprob_oracle.py) on it, stamp".  The tolerance is that oracle's, unchanged, on the
drawable entries."""
import numpy as np

import recommend_logprob_oracle as RL
import tags_oracle as T

OK, EMPTY, RANGE, EXCLUDED, TAGS, REPEAT, NOSCORE = range(7)


def why(L, lists, tags=None, want_any=None, want_all=None, ex_lists=None):
    """int32 [B, k]: the lowest code that applies to each entry (0 drawable, 1 the entry is -1, 2 any other negative
    value or >= V, 3 in the row's exclusion list, 4 fails the tag test, 5 passed 2-4 and an earlier slot holds the same
    column, 6 passed all of that and its score is -inf)."""
    lists = np.asarray(lists, dtype=np.int64)
    B, k = lists.shape
    V = L.shape[1]
    tag_ok = T.eligible(tags, want_any, want_all) if tags is not None else np.ones((B, V), dtype=bool)
    out = np.zeros((B, k), dtype=np.int32)
    for r in range(B):
        ex = set(int(c) for c in ex_lists[r]) if ex_lists is not None else set()
        seen = set()
        for t in range(k):
            c = int(lists[r, t])
            if c == -1:
                out[r, t] = EMPTY
            elif c < 0 or c >= V:
                out[r, t] = RANGE
            elif c in ex:
                out[r, t] = EXCLUDED
            elif not tag_ok[r, c]:
                out[r, t] = TAGS
            elif c in seen:
                out[r, t] = REPEAT
            else:
                seen.add(c)                     # (the lowest slot stays: a NOSCORE first copy still makes the next a REPEAT)
                out[r, t] = NOSCORE if L[r, c] == -np.inf else OK
    return out


def clean(lists, codes):
    """the list with every non-drawable entry taken out (-1)"""
    return np.where(codes == OK, np.asarray(lists, dtype=np.int64), -1)


def logp(L, lists, tau, tags=None, want_any=None, want_all=None, ex_lists=None):
    """-> (logp float64 [B, k], codes int32 [B, k], tolerance float64 [B, k]): clean, RL.logp on the drawable entries
    in their order (a non-drawable entry is ABSENT for the others), stamp: 0 at EMPTY, -inf at the codes 2-6.  The
    tolerance is RL.tolerance of the row, 0 at the non-drawable entries (they are exact)."""
    lists = np.asarray(lists, dtype=np.int64)
    B, k = lists.shape
    codes = why(L, lists, tags, want_any, want_all, ex_lists)
    cl = clean(lists, codes)
    elig = RL.eligible(L, tags, want_any, want_all, ex_lists)
    packed = np.full((B, k), -1, dtype=np.int64)            # RL.logp wants the -1 entries last
    for r in range(B):
        live = cl[r][cl[r] >= 0]
        packed[r, :len(live)] = live
    lp_packed = RL.logp(L, elig, packed, tau)
    tol_packed = RL.tolerance(L, elig, tau, lp_packed)
    lp = np.zeros((B, k), dtype=np.float64)
    tol = np.zeros((B, k), dtype=np.float64)
    for r in range(B):
        at = np.nonzero(cl[r] >= 0)[0]
        lp[r, at] = lp_packed[r, :len(at)]
        tol[r, at] = tol_packed[r, :len(at)]
    lp[codes >= RANGE] = -np.inf
    return lp, codes, tol
