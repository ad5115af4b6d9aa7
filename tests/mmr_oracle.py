"""The float64 oracle of score_items(diversify=) (arx_diverse.h, arx/slate.py): the greedy MMR selection over a scored
slate, and a replay that judges a device's pick at every step against the float64 best GIVEN the device's own prefix
(so one early near-tie cannot make every later step look wrong).  Pure numpy; shared by the CPU and the GPU tests."""
import numpy as np


def unit_rows(P):
    """float64 rows of P scaled to length 1; a zero row stays zero."""
    P = np.asarray(P, dtype=np.float64)
    n = np.sqrt((P * P).sum(axis=1))
    return P * np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)[:, None]


class _Row(object):
    """One request row: live slots, rel, the slots' unit rows and groups; pen / picked / group counts as picks go."""

    def __init__(self, cand, s, X, lam, groups, m):
        cand = np.asarray(cand).astype(np.int64)
        s = np.asarray(s, dtype=np.float64)
        V = X.shape[0]
        self.C = len(cand)
        self.s = s
        self.live = (cand >= 0) & (cand < V) & np.isfinite(s)
        c = np.where(self.live, cand, 0)
        self.x = np.where(self.live[:, None], X[c], 0.0) if V else np.zeros((self.C, X.shape[1]))
        self.rel = np.zeros(self.C)
        if self.live.any():
            lo, hi = s[self.live].min(), s[self.live].max()
            self.rel[self.live] = (s[self.live] - lo) / (hi - lo) if hi > lo else 1.0
        self.g = np.full(self.C, -1, dtype=np.int64)
        if groups is not None and V:
            self.g[self.live] = np.asarray(groups).astype(np.int64)[c[self.live]]
        self.m = None if groups is None else max(1, int(m))
        self.lam = float(lam)
        self.pen = np.zeros(self.C)
        self.picked = np.zeros(self.C, dtype=bool)
        self.count = {}

    def eligible(self):
        e = self.live & ~self.picked
        if self.m is not None:
            full = np.array([g >= 0 and self.count.get(int(g), 0) >= self.m for g in self.g])
            e &= ~full
        return e

    def obj(self):
        return self.lam * self.rel - (1.0 - self.lam) * self.pen

    def ranked(self):
        """the eligible slots by (obj desc, score desc, slot asc)"""
        e = np.nonzero(self.eligible())[0]
        o = self.obj()
        return e[np.lexsort((e, -self.s[e], -o[e]))]

    def take(self, j):
        self.picked[j] = True
        if self.g[j] >= 0:
            self.count[int(self.g[j])] = self.count.get(int(self.g[j]), 0) + 1
        self.pen = np.maximum(self.pen, self.x @ self.x[j])


def _args(cand, s, lam, groups, m):
    cand, s = np.asarray(cand), np.asarray(s)
    B = cand.shape[0]
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (B,))
    m = None if groups is None else np.broadcast_to(np.asarray(m), (B,))
    return cand, s, B, lam, m


def select(cand, s, P, lam, k, groups=None, m=None):
    """(ids int32 [B, k], values [B, k] of s's dtype, pos int32 [B, k]): section 1 of the contract in float64.  cand,
    s [B, C]; P [V, d]; lam a scalar or [B]; groups [V] with m a scalar or [B], or both None."""
    cand, s, B, lam, m = _args(cand, s, lam, groups, m)
    X = unit_rows(P)
    ids = np.full((B, k), -1, dtype=np.int32)
    vals = np.full((B, k), -np.inf, dtype=s.dtype)
    pos = np.full((B, k), -1, dtype=np.int32)
    for r in range(B):
        row = _Row(cand[r], s[r], X, lam[r], groups, None if m is None else m[r])
        for t in range(k):
            order = row.ranked()
            if not len(order):
                break
            j = int(order[0])
            ids[r, t], vals[r, t], pos[r, t] = cand[r, j], s[r, j], j
            row.take(j)
    return ids, vals, pos


def replay(cand, s, P, lam, groups, m, got_pos):
    """Judge got_pos [B, k] (the device's slots, -1 past its last pick) step by step, each step with the DEVICE's own
    earlier picks as the prefix.  Returns float64 / int arrays [B, k]:
      pick  the float64 objective of the device's pick (nan where it wrote -1 or picked an ineligible slot)
      best  the float64 best over the eligible slots (nan where none is eligible)
      gap   best minus the second best eligible objective (inf with fewer than two)
      want  the oracle's slot at that step: by (obj desc, score desc, slot asc), -1 where none is eligible
      ok    the pick was eligible (live, not picked before, its group not full) -- or -1 with nothing eligible."""
    cand, s, B, lam, m = _args(cand, s, lam, groups, m)
    got_pos = np.asarray(got_pos)
    k = got_pos.shape[1]
    X = unit_rows(P)
    pick = np.full((B, k), np.nan)
    best = np.full((B, k), np.nan)
    gap = np.full((B, k), np.inf)
    want = np.full((B, k), -1, dtype=np.int64)
    ok = np.zeros((B, k), dtype=bool)
    for r in range(B):
        row = _Row(cand[r], s[r], X, lam[r], groups, None if m is None else m[r])
        for t in range(k):
            order = row.ranked()
            o = row.obj()
            j = int(got_pos[r, t])
            if len(order):
                want[r, t], best[r, t] = order[0], o[order[0]]
                if len(order) > 1:
                    gap[r, t] = o[order[0]] - o[order[1]]
            if j < 0:
                ok[r, t] = not len(order)
                if len(order):
                    break                                  # (the device stopped early: nothing after it is judged ok)
                continue
            if j >= row.C or j not in order:
                break
            ok[r, t], pick[r, t] = True, o[j]
            row.take(j)
    return pick, best, gap, want, ok
