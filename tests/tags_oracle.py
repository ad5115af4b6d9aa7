"""The numpy oracle of recommend within item tags, shared by the CPU and GPU tests.

Column c (tag word tags[c], uint32) is eligible for row r (words any[r], all[r]) iff
    (any[r] == 0 or tags[c] & any[r] != 0) and tags[c] & all[r] == all[r].
topk: ineligible and excluded columns of the given logits set to -inf, a stable sort by (-value, column), the first
k, -inf entries -> index -1.
"""
import numpy as np


def eligible(tags, want_any, want_all):
    """bool [B, V]"""
    t = np.asarray(tags).astype(np.uint32)[None, :]
    a = np.asarray(want_any).astype(np.uint32)[:, None]
    l = np.asarray(want_all).astype(np.uint32)[:, None]
    return ((a == 0) | ((t & a) != 0)) & ((t & l) == l)


def masked(logits, tags=None, want_any=None, want_all=None, ex_lists=None):
    x = np.array(logits, dtype=np.float32, copy=True)
    if tags is not None:
        x[~eligible(tags, want_any, want_all)] = -np.inf
    if ex_lists is not None:
        for r, cols in enumerate(ex_lists):
            if len(cols):
                x[r, np.asarray(cols, dtype=np.int64)] = -np.inf
    return x


def topk(logits, k, tags=None, want_any=None, want_all=None, ex_lists=None):
    """logits [B, V]; -> (values [B, k] float32, indices [B, k] int64)."""
    x = masked(logits, tags, want_any, want_all, ex_lists)
    B, V = x.shape
    vals = np.empty((B, k), dtype=np.float32)
    inds = np.empty((B, k), dtype=np.int64)
    kth = np.partition(x, V - k, axis=1)[:, V - k]
    for r in range(B):
        c = np.nonzero(x[r] >= kth[r])[0]              # (ascending columns: the lexsort below is stable in them)
        o = np.lexsort((c, -x[r, c]))[:k]
        vals[r], inds[r] = x[r, c[o]], c[o]
    inds[np.isneginf(vals)] = -1
    return vals, inds


def brute_topk(logits, k, tags, want_any, want_all, ex_lists):
    """The same answer by a per-row, per-column loop (the oracle's own check)."""
    B, V = logits.shape
    vals = np.full((B, k), -np.inf, dtype=np.float32)
    inds = np.full((B, k), -1, dtype=np.int64)
    for r in range(B):
        a, l = int(want_any[r]), int(want_all[r])
        ok = []
        for c in range(V):
            t = int(tags[c])
            if a != 0 and (t & a) == 0:
                continue
            if (t & l) != l:
                continue
            if ex_lists is not None and c in set(int(x) for x in ex_lists[r]):
                continue
            if logits[r, c] == -np.inf:
                continue
            ok.append((-float(logits[r, c]), c))
        ok.sort()
        for j, (nv, c) in enumerate(ok[:k]):
            vals[r, j], inds[r, j] = -nv, c
    return vals, inds


def random_tags(rng, V):
    """bit b set on a column with probability 2^-(1 + b % 6)"""
    t = np.zeros(V, dtype=np.uint32)
    for b in range(32):
        t |= (rng.random(V) < 2.0 ** -(1 + b % 6)).astype(np.uint32) << np.uint32(b)
    return t


def random_words(rng, B, zero_every=17):
    """Row words whose eligible share spans about 50 % (any = one bit of probability 1/2) down to about 2 %
    (all = bits of probability 1/2 x 1/4 x 1/8 ... ); every zero_every-th row is (0, 0)."""
    any_w = np.zeros(B, dtype=np.uint32)
    all_w = np.zeros(B, dtype=np.uint32)
    for r in range(B):
        kind = r % 5
        if kind == 0:
            any_w[r] = 1 << (6 * int(rng.integers(0, 5)))                # one bit of p = 1/2: 50 %
        elif kind == 1:
            all_w[r] = 1 << (1 + 6 * int(rng.integers(0, 5)))            # p = 1/4
        elif kind == 2:
            any_w[r] = (1 << 4) | (1 << 5) | (1 << 11)                   # three rare bits: ~ 8 %
        elif kind == 3:
            all_w[r] = (1 << 0) | (1 << 2)                               # 1/2 x 1/8: ~ 6 %
            any_w[r] = (1 << 1) | (1 << 7)                               # ... x 7/16: ~ 2.7 %
        else:
            all_w[r] = 1 << 6                                            # 1/2
            any_w[r] = (1 << 4) | (1 << 5)                               # x (1/32 + 1/64): ~ 2.3 %
    any_w[::zero_every] = 0
    all_w[::zero_every] = 0
    return any_w, all_w


def i32(words):
    """uint32 words -> the int32 bit patterns the device holds"""
    return np.ascontiguousarray(np.asarray(words).astype(np.uint32)).view(np.int32)
