"""A numpy compute double of the stages arx.dist.ShardedHMF.list_logprob adds to those of recommend_sampled
(tests/numpy_backend_sample.py): the per-shard prepare (HipBackend.shard_list_prepare: arx_list_logp_prepare_shard), the
owner's merge (arx_list_logp_merge_shards) and the stamp -- for the gloo tests without a GPU.  prepare_shard() is also
the oracle of the kernel's four outputs in tests/test_sharded_list_logprob_gpu.py."""
import numpy as np
import torch

from numpy_backend_sample import SampleRecBackend
from numpy_backend_tags import _np

OK, EMPTY, RANGE, EXCLUDED, TAGS, REPEAT, NOSCORE = range(7)


def prepare_shard(lists, V_global, W, s, ex=None, tags=None):
    """What arx_list_logp_prepare_shard writes on shard s of W, from include/arx_list_logp_shard.h: lists int [B, k] of
    global ids; ex: (row_keys, key_rows, ex_ptr, ex_cols of LOCAL columns) or None; tags: (col_tags of the shard's rows,
    want_any, want_all, want_rows) or None.  -> (clean local columns, codes, pk_cols, pk_slot), each int32 [B, k]."""
    lists = np.asarray(lists, dtype=np.int64)
    B, k = lists.shape
    clean = np.full((B, k), -1, dtype=np.int64)
    codes = np.zeros((B, k), dtype=np.int32)
    for r in range(B):
        mine = set()
        if ex is not None:
            keys, key_rows, ptr, cols = ex
            key = int(keys[r % key_rows])
            if key >= 0:
                mine = set(int(c) for c in cols[ptr[key]:ptr[key + 1]])
        seen = set()
        for t in range(k):
            v = int(lists[r, t])
            if v == -1:
                codes[r, t] = EMPTY
            elif v < 0 or v >= V_global:
                codes[r, t] = RANGE
            elif v % W != s:
                continue                                             # another shard's: no pick, nothing to say
            else:
                c = v // W
                if c in mine:
                    codes[r, t] = EXCLUDED
                    continue
                if tags is not None:
                    col_tags, want_any, want_all, want_rows = tags
                    w = int(np.uint32(col_tags[c]))
                    wa, wl = int(np.uint32(want_any[r % want_rows])), int(np.uint32(want_all[r % want_rows]))
                    if (wa != 0 and (w & wa) == 0) or (w & wl) != wl:
                        codes[r, t] = TAGS
                        continue
                if c in seen:
                    codes[r, t] = REPEAT
                    continue
                seen.add(c)
                clean[r, t] = c
    pk_cols = np.empty((B, k), dtype=np.int64)
    pk_slot = np.empty((B, k), dtype=np.int64)
    for r in range(B):                                               # arx_sample_logp_sort: (column as unsigned, slot)
        o = np.lexsort((np.arange(k), clean[r] & 0xffffffff))
        pk_cols[r], pk_slot[r] = clean[r][o], o
    return clean.astype(np.int32), codes, pk_cols.astype(np.int32), pk_slot.astype(np.int32)


def merge_shards(lists, V_global, codes):
    """What arx_list_logp_merge_shards writes: lists int [B, k] global ids, codes [W, B, k] -> (clean, why) int32."""
    lists = np.asarray(lists, dtype=np.int64)
    W = codes.shape[0]
    B, k = lists.shape
    inr = (lists >= 0) & (lists < V_global)
    own = np.where(inr, lists % W, 0)
    why = np.take_along_axis(codes, own[None], 0)[0].astype(np.int32)
    why[~inr] = RANGE
    why[lists == -1] = EMPTY
    return np.where(why == OK, lists, -1).astype(np.int32), why


class ListRecBackend(SampleRecBackend):
    def shard_list_prepare(self, lists, n_items, world, shard, V, ex, tags, codes):
        ex_n = tuple(_np(t) for t in ex) if ex is not None else None
        tags_n = tuple(_np(t) for t in tags) if tags is not None else None
        ls = lists.numpy()
        clean, cd, _, _ = prepare_shard(ls, n_items, world, shard, ex_n, tags_n)
        codes.numpy()[...] = cd
        # the handle: this shard's surviving entries as GLOBAL ids -- what the double's shard_rest_mass takes as picks
        return torch.from_numpy(np.where(clean >= 0, ls, -1).astype(np.int32))

    def shard_rest_mass(self, U, E, bias, ex, picks, world, shard, sample, packed, P_max, tags=None, prepared=None):
        return super().shard_rest_mass(U, E, bias, ex, picks if prepared is None else prepared, world, shard, sample,
                                       packed, P_max, tags=tags)

    def list_logp_merge_shards(self, lists, n_items, codes, clean, why):
        c, w = merge_shards(lists.numpy(), n_items, codes.numpy())
        clean.numpy()[...] = c
        why.numpy()[...] = w

    def list_logp_stamp(self, clean, values, why, logp):
        c, v, w, lp = clean.numpy(), values.numpy(), why.numpy(), logp.numpy()
        w[(c >= 0) & np.isneginf(v)] = NOSCORE
        lp[w >= RANGE] = -np.inf
        v[w >= RANGE] = -np.inf
