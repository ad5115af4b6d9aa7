"""A numpy compute double of the two recommend stages of arx.dist.ShardedHMF whose shard_topk knows item tags
(HipBackend.shard_topk's tags=): for the gloo tests without a GPU."""
import numpy as np

from numpy_backend import NumpyBackend
import tags_oracle as T


def _np(t):
    return t if isinstance(t, int) else t.numpy()


class TagsRecBackend(NumpyBackend):
    def shard_topk(self, U, E, bias, k, ex, values, indices, lse=None, tags=None):
        u, e, b = (t.numpy().astype(np.float64) for t in (U, E, bias))
        x = u @ e.T + b[None, :]
        B, V = x.shape
        if ex is not None:
            keys, key_rows, ptr, cols = (_np(t) for t in ex)
            for r in range(B):
                key = int(keys[r % key_rows])
                if key >= 0:
                    x[r, cols[ptr[key]:ptr[key + 1]].astype(np.int64)] = -np.inf
        if tags is not None:
            col_tags, want_any, want_all, want_rows = (_np(t) for t in tags)
            assert len(col_tags) == V and col_tags.dtype == np.int32
            rows = np.arange(B) % want_rows
            ok = T.eligible(col_tags.view(np.uint32), want_any.view(np.uint32)[rows], want_all.view(np.uint32)[rows])
            x[~ok] = -np.inf
        vals = np.full((B, k), -np.inf)
        idx = np.full((B, k), -1, dtype=np.int64)
        for r in range(B):
            o = np.lexsort((np.arange(V), -x[r]))[:k]
            vals[r, :len(o)], idx[r, :len(o)] = x[r, o], o
        idx[np.isneginf(vals)] = -1
        values.numpy()[...] = vals.astype(np.float32)
        indices.numpy()[...] = idx.astype(np.int32)

    def topk_merge_shards(self, v, c, vo, io):
        vv, cc = v.numpy().astype(np.float64), c.numpy().astype(np.int64)
        W, B, k = vv.shape
        gid = cc * W + np.arange(W)[:, None, None]
        for r in range(B):
            x, g, ok = vv[:, r].ravel(), gid[:, r].ravel(), cc[:, r].ravel() >= 0
            x, g = x[ok], g[ok]
            o = np.lexsort((g, -x))[:k]
            rv = np.full(k, -np.inf)
            ri = np.full(k, -1, dtype=np.int64)
            rv[:len(o)], ri[:len(o)] = x[o], g[o]
            ri[np.isneginf(rv)] = -1
            vo.numpy()[r], io.numpy()[r] = rv.astype(np.float32), ri.astype(np.int32)
