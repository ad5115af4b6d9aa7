"""TEST DOUBLE: the numpy compute double of the sharded tests plus the stages arx.dist.ShardedHMF.score_items asks of a
backend (HipBackend.slate_scores / slate_merge_shards / slate_order); shard_route is NumpyBackend's.  Lives in tests/
on purpose: the package has no CPU path."""
import numpy as np

from numpy_backend import _n
from numpy_backend_w2v import NumpyW2VBackend
import slate_oracle as SO


class SlateBackend(NumpyW2VBackend):
    def slate_scores(self, U, E, bias, local_cols, out):
        _n(out)[...] = SO.scores(_n(U), _n(E), None if bias is None else _n(bias), _n(local_cols)).astype(np.float32)

    def slate_merge_shards(self, parts, out):
        p = _n(parts)
        assert p.ndim == 3 and 1 <= p.shape[0] <= 64
        assert ((~np.isneginf(p)).sum(0) <= 1).all(), "a slot scored by two shards"
        _n(out)[...] = p.max(0)

    def slate_order(self, scores, cand, k, values, pos, ids):
        i, v = SO.order(_n(scores), _n(cand), k)
        _n(ids)[...] = i
        _n(values)[...] = v
