"""TEST DOUBLE: the numpy compute double of tests/numpy_backend_w2v.py plus the two stages arx.dist's similar_items asks
of a backend (HipBackend.gather_rows_unit / shard_similar) and the view's het_rows_range double of
test_sharded_het_view_cpu.py.  Lives in tests/ on purpose: the package has no CPU path."""
import numpy as np

from numpy_backend import _n
from numpy_backend_w2v import NumpyW2VBackend
from test_sharded_het_view_cpu import _backend as _view_backend


def _inv_norm(e):
    s = (e ** 2).sum(1)
    with np.errstate(divide='ignore'):
        return np.where(s > 0, 1.0 / np.sqrt(s), 0.0)


class NumpySimilarBackend(NumpyW2VBackend):
    het_rows_range = type(_view_backend()).het_rows_range

    def gather_rows_unit(self, E, rows, out):
        """out[r] = E[rows[r]] / |E[rows[r]]|; zeros for rows[r] < 0 and for a zero row (float64, stored as float32)."""
        e, r = _n(E).astype(np.float64), _n(rows).astype(np.int64)
        assert len(r) == 0 or r.max() < e.shape[0]
        rr = np.maximum(r, 0)
        _n(out)[...] = np.where((r >= 0)[:, None], e[rr] * _inv_norm(e)[rr][:, None], 0.0)

    def shard_similar(self, Q, E, k, self_cols, values, indices):
        """values / indices [B, k]: the k best of (Q . E^T) * (1 / |E_j|) by (value desc, local column asc), the row's
        self column (a column of [0, V); anything else: none) left out; (-inf, -1) where fewer than k are left."""
        q, e = _n(Q).astype(np.float64), _n(E).astype(np.float64)
        B, V = q.shape[0], e.shape[0]
        x = (q @ e.T) * _inv_norm(e)[None, :] + 0.0
        if self_cols is not None:
            for r, c in enumerate(_n(self_cols).astype(np.int64)):
                if 0 <= c < V:
                    x[r, c] = -np.inf
        vals = np.full((B, k), -np.inf)
        idx = np.full((B, k), -1, dtype=np.int64)
        for r in range(B):
            o = np.lexsort((np.arange(V), -x[r]))[:k]
            vals[r, :len(o)], idx[r, :len(o)] = x[r, o], o
        idx[np.isneginf(vals)] = -1
        _n(values)[...] = vals.astype(np.float32)
        _n(indices)[...] = idx.astype(np.int32)
