"""TEST DOUBLE: the numpy compute double of tests/numpy_backend_pair.py plus the two slot-addressed window calls that
arx.dist.ShardedW2V asks of a backend (arx_window_slots_fwd / _bwd), and the recommend / evaluate stage doubles of the
sharded serving tests.  Lives in tests/ on purpose: the package has no CPU path."""
import numpy as np

from numpy_backend import _n
from numpy_backend_pair import NumpyPairBackend
from test_sharded_eval_cpu import _backend as _eval_backend
from test_sharded_recommend_cpu import _backend as _rec_backend


class NumpyW2VBackend(NumpyPairBackend, type(_rec_backend()), type(_eval_backend())):
    def window_slots_fwd(self, R, slots, n, scale, base, base_scale, out):
        """out[b] = base_scale * base[b] + scale * sum_t R[slots[t * mb + b]] (ascending t)."""
        r, s = _n(R).astype(np.float64), _n(slots).astype(np.int64)
        mb = _n(out).shape[0]
        assert len(s) == n * mb and (len(s) == 0 or (s.min() >= 0 and s.max() < r.shape[0]))
        assert len(np.unique(s)) == len(s), "a slot named twice"
        acc = np.zeros((mb, r.shape[1]), dtype=np.float64)
        for t in range(n):
            acc += r[s[t * mb:(t + 1) * mb]]
        x = scale * acc
        if base is not None:
            x = x + base_scale * _n(base).astype(np.float64)
        _n(out)[...] = x

    def window_slots_bwd(self, dX, slots, n, scale, base_scale, dbase, acc_dbase, dR):
        """dbase[b] (+)= base_scale * dX[b]; dR[slots[t * mb + b]] = scale * dX[b]; other rows of dR are kept."""
        g, s = _n(dX).astype(np.float64), _n(slots).astype(np.int64)
        mb = g.shape[0]
        assert len(s) == n * mb and (len(s) == 0 or (s.min() >= 0 and s.max() < _n(dR).shape[0]))
        assert len(np.unique(s)) == len(s), "a slot named twice"
        u = base_scale * g
        _n(dbase)[...] = (_n(dbase) + u) if acc_dbase else u
        for t in range(n):
            _n(dR)[s[t * mb:(t + 1) * mb]] = scale * g
