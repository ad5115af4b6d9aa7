"""TEST DOUBLE: the numpy compute double of tests/numpy_backend.py plus what a `loss` other than 'mw' asks of a
backend of arx.dist.ShardedHMF -- the sampled loss with a kind ('mce'), the slot-indirect pair loss and the
rank-select negative draw -- and the fp64 statement of a pair step on the global batch that the sharded tests compare
with.  Lives in tests/ on purpose: the package has no CPU path."""
import numpy as np

from numpy_backend import NumpyBackend, _n
from test_bpr_cpu import rank_select

MCE_SAT = 64.0          # (csrc/common.h kMceSat, oracle/ref_graph.py MCE_SAT)


class NumpyPairBackend(NumpyBackend):
    def loss_mw_fused_pos(self, logits, U, T, tb, urows, ptr, items, i2s, bl, dl, t_out, dt, dU, dT, gscale,
                          kind='mw'):
        if kind == 'mw':
            return super().loss_mw_fused_pos(logits, U, T, tb, urows, ptr, items, i2s, bl, dl, t_out, dt, dU, dT,
                                             gscale)
        assert kind == 'mce'
        # arx_loss_mce_fused_pos: log(1 + sum_s m_rs exp(min(x_rs - t_r, 64))) with the positives masked out
        self.dot_score(U, T, tb, t_out)
        x = _n(logits).astype(np.float64)
        t = _n(t_out).astype(np.float64)[:, None]
        B, S = x.shape
        mask = np.ones((B, S), dtype=bool)
        p, it, m = _n(ptr), _n(items), _n(i2s)
        for r, u in enumerate(_n(urows)):
            for v in it[p[u]:p[u + 1]]:
                if m[v] >= 0:
                    mask[r, m[v]] = False
        x = np.minimum(x, t + MCE_SAT)
        mx = np.maximum(np.where(mask, x, -np.inf).max(1, keepdims=True), t)
        ex = np.where(mask, np.exp(x - mx), 0.0)
        z = np.exp(t - mx)[:, 0] + ex.sum(1)
        _n(bl)[...] = mx[:, 0] - t[:, 0] + np.log(z)
        d = gscale * ex / z[:, None]
        g = -d.sum(1)
        _n(dl)[...] = d
        _n(dt)[...] = g
        _n(dU)[...] = g[:, None] * _n(T).astype(np.float64)
        _n(dT)[...] = g[:, None] * _n(U).astype(np.float64)

    def pair_loss_slots(self, U, R, pos_slot, neg_slot, kind, gscale, pos_score, neg_score, bl, dU, dR, counts):
        """arx_pair_loss_slots: rows of dR that no slot names keep what they held; columns behind d too."""
        u, rr = _n(U).astype(np.float64), _n(R).astype(np.float64)
        d = u.shape[1]
        ps_, ns_ = _n(pos_slot).astype(np.int64), _n(neg_slot).astype(np.int64)
        named = np.concatenate([ps_, ns_[ns_ >= 0]])
        assert len(np.unique(named)) == len(named), "a slot named twice"
        assert named.min() >= 0 and named.max() < rr.shape[0]
        live = ns_ >= 0
        P = rr[ps_]
        N = np.where(live[:, None], rr[np.maximum(ns_, 0)], 0.0)
        ps = (u * P[:, :d]).sum(1) + P[:, d]
        ns = (u * N[:, :d]).sum(1) + N[:, d]
        x = ns - ps
        if kind == 'bpr':
            loss, g = np.logaddexp(0.0, x), 1.0 / (1.0 + np.exp(-x))
        else:
            assert kind == 'bpr-hinge'
            loss, g = np.maximum(1.0 + x, 0.0), (1.0 + x > 0).astype(np.float64)
        c = gscale * g * live
        _n(pos_score)[...] = ps
        _n(neg_score)[...] = ns
        _n(bl)[...] = loss * live
        _n(dU)[...] = c[:, None] * (N[:, :d] - P[:, :d])
        g_out = _n(dR)
        g_out[ps_, :d] = -c[:, None] * u
        g_out[ps_, d] = -c
        g_out[ns_[live], :d] = (c[:, None] * u)[live]
        g_out[ns_[live], d] = c[live]
        _n(counts)[...] = [int(np.sign(x[live]).sum()), int(live.sum())]

    def neg_draw_uniform(self, urows, ex_ptr, ex_cols, V, seed, counter, out):
        """One item outside the row's user's sorted, unique list, uniform by rank-select (the statement of
        arx_neg_draw_uniform; the random numbers are numpy's, keyed by (seed, counter)); -1 for a full list."""
        ptr, cols = _n(ex_ptr), _n(ex_cols)
        rng = np.random.default_rng([int(seed) & 0xFFFFFFFF, int(seed) >> 32, int(counter)])
        o = _n(out)
        for r, u in enumerate(_n(urows)):
            lst = cols[ptr[u]:ptr[u + 1]].astype(np.int64)
            assert (np.diff(lst) > 0).all(), "the draw needs sorted, unique lists"
            n_elig = int(V) - len(lst)
            k = int(rng.integers(0, 1 << 32)) * n_elig >> 32
            o[r] = rank_select(lst, k) if n_elig > 0 else -1


class PairRef(object):
    """'bpr' / 'bpr-hinge' on the global batch in fp64: x = neg_score - pos_score, the
    mean over ALL rows (a void row -- negative < 0 -- adds 0 and no gradient), duplicate rows merged, one Adagrad
    update per table row."""

    def __init__(self, tables, lr, acc0=0.1):
        f = lambda a: np.array(a, dtype=np.float64)
        self.U, self.I, self.b = f(tables['user']), f(tables['item']), f(tables['item_bias']).reshape(-1)
        self.AU, self.AI, self.Ab = (np.full_like(t, acc0) for t in (self.U, self.I, self.b))
        self.lr = float(lr)

    def step(self, users, pos, neg, kind):
        users, pos, neg = (np.asarray(a, dtype=np.int64) for a in (users, pos, neg))
        live = neg >= 0
        ng = np.maximum(neg, 0)
        u, P, N = self.U[users], self.I[pos], self.I[ng] * live[:, None]
        ps = (u * P).sum(1) + self.b[pos]
        ns = ((u * N).sum(1) + self.b[ng]) * live
        x = ns - ps
        if kind == 'bpr':
            bl, g = np.logaddexp(0.0, x), 1.0 / (1.0 + np.exp(-x))
        else:
            bl, g = np.maximum(1.0 + x, 0.0), (1.0 + x > 0).astype(np.float64)
        c = g * live / len(users)
        gU, gI, gb = np.zeros_like(self.U), np.zeros_like(self.I), np.zeros_like(self.b)
        np.add.at(gU, users, c[:, None] * (N - P))
        np.add.at(gI, pos, -c[:, None] * u)
        np.add.at(gb, pos, -c)
        np.add.at(gI, ng[live], (c[:, None] * u)[live])
        np.add.at(gb, ng[live], c[live])
        for w, a, gr in ((self.U, self.AU, gU), (self.I, self.AI, gI), (self.b, self.Ab, gb)):
            a += gr * gr                                    # (a row without gradient: + 0, - 0)
            w -= self.lr * gr / np.sqrt(a)
        auc = 0.5 - 0.5 * np.sign(x[live]).mean() if live.any() else 0.5
        return dict(loss=float((bl * live).mean()), ps=ps, ns=ns, x=x, live=live, auc=float(auc))

    def compare(self, got, rtol, atol):
        for name, want in (('user', self.U), ('user/Adagrad', self.AU), ('item', self.I), ('item/Adagrad', self.AI),
                           ('item_bias', self.b), ('item_bias/Adagrad', self.Ab)):
            np.testing.assert_allclose(got[name].reshape(want.shape), want, rtol=rtol, atol=atol, err_msg=name)
