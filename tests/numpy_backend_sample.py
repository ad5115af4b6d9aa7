"""A numpy compute double of the stages of arx.dist.ShardedHMF.recommend_sampled(sample_temperature=, return_logprob=):
the keyed shard top-k (HipBackend.shard_topk's sample=), the owner's strip, the shard's rest-mass pass and the finish over
the W slabs -- for the gloo tests without a GPU.  The noise is tests/sample_oracle.py's: bits(seed, rows = GLOBAL user
ids, cols = GLOBAL item ids), g = float32(gumbel64), key = float32(float64(tau) g + score)."""
import numpy as np

from numpy_backend_tags import TagsRecBackend, _np
import sample_oracle as SM
import tags_oracle as T

FLT_MAX = float(np.finfo(np.float32).max)


def seed_of(words):
    w = np.asarray(words).astype(np.int64) & 0xffffffff
    return int(w[0]) | (int(w[1]) << 32)


def noise(seed, users, gids):
    """float32 [len(users), len(gids)]; a negative user id (a padding row) gets a row of zeros (its tau counts as 0)"""
    users = np.asarray(users, dtype=np.int64)
    g = np.zeros((len(users), len(gids)), dtype=np.float32)
    ok = users >= 0
    if ok.any() and len(gids):
        g[ok] = SM.gumbel64(SM.bits(seed, users[ok], np.asarray(gids, dtype=np.uint32))).astype(np.float32)
    return g


class SampleRecBackend(TagsRecBackend):
    def _masked(self, U, E, bias, ex, tags):
        u, e, b = (t.numpy().astype(np.float64) for t in (U, E, bias))
        x = (u @ e.T + b[None, :]).astype(np.float32)               # (dyadic tables: exact)
        B, V = x.shape
        if ex is not None:
            keys, key_rows, ptr, cols = (_np(t) for t in ex)
            for r in range(B):
                key = int(keys[r % key_rows])
                if key >= 0:
                    x[r, cols[ptr[key]:ptr[key + 1]].astype(np.int64)] = -np.inf
        if tags is not None:
            col_tags, want_any, want_all, want_rows = (_np(t) for t in tags)
            rows = np.arange(B) % want_rows
            ok = T.eligible(col_tags.view(np.uint32), want_any.view(np.uint32)[rows], want_all.view(np.uint32)[rows])
            x[~ok] = -np.inf
        return x

    def shard_topk(self, U, E, bias, k, ex, values, indices, lse=None, tags=None, sample=None):
        if sample is None:
            return super().shard_topk(U, E, bias, k, ex, values, indices, lse=lse, tags=tags)
        tau, tau_rows, words, W, s, users = (_np(t) for t in sample)
        x = self._masked(U, E, bias, ex, tags)
        B, V = x.shape
        assert tau_rows == B and len(users) == B
        tau = np.where(users >= 0, tau, 0).astype(np.float32)
        ky = SM.keys(x, noise(seed_of(words), users, np.arange(V) * W + s), tau)
        vals = np.full((B, k), -np.inf, dtype=np.float32)
        idx = np.full((B, k), -1, dtype=np.int64)
        for r in range(B):
            o = np.lexsort((np.arange(V), -ky[r].astype(np.float64)))[:k]
            vals[r, :len(o)], idx[r, :len(o)] = ky[r, o], o
        idx[np.isneginf(vals)] = -1
        values.numpy()[...] = vals                                   # the KEYS: not stripped
        indices.numpy()[...] = idx.astype(np.int32)

    def sample_strip(self, values, indices, sample):
        tau, tau_rows, words, mul, add, users = (_np(t) for t in sample)
        v, ids = values.numpy(), indices.numpy()
        assert (mul, add) == (1, 0)
        seed = seed_of(words)
        for r in range(v.shape[0]):
            live = ids[r] >= 0
            v[r, ~live] = -np.inf
            if users[r] < 0 or tau[r] == 0 or not live.any():
                continue
            g = noise(seed, [users[r]], ids[r][live])[0]
            v[r, live] = (v[r, live].astype(np.float64) - np.float64(tau[r]) * g.astype(np.float64)).astype(np.float32)

    def shard_mass_parts(self, B, V, d):
        return 1 + V % 3                                             # (uneven shards pad to the largest)

    def shard_rest_mass(self, U, E, bias, ex, picks, world, shard, sample, packed, P_max, tags=None):
        tau = _np(sample[0])
        x = self._masked(U, E, bias, ex, tags).astype(np.float64)
        B, V = x.shape
        pk = picks.numpy().astype(np.int64)
        k = pk.shape[1]
        P = self.shard_mass_parts(B, V, 0)
        assert P <= P_max and tuple(packed.shape) == (B, 2 * P_max + k)
        out = packed.numpy()
        out[:, :P_max], out[:, P_max:2 * P_max], out[:, 2 * P_max:] = -FLT_MAX, 0.0, -np.inf
        edges = np.linspace(0, V, P + 1).astype(np.int64)
        for r in range(B):
            rest = x[r].copy()
            for t in range(k):
                if pk[r, t] >= 0 and pk[r, t] % world == shard:
                    c = pk[r, t] // world
                    out[r, 2 * P_max + t] = x[r, c]
                    rest[c] = -np.inf
            t_r = float(tau[r]) if tau[r] > 0 else 1.0
            for p in range(P):
                seg = rest[edges[p]:edges[p + 1]]
                seg = seg[seg > -np.inf]
                if len(seg):
                    out[r, p] = seg.max()
                    out[r, P_max + p] = np.exp((seg - seg.max()) / t_r).sum()

    def sample_logp_finish_shards(self, indices, recv, P_max, sample, logp, values):
        tau = _np(sample[0])
        ids, rv = indices.numpy().astype(np.int64), recv.numpy().astype(np.float64)
        W, B, wd = rv.shape
        k = ids.shape[1]
        lp, vals = logp.numpy(), values.numpy()
        lp[...] = 0
        for r in range(B):
            sc = np.array([rv[ids[r, t] % W, r, 2 * P_max + t] if ids[r, t] >= 0 else -np.inf for t in range(k)])
            vals[r] = sc
            if tau[r] == 0:
                continue
            m, S = rv[:, r, :P_max].ravel(), rv[:, r, P_max:2 * P_max].ravel()
            with np.errstate(divide='ignore'):
                run = -np.inf
                for mm, ss in zip(m, S):
                    if ss > 0:
                        run = np.logaddexp(run, mm / tau[r] + np.log(ss))
            for t in range(k - 1, -1, -1):
                if sc[t] > -np.inf:
                    run = np.logaddexp(run, sc[t] / tau[r])
                    lp[r, t] = sc[t] / tau[r] - run
