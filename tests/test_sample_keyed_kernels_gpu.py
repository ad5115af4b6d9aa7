"""The keyed kernels of include/arx_sample_shard.h on the GPU, with no process group: the Gumbel add / strip / fused
filter fed other noise rows and columns (noise column = column * col_mul + col_add, noise row = noise_rows[row]), and
the propensities' finish over W shard slabs.  Device against device where the un-keyed entry is the reference (exact),
the oracles of tests/sample_oracle.py and tests/recommend_logprob_oracle.py elsewhere."""
import numpy as np
import pytest

import recommend_logprob_oracle as RL
import sample_oracle as S
import tags_oracle as T
from test_recommend_exclude_gpu import _Rig
from test_recommend_sample_gpu import TAUS, _dev_noise, _dev_sample, _dev_tags, _taus

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


def _keyed(dev, tau, seed, mul, add, rows=None):
    import torch
    nr = None if rows is None else torch.from_numpy(np.asarray(rows, dtype=np.int32)).to(dev)
    return _dev_sample(dev, tau, seed) + (mul, add, nr)


def _keyed_noise(dev, seed, rows, ncols, mul, add, col0=0):
    """g [len(rows), ncols] float32 of the noise rows `rows` and the noise columns (col0 + c) * mul + add, as the
    device computes it: the keyed add of tau = 1 on zeros."""
    import torch
    from arx import ops
    z = torch.zeros((len(rows), ncols), dtype=torch.float32, device=dev)
    ops.topk_gumbel_add(z, col0, _keyed(dev, np.ones(len(rows), dtype=np.float32), seed, mul, add, rows))
    return z.cpu().numpy()


def _logits(rng, B, V):
    x = rng.standard_normal((B, V)).astype(np.float32)
    x[rng.random((B, V)) < 0.01] = -np.inf
    return x


# ---------------------------------------------------------------- 1. device against device, exact
def test_keyed_add_equals_the_unkeyed_entry(dev):
    import torch
    from arx import ops
    B, n, seed = 50, 1000, 4
    rng = np.random.default_rng(0)
    tau = TAUS[rng.integers(0, 4, B)]
    tau[[0, 7]] = 0
    x = _logits(rng, B, n)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    plain = _dev_sample(dev, tau, seed)

    def run(a, col0, sample):
        t = up(a)
        ops.topk_gumbel_add(t, col0, sample)
        return t.cpu().numpy()
    ref = run(x, 0, plain)
    assert (ref != x)[tau > 0].any()
    # (1, 0, NULL): the un-keyed entry, bit for bit
    np.testing.assert_array_equal(run(x, 0, plain + (1, 0, None)), ref)
    np.testing.assert_array_equal(run(x, 0, _keyed(dev, tau, seed, 1, 0, np.arange(B))), ref)
    # (W, s) = (3, 2) over n columns: the un-keyed add over 3 n columns, at the columns 2::3
    wide = np.zeros((B, 3 * n), dtype=np.float32)
    wide[:, 2::3] = x
    ref3 = run(wide, 0, plain)[:, 2::3]
    np.testing.assert_array_equal(run(x, 0, plain + (3, 2, None)), ref3)
    # col0 != 0, a strided view: columns [col0, col0 + m) of the shard are the global columns 3 (col0 + c) + 2
    col0, m = 333, 500
    full = up(x)
    ops.topk_gumbel_add(full[:, col0:col0 + m], col0, plain + (3, 2, None))
    got = full.cpu().numpy()
    np.testing.assert_array_equal(got[:, col0:col0 + m], ref3[:, col0:col0 + m])
    np.testing.assert_array_equal(got[:, :col0], x[:, :col0])
    np.testing.assert_array_equal(got[:, col0 + m:], x[:, col0 + m:])
    # noise_rows = a permutation: row r draws the noise of row perm[r]
    perm = rng.permutation(B)
    tau_p, x_p = np.empty_like(tau), np.empty_like(x)
    tau_p[perm], x_p[perm] = tau, x
    ref_p = run(x_p, 0, _dev_sample(dev, tau_p, seed))
    np.testing.assert_array_equal(run(x, 0, _keyed(dev, tau, seed, 1, 0, perm)), ref_p[perm])
    # a negative noise row (a padding row): untouched, whatever its tau
    rows = np.arange(B)
    rows[[3, 9]] = -1
    got = run(x, 0, _keyed(dev, np.where(tau == 0, 1, tau).astype(np.float32), seed, 3, 2, rows))
    np.testing.assert_array_equal(got[[3, 9]], x[[3, 9]])
    assert (got[4] != x[4]).any()


def test_keyed_strip_inverts_keyed_add(dev):
    import torch
    from arx import ops
    B, V, k, seed, W, s = 60, 2000, 40, 8, 3, 2
    rng = np.random.default_rng(1)
    users = rng.integers(0, 2 ** 31, B)
    users[5] = -1
    tau = TAUS[rng.integers(0, 4, B)]
    tau[[0, 7]] = 0
    score = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    kt = torch.from_numpy(score.copy()).to(dev)
    sample = _keyed(dev, tau, seed, W, s, users)
    ops.topk_gumbel_add(kt, 0, sample)
    ky = kt.cpu().numpy()
    idx = np.stack([rng.choice(V, k, replace=False) for _ in range(B)]).astype(np.int32)
    idx[rng.random((B, k)) < 0.1] = -1
    vals = np.take_along_axis(ky, np.maximum(idx, 0), 1)
    dv = torch.from_numpy(np.ascontiguousarray(vals)).to(dev)
    ops.topk_gumbel_strip(dv, torch.from_numpy(idx).to(dev), sample)       # local columns, the shard's map
    got = dv.cpu().numpy()
    ok = idx >= 0
    assert np.isneginf(got[~ok]).all()
    sc = np.take_along_axis(score, np.maximum(idx, 0), 1)
    assert (np.abs(got.astype(np.float64) - sc)[ok] <= S.strip_bound(vals, sc)[ok]).all()
    still = (tau == 0) | (users < 0)
    np.testing.assert_array_equal(got[still][ok[still]], vals[still][ok[still]])   # tau = 0 / a padding row: left alone
    np.testing.assert_array_equal(ky[still], score[still])
    # the owner's form: GLOBAL ids with (1, 0) read the same noise
    dv = torch.from_numpy(np.ascontiguousarray(vals)).to(dev)
    gid = np.where(ok, idx * W + s, -1).astype(np.int32)
    ops.topk_gumbel_strip(dv, torch.from_numpy(gid).to(dev), _keyed(dev, tau, seed, 1, 0, users))
    np.testing.assert_array_equal(dv.cpu().numpy(), got)


# ---------------------------------------------------------------- 2. against the oracle
def test_keyed_noise_against_the_oracle(dev):
    """The method of test_gumbel_add_kernel at the noise rows 0 and 2^31 - 1 and the strided columns 3 c + 2."""
    V, seed, W, s = 3000, 1, 3, 2
    rows = [0, 2 ** 31 - 1, 12345]
    x = S.bits(seed, rows, np.arange(V, dtype=np.uint32) * np.uint32(W) + np.uint32(s))
    g = _keyed_noise(dev, seed, rows, V, W, s)
    assert np.isfinite(g).all()
    sure = S.recoverable(x)
    assert sure.mean() > 0.2
    np.testing.assert_array_equal(S.m_of_g(g)[sure], (x >> np.uint32(9))[sure])
    g64 = S.gumbel64(x)
    own = np.abs(S.gumbel32(x).astype(np.float64) - g64).max()
    got = np.abs(g.astype(np.float64) - g64).max()
    print("keyed g against float64: device %.3g, numpy float32 %.3g" % (got, own))
    assert got <= 4 * own
    # the largest noise column the entry takes: (col0 + c) * 3 + 2 just below 2^31
    col0 = (2 ** 31 - 1 - s) // W - 7
    g = _keyed_noise(dev, seed, rows, 8, W, s, col0=col0)
    xb = S.bits(seed, rows, (np.arange(col0, col0 + 8, dtype=np.uint64) * W + s).astype(np.uint32))
    assert np.abs(g.astype(np.float64) - S.gumbel64(xb)).max() <= 4 * own


# ---------------------------------------------------------------- 3. TopKScan with a keyed sample
def _seed_for(dev, users, W, s, logits, tau, k, base, **filt):
    """The first seed >= base of 8 whose ORACLE (numpy alone) leaves <= 1 % of the rows with a k-th / (k + 1)-th key
    inside the strip bound; the noise: the device's own, at the keyed rows and columns."""
    B, V = logits.shape
    for seed in range(base, base + 8):
        g = _keyed_noise(dev, seed, users, V, W, s)
        kv, sc, ei, ky = S.sample_topk(logits, g, tau, k, **filt)
        close = S.close_rows(ky, kv, sc, k)
        if close.mean() <= 0.01:
            return seed, kv, sc, ei, ky, close
    raise AssertionError("no seed in [%d, %d) with <= 1 %% close rows" % (base, base + 8))


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("k", [1, 30])
@pytest.mark.parametrize("mode", ["plain", "ex_tags"])
def test_topk_scan_keyed_smallest_shapes(dev, d, k, mode):
    """The fused filter's smallest shapes (a first chunk of 256, five full tiles, a ragged one of 17 columns, two row
    panels) as shard 2 of 3 with random user ids as noise rows: fused (no overflow) and chunked give the oracle's ids
    on the device's own logits and noise; the keys come back unstripped; tau = 0 rows equal the plain scan."""
    import torch
    from arx.topk import TopKScan
    B, V, W, s = 130, 256 + 5 * 64 + 17, 3, 2
    rig = _Rig(B, V, d, seed=7 * d + k)
    rng = np.random.default_rng(d + k)
    tau = _taus(rng, B)
    users = rng.integers(0, 2 ** 31, B)
    filt, targs, ex = {}, None, None
    if mode == 'ex_tags':
        tags = T.random_tags(rng, V)
        want_any, want_all = T.random_words(rng, B)
        filt.update(tags=tags, want_any=want_any, want_all=want_all)
        targs = _dev_tags(dev, tags, want_any, want_all)
        top = np.argpartition(-rig.logits, 50, axis=1)[:, :50]           # adversarial: each row's own top 50
        filt['ex_lists'] = rig.exclusions(np.arange(B, dtype=np.int32), [np.sort(t) for t in top])
        ex = rig.ex
    seed, kv, sc, ei, ky, close = _seed_for(dev, users, W, s, rig.logits, tau, k, 100 * d + k, **filt)
    sample = _keyed(dev, tau, seed, W, s, users)
    scan = TopKScan(B, V, d, k, dev, chunk=256)
    assert scan.fused
    lat, pool, bias = rig.latent.value, rig.pool.value, rig.pool.bias_value
    e = lambda dt: torch.empty((B, k), dtype=dt, device=dev)
    gv, gi, pv, pi = e(torch.float32), e(torch.int32), e(torch.float32), e(torch.int32)
    zero = np.nonzero(tau == 0)[0]
    assert len(zero) >= 8
    for fused in (True, False):
        scan.fused = fused
        scan.run(lat, pool, bias, rig.rt.ws, gv, gi, ex, tags=targs, sample=sample, strip=False)
        if fused:
            assert not scan.overflowed()
        scan.run(lat, pool, bias, rig.rt.ws, pv, pi, ex, tags=targs)
        v, i = gv.cpu().numpy(), gi.cpu().numpy()
        np.testing.assert_array_equal(i[~close], ei[~close], err_msg='fused=%s' % fused)
        # the KEYS, unstripped: the oracle's keys of the same columns (the same logits and noise bits)
        same = (i == ei) & (i >= 0)
        kk = np.take_along_axis(ky, np.maximum(i, 0), 1)
        with np.errstate(invalid='ignore'):                              # (-inf - -inf beside an index -1)
            assert (np.abs(v.astype(np.float64) - kk)[same] <= S.strip_bound(kk, sc)[same]).all()
        live = same & (tau > 0)[:, None]
        assert live.any() and (v[live] != sc[live]).mean() > 0.9         # keys, not scores
        np.testing.assert_array_equal(i[zero], pi.cpu().numpy()[zero])
        np.testing.assert_array_equal(v[zero], pv.cpu().numpy()[zero])


# ---------------------------------------------------------------- 4. the finish over W slabs
def _slabs(rng, B, V, k, W, P, tau):
    """Scores, eligibility and picks of B rows over V global columns, and what W shards send their owner: packed
    [W, B, 2 P + k] (m parts, S parts, pick scores); shard 1 has fewer parts than P and pads with the empty mass."""
    L = (rng.standard_normal((B, V)) * 2).astype(np.float32)
    elig = rng.random((B, V)) < 0.8
    elig[1] = False
    elig[1, [3, 4, 8, 100]] = True                                       # fewer than k eligible: -1 tails
    picks = np.full((B, k), -1, dtype=np.int64)
    for r in range(B):
        c = np.nonzero(elig[r])[0]
        p = rng.permutation(c)[:k]
        picks[r, :len(p)] = p
    packed = np.zeros((W, B, 2 * P + k), dtype=np.float32)
    packed[:, :, :P], packed[:, :, P:2 * P], packed[:, :, 2 * P:] = -FLT_MAX, 0.0, -np.inf
    for w in range(W):
        cols = np.arange(w, V, W)
        parts = P if w != 1 else max(1, P - 2)
        edges = np.linspace(0, len(cols), parts + 1).astype(np.int64)
        for r in range(B):
            t = float(tau[r]) if tau[r] > 0 else 1.0
            rest = elig[r].copy()
            rest[picks[r][picks[r] >= 0]] = False
            for p in range(parts):
                cc = cols[edges[p]:edges[p + 1]]
                sv = L[r, cc[rest[cc]]].astype(np.float64)
                if len(sv):
                    packed[w, r, p] = sv.max()
                    packed[w, r, P + p] = np.exp((sv - sv.max()) / t).sum()
            for j in range(k):
                if picks[r, j] >= 0 and picks[r, j] % W == w:
                    packed[w, r, 2 * P + j] = L[r, picks[r, j]]
    return L, elig, picks, packed


@pytest.mark.parametrize("P", [1, 5])
def test_finish_over_shard_slabs(dev, P):
    import torch
    from arx import ops
    B, V, k, W = 70, 600, 30, 3
    rng = np.random.default_rng(10 + P)
    tau = TAUS[rng.integers(1, 4, B)]
    tau[[0, 9]] = 0
    L, elig, picks, packed = _slabs(rng, B, V, k, W, P, tau)
    owners = picks[picks >= 0] % W
    assert all((owners == w).any() for w in range(W)) and (picks[1] == -1).any()
    recv = torch.from_numpy(packed).to(dev)
    ids = torch.from_numpy(picks.astype(np.int32)).to(dev)
    sample = _dev_sample(dev, tau, 0)
    lp = torch.empty((B, k), dtype=torch.float32, device=dev)
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    ops.sample_logp_finish_shards(ids, recv[:, :, 2 * P:], recv[:, :, :P], recv[:, :, P:2 * P], P, sample, lp, vals)
    exp = RL.logp(L, elig, picks, tau)
    tol = RL.tolerance(L, elig, tau, exp)
    got = lp.cpu().numpy()
    print("P %d: largest error / tolerance %.3f" % (P, RL.worst(got, exp, tol)))
    assert RL.worst(got, exp, tol) <= 1
    assert (got[tau == 0] == 0).all() and (got[picks < 0] == 0).all() and (got <= 0).all()
    sc = np.where(picks >= 0, np.take_along_axis(L, np.maximum(picks, 0), 1), -np.inf).astype(np.float32)
    np.testing.assert_array_equal(vals.cpu().numpy(), sc)
    # values are optional
    lp2 = torch.empty_like(lp)
    ops.sample_logp_finish_shards(ids, recv[:, :, 2 * P:], recv[:, :, :P], recv[:, :, P:2 * P], P, sample, lp2)
    np.testing.assert_array_equal(lp2.cpu().numpy(), got)


@pytest.mark.parametrize("P", [1, 5])
def test_finish_over_one_slab_is_the_single_device_finish(dev, P):
    import torch
    from arx import ops
    B, V, k = 70, 600, 30
    rng = np.random.default_rng(20 + P)
    tau = TAUS[rng.integers(1, 4, B)]
    tau[[0, 9]] = 0
    L, elig, picks, packed = _slabs(rng, B, V, k, 1, P, tau)
    recv = torch.from_numpy(packed).to(dev)
    ids = torch.from_numpy(picks.astype(np.int32)).to(dev)
    sample = _dev_sample(dev, tau, 0)
    e = lambda: torch.empty((B, k), dtype=torch.float32, device=dev)
    lp_a, v_a, lp_b, v_b = e(), e(), e(), e()
    ops.sample_logp_finish_shards(ids, recv[:, :, 2 * P:], recv[:, :, :P], recv[:, :, P:2 * P], P, sample, lp_a, v_a)
    ops.sample_logp_finish(ids, recv[0, :, 2 * P:], recv[0, :, :P], recv[0, :, P:2 * P], P, sample, lp_b, v_b)
    np.testing.assert_array_equal(lp_a.cpu().numpy(), lp_b.cpu().numpy())
    np.testing.assert_array_equal(v_a.cpu().numpy(), v_b.cpu().numpy())
    assert (lp_a.cpu().numpy() < 0).any()


def test_picks_to_shard(dev):
    import torch
    from arx import ops
    rng = np.random.default_rng(3)
    ids = rng.integers(-1, 2 ** 31 - 1, (37, 30)).astype(np.int32)
    ids[0, :4] = [-1, 0, 2, 5]
    t = torch.from_numpy(ids).to(dev)
    for W, s in ((1, 0), (3, 2), (3, 0), (8, 5)):
        out = torch.empty_like(t)
        ops.picks_to_shard(t, W, s, out)
        exp = np.where((ids >= 0) & (ids % W == s), ids // W, -1)
        np.testing.assert_array_equal(out.cpu().numpy(), exp)
