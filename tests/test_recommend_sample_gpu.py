"""Sampled recommend (sample_temperature / sample_seed), on the GPU.

The oracle (tests/sample_oracle.py) ranks the DEVICE's own logits plus the DEVICE's own noise in numpy: the noise is
gumbel_add on a zero matrix with tau = 1 (fmaf(1, g, 0) is g itself), the key float32(float64(tau) * float64(g) +
float64(v)), then a stable sort by (-key, column).  Ids are compared exactly; values against the device logits within
the strip bound 2^-23 (|key| + |score|).  The rig and the models are those of tests/test_recommend_exclude_gpu.py.
"""
import numpy as np
import pytest

import sample_oracle as S
import tags_oracle as T
from test_recommend_exclude_gpu import _Rig, _const, _hmf, _row_cols, _seq, _skipgram

pytestmark = pytest.mark.gpu

TAUS = np.array([0, 0.25, 1, 4], dtype=np.float32)


def _dev_sample(dev, tau, seed):
    import torch
    from arx.topk import sample_params
    tau, words = sample_params(tau, seed, len(tau))
    return (torch.from_numpy(tau).to(dev), len(tau), torch.from_numpy(words).to(dev))


def _dev_noise(dev, seed, rows, V):
    """g [rows, V] float32 as the device computes it: gumbel_add of tau = 1 on zeros."""
    import torch
    from arx import ops
    z = torch.zeros((rows, V), dtype=torch.float32, device=dev)
    ops.topk_gumbel_add(z, 0, _dev_sample(dev, np.ones(rows, dtype=np.float32), seed))
    return z.cpu().numpy()


def _dev_tags(dev, tags, want_any, want_all):
    import torch
    up = lambda a: torch.from_numpy(T.i32(a)).to(dev)
    return (up(tags), up(want_any), up(want_all), len(want_any))


def _taus(rng, B, zero_every=17):
    tau = TAUS[rng.integers(0, 4, B)]
    tau[::zero_every] = 0
    return tau


def _check_values(gv, gi, logits_masked, ky, err=''):
    """the stripped values against the device logits, within the strip bound; -inf next to -1"""
    ok = gi >= 0
    assert np.isneginf(gv[~ok]).all(), err
    sc = np.take_along_axis(logits_masked, np.maximum(gi, 0), 1)
    kk = np.take_along_axis(ky, np.maximum(gi, 0), 1)
    with np.errstate(invalid='ignore'):                               # (-inf - -inf next to an index -1)
        bad = ok & ~(np.abs(gv.astype(np.float64) - sc.astype(np.float64)) <= S.strip_bound(kk, sc))
    assert not bad.any(), (err, np.argwhere(bad)[:5])


# ---------------------------------------------------------------- 1. / 2. the kernels
def test_gumbel_add_kernel(dev):
    import torch
    from arx import ops
    B, V, tau_rows, seed = 96, 3000, 40, 1
    rows = np.arange(B) % tau_rows
    x = S.bits(seed, range(tau_rows), range(V))[rows]
    g = _dev_noise(dev, seed, tau_rows, V)[rows]
    assert np.isfinite(g).all()
    # the hash bits, exactly, through u = exp(-exp(-g)) -- wherever a float32 g can carry them: near g = 0
    # neighbouring m lie 3.2e-7 apart in g, one or two float32 roundings (numpy's own float32 g misreads 2 of these
    # 120 000), so the comparison is over the elements whose neighbours lie further off than 4 x the error of a
    # correctly rounded evaluation (S.recoverable: about a quarter, both tails of u); the rest is held by the bound on
    # g below and by the bit-exact keys of the windows
    sure = S.recoverable(x)
    assert sure.mean() > 0.2
    np.testing.assert_array_equal(S.m_of_g(g)[sure], (x >> np.uint32(9))[sure])
    g64 = S.gumbel64(x)
    own = np.abs(S.gumbel32(x).astype(np.float64) - g64).max()       # numpy's float32 formula against float64
    got = np.abs(g.astype(np.float64) - g64).max()
    print("g against float64: device %.3g, numpy float32 %.3g" % (got, own))
    assert got <= 4 * own
    assert g.min() >= -2.8117 and g.max() <= 16.6357
    # windows as strided views; tau = 0 rows and -inf entries stay bit for bit
    rng = np.random.default_rng(0)
    tau = TAUS[rng.integers(0, 4, tau_rows)]
    tau[[0, 7]] = 0
    tau[1] = 1
    x0 = rng.standard_normal((B, V)).astype(np.float32)
    x0[rng.random((B, V)) < 0.01] = -np.inf
    args = _dev_sample(dev, tau, seed)
    for col0, ncols in ((0, V), (1000, 1000), (1777, 1223), (2999, 1), (1500, 0)):
        full = torch.from_numpy(x0).to(dev)
        sub = full[:, col0:col0 + ncols]                               # a strided view: ld = V
        ops.topk_gumbel_add(sub, col0, args)
        got = full.cpu().numpy()
        exp = x0.copy()
        exp[:, col0:col0 + ncols] = S.keys(x0[:, col0:col0 + ncols], g[:, col0:col0 + ncols], tau[rows])
        np.testing.assert_array_equal(got, exp, err_msg=str((col0, ncols)))
        zero = tau[rows] == 0
        np.testing.assert_array_equal(got[zero], x0[zero])
        assert np.isneginf(got[np.isneginf(x0)]).all() and np.isfinite(got[np.isfinite(x0)]).all()


def test_gumbel_strip_kernel(dev):
    import torch
    from arx import ops
    B, V, k, tau_rows, seed = 96, 3000, 50, 40, 3
    rows = np.arange(B) % tau_rows
    g = _dev_noise(dev, seed, tau_rows, V)[rows]
    rng = np.random.default_rng(1)
    tau = TAUS[rng.integers(0, 4, tau_rows)]
    tau[[0, 7]] = 0
    score = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    ky = S.keys(score, g, tau[rows])
    idx = np.stack([rng.choice(V, k, replace=False) for _ in range(B)]).astype(np.int32)
    idx[rng.random((B, k)) < 0.1] = -1
    vals = np.take_along_axis(ky, np.maximum(idx, 0), 1)
    dv = torch.from_numpy(np.ascontiguousarray(vals)).to(dev)
    ops.topk_gumbel_strip(dv, torch.from_numpy(idx).to(dev), _dev_sample(dev, tau, seed))
    got = dv.cpu().numpy()
    _check_values(got, idx, score, ky)
    assert (idx < 0).any() and np.isfinite(got[idx >= 0]).all()
    zero = tau[rows] == 0
    keep = zero[:, None] & (idx >= 0)
    np.testing.assert_array_equal(got[keep], vals[keep])               # exact at tau = 0


# ---------------------------------------------------------------- 3. the dense nodes
@pytest.mark.parametrize("with_tags", [False, True])
@pytest.mark.parametrize("with_ex", [False, True])
def test_dense_topk_sampled(dev, with_ex, with_tags):
    import torch
    from arx.hmf import hmf_model as hm
    from arx.lstm.seqModel import TopKSoftmax
    B, V, k, seed = 64, 300, 100, 11
    rig = _Rig(B, V, 32, seed=1)
    rng = np.random.default_rng(2)
    tau = _taus(rng, B)
    tags = want_any = want_all = row_lists = None
    if with_tags:
        tags = T.random_tags(rng, V)
        want_any, want_all = T.random_words(rng, B)
        want_any[5], want_all[5] = 0, 0xffffffff                         # nothing eligible
    if with_ex:
        lists = [np.unique(rng.integers(0, V, 40)) for _ in range(B)]
        lists[6] = np.arange(V)                                          # everything excluded
        row_lists = rig.exclusions(np.arange(B, dtype=np.int32), lists)
    g = _dev_noise(dev, seed, B, V)
    kv, sc, ei, ky = S.sample_topk(rig.logits, g, tau, k, tags, want_any, want_all, row_lists)
    xm = T.masked(rig.logits, tags, want_any, want_all, row_lists)
    sargs = _dev_sample(dev, tau, seed)
    targs = _dev_tags(dev, tags, want_any, want_all) if with_tags else None
    kw = dict(exclude=(lambda: rig.ex) if with_ex else None, tags=(lambda: targs) if with_tags else None)
    for cls in (hm.TopK, TopKSoftmax):
        node = cls(rig.rt, _const(rig.rt, torch.from_numpy(rig.logits).to(dev)), k,
                   sample=sargs if with_tags else (lambda: sargs), **kw)          # the tuple itself, or a callable
        node.forward(False)
        gv, gi = node.value.cpu().numpy(), node.indices.cpu().numpy()
        np.testing.assert_array_equal(gi, ei, err_msg=cls.__name__)
        _check_values(gv, gi, xm, ky, cls.__name__)
        if with_tags:
            assert (gi[5] == -1).all()
        if with_ex:
            assert (gi[6] == -1).all()
        zero = tau == 0
        _, pi = T.topk(xm, k)
        np.testing.assert_array_equal(gi[zero], pi[zero])                # tau = 0: the plain answer
    plain = TopKSoftmax(rig.rt, _const(rig.rt, torch.from_numpy(rig.logits).to(dev)), k)
    plain.forward(False)
    np.testing.assert_array_equal(node.lse.cpu().numpy(), plain.lse.cpu().numpy())


# ---------------------------------------------------------------- 4. the streaming node
def _seed_for(dev, logits, tau, k, base, **filt):
    """The first seed >= base whose oracle keeps the rows with a k-th / (k + 1)-th key closer than the strip bound at
    <= 1 % (decided on the oracle alone, in numpy)."""
    B, V = logits.shape
    for seed in range(base, base + 8):
        g = _dev_noise(dev, seed, B, V)
        kv, sc, ei, ky = S.sample_topk(logits, g, tau, k, **filt)
        close = S.close_rows(ky, kv, sc, k)
        if close.mean() <= 0.01:
            return seed, ei, ky, close
    raise AssertionError("no seed in [%d, %d) with <= 1 %% close rows" % (base, base + 8))


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("k", [1, 30])
@pytest.mark.parametrize("mode", ["plain", "ex", "tags", "ex_tags"])
def test_stream_topk_sampled_smallest_shapes(dev, d, k, mode):
    """The fused filter's smallest shapes: a first chunk of 256, five full tiles and a ragged one of 17 columns, two
    row panels (the second ragged), with bias.  Fused (no overflow) and chunked give the oracle's ids; values within
    the strip bound; tau = 0 rows equal the plain node bit for bit; the log-sum-exp equals the plain node's."""
    from arx.hmf import hmf_model as hm
    B, V = 130, 256 + 5 * 64 + 17
    want_lse = (d // 32 + k) % 2 == 0                                    # on for (32, 1), (64, 30), (128, 30)
    rig = _Rig(B, V, d, seed=5 * d + k)
    rng = np.random.default_rng(d + k)
    tau = _taus(rng, B)
    filt = {}
    targs = None
    if 'tags' in mode:
        tags = T.random_tags(rng, V)
        want_any, want_all = T.random_words(rng, B)
        filt.update(tags=tags, want_any=want_any, want_all=want_all)
        targs = _dev_tags(dev, tags, want_any, want_all)
    if 'ex' in mode:
        top = np.argpartition(-rig.logits, 50, axis=1)[:, :50]           # adversarial: each row's own top 50
        filt['ex_lists'] = rig.exclusions(np.arange(B, dtype=np.int32), [np.sort(t) for t in top])
    seed, ei, ky, close = _seed_for(dev, rig.logits, tau, k, 100 * d + k, **filt)
    xm = T.masked(rig.logits, filt.get('tags'), filt.get('want_any'), filt.get('want_all'), filt.get('ex_lists'))
    sargs = _dev_sample(dev, tau, seed)
    kw = dict(chunk=256, want_lse=want_lse, exclude=(lambda: rig.ex) if 'ex' in mode else None,
              tags=(lambda: targs) if targs is not None else None)
    plain = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, **kw)
    node = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, sample=lambda: sargs, **kw)
    assert node.fused and plain.fused
    zero = np.nonzero(tau == 0)[0]
    assert len(zero) >= 8
    for fused in (True, False):
        node.fused = plain.fused = fused
        node.forward(False)
        plain.forward(False)
        if fused:
            assert not node.overflowed()
        gv, gi = node.value.cpu().numpy(), node.indices.cpu().numpy()
        np.testing.assert_array_equal(gi[~close], ei[~close], err_msg='fused=%s' % fused)
        _check_values(gv, gi, xm, ky, 'fused=%s' % fused)
        np.testing.assert_array_equal(gi[zero], plain.indices.cpu().numpy()[zero])
        np.testing.assert_array_equal(gv[zero], plain.value.cpu().numpy()[zero])
        if want_lse:
            np.testing.assert_array_equal(node.lse.cpu().numpy(), plain.lse.cpu().numpy())


# ---------------------------------------------------------------- 5. one captured plan
def test_one_captured_plan_new_temperature_and_seed(dev):
    from arx import graph as G
    from arx.hmf import hmf_model as hm
    from arx.topk import sample_params
    B, V, k = 130, 256 + 5 * 64 + 17, 30
    rig = _Rig(B, V, 64, seed=21)
    tau_in, seed_in = G.FloatInput(rig.rt, (B,), 'tau'), G.IdsInput(rig.rt, 2, 'seed')
    node = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, chunk=256, sample=lambda: (tau_in.value, B, seed_in.value))
    plan = G.Plan(rig.rt, [node], False, [])
    got = {}
    for n, (t, base) in enumerate([(1.0, 50), (0.25, 60), (4.0, 70), (0.25, 60), (1.0, 50)]):
        tau = np.full(B, t, dtype=np.float32)
        seed, ei, ky, close = _seed_for(dev, rig.logits, tau, k, base)
        tf, words = sample_params(tau, seed, B)
        tau_in.feed(tf)
        seed_in.feed(words)
        plan.run()                                                       # eager, captured, then replays
        assert not node.overflowed()
        gi = node.indices.cpu().numpy()
        np.testing.assert_array_equal(gi[~close], ei[~close], err_msg='call %d' % n)
        if (t, seed) in got:
            np.testing.assert_array_equal(gi, got[(t, seed)])            # the same seed: the same ids
        got[(t, seed)] = gi
    assert plan.graph is not None and len(got) == 3


# ---------------------------------------------------------------- 6. the models
def _model_oracle(dev, logits, tau, seed, k, **filt):
    g = _dev_noise(dev, seed, logits.shape[0], logits.shape[1])
    kv, sc, ei, ky = S.sample_topk(logits, g, tau, k, **filt)
    return ei, S.close_rows(ky, kv, sc, k)


def test_hmf_sampled_dense_and_streamed(dev, monkeypatch):
    from arx.hmf import hmf_model as hm
    syn, mat = _hmf(4)
    monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '0')
    _, st = _hmf(4)
    assert isinstance(st.topk, hm.StreamTopK) and isinstance(mat.topk, hm.TopK)
    st.topk.chunk = 1536
    st.topk._buf = st.topk._buf[:, :1536].contiguous()
    B, k = mat.batch_size, mat.topk.k
    rng = np.random.default_rng(6)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    rec = lambda m, **kw: m.step(None, list(users), None, recommend=True, **kw)
    base = rec(mat)
    logits = mat.topk.inputs[0].value.cpu().numpy()                      # (read before a sampled call turns them to keys)
    np.testing.assert_array_equal(rec(st), base)
    for n in range(3):                                                   # eager, captured, replayed
        tau = _taus(np.random.default_rng(30 + n), B, zero_every=5)
        ei, close = _model_oracle(dev, logits, tau, 40 + n, k)
        assert close.mean() <= 0.04
        a = rec(mat, sample_temperature=tau, sample_seed=40 + n)
        b = rec(st, sample_temperature=tau, sample_seed=40 + n)
        np.testing.assert_array_equal(a, b, err_msg='call %d' % n)
        np.testing.assert_array_equal(a[~close], ei[~close], err_msg='call %d' % n)
        np.testing.assert_array_equal(a[tau == 0], base[tau == 0])
    twin = st._recommend_node('recommend_sample')
    assert isinstance(twin, hm.StreamTopK) and twin.fused and twin.chunk == 1536
    for m in (mat, st):
        np.testing.assert_array_equal(rec(m, sample_temperature=0, sample_seed=9), base)
        np.testing.assert_array_equal(rec(m), base)
        assert m.att_emb.sample_draws == 0                               # explicit seeds leave the counter alone
    one = rec(mat, sample_temperature=1.0)
    two = rec(mat, sample_temperature=1.0)
    assert mat.att_emb.sample_draws == 2 and (one != two).any()
    np.testing.assert_array_equal(one, rec(mat, sample_temperature=1.0, sample_seed=0))
    np.testing.assert_array_equal(two, rec(st, sample_temperature=1.0, sample_seed=1))
    assert mat.att_emb.sample_draws == 2
    for bad in (dict(sample_temperature=-1.0), dict(sample_temperature=[1.0] * (B - 1)),
                dict(sample_temperature=1.0, sample_seed=-1), dict(sample_temperature=float('nan'))):
        with pytest.raises(ValueError):
            rec(mat, **bad)


def test_hmf_sampled_never_returns_an_ineligible_item(dev):
    syn, model = _hmf(3)
    B = model.batch_size
    rng = np.random.default_rng(5)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    item_tags = T.random_tags(rng, syn.n_items)
    sets = {int(u): rng.integers(0, syn.n_items, 60).tolist() for u in users}
    model.prepare_recommend_exclusions(sets)
    model.prepare_item_tags(item_tags)
    want_any, want_all = T.random_words(rng, B, zero_every=5)
    col_tags = item_tags[np.asarray(syn.logit_ind2item_ind, dtype=np.int64)]
    ok = T.eligible(col_tags, want_any, want_all)
    for r, cols in enumerate(_row_cols(syn, sets, users)):
        ok[r, cols] = False
    seen = set()
    for seed in range(20):
        got = model.step(None, list(users), None, recommend=True, exclude_seen=True, tags_any=want_any,
                         tags_all=want_all, sample_temperature=2.0, sample_seed=seed)
        for r in range(B):
            ids = got[r][got[r] >= 0]
            assert ok[r, ids].all() and len(set(ids.tolist())) == len(ids)
            assert len(ids) == min(model.topk.k, ok[r].sum())
        seen.add(got.tobytes())
    assert len(seen) == 20
    assert 'recommend_ex_tags_sample' in model._plans and 'recommend_ex_tags' not in model._plans


def test_linear_seq_sampled(dev):
    syn, model = _skipgram()
    B = model.batch_size
    rng = np.random.default_rng(9)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    ctx = syn.sample_batch(B, rng)[1][None, :]
    rec = lambda **kw: model.step(None, list(users), ctx.tolist(), recommend=True, **kw)
    plain = rec()
    logits = model.topk.inputs[0].value.cpu().numpy()
    for n in range(3):
        tau = _taus(np.random.default_rng(40 + n), B, zero_every=5)
        ei, close = _model_oracle(dev, logits, tau, 70 + n, 8)
        got = rec(sample_temperature=tau, sample_seed=70 + n)
        np.testing.assert_array_equal(got[~close], ei[~close], err_msg='run %d' % n)
        np.testing.assert_array_equal(got[tau == 0], plain[tau == 0])
    np.testing.assert_array_equal(rec(sample_temperature=0.0), plain)
    one, two = rec(sample_temperature=1.0), rec(sample_temperature=1.0)
    assert model.att_emb.sample_draws == 3 and (one != two).any()
    np.testing.assert_array_equal(rec(), plain)
    sets = {int(u): rng.integers(0, syn.n_items, 50).tolist() for u in users}
    model.prepare_recommend_exclusions(sets)
    rows = _row_cols(syn, sets, users)
    for seed in range(20):
        got = rec(exclude_seen=True, sample_temperature=2.0, sample_seed=seed)
        assert all(not set(got[r].tolist()) & set(rows[r]) for r in range(B))


@pytest.mark.parametrize("stream", [False, True])
def test_seq_step_recommend_sampled(dev, monkeypatch, stream):
    """SeqModel.step_recommend(sample_temperature=): ids follow the oracle; a value is exp(logit - lse) with the plain
    call's normaliser -- the item's softmax probability at temperature 1."""
    syn, mat = _seq(11)
    mat._bucket(0)                                   # (materialised: built before the streaming switch below)
    if stream:
        monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '0')
    _, model = _seq(11)
    B, L, k = 16, 4, 7
    bk = model._bucket(0)
    if stream:
        assert 'recommend_stream' in bk
        bk['recommend_stream'].chunk = 128
        bk['recommend_stream']._buf = bk['recommend_stream']._buf[:, :128].contiguous()
    rng = np.random.default_rng(2)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    tg = np.stack([syn.sample_batch(B, rng)[1] for _ in range(L)], 0)
    inp = np.concatenate([np.full((1, B), syn.n_items, dtype=np.int32), tg[:-1]], 0)
    positions = rng.integers(0, L, size=B).tolist()
    rec = lambda m, **kw: m.step_recommend(None, list(users), inp.tolist(), positions, 0, **kw)
    rec(mat)
    rows = [int(p) * B + i for i, p in enumerate(positions)]
    logits = mat._bucket(0)['full'].value.cpu().numpy()[rows]
    base = rec(model)
    pnode = bk['recommend_stream' if stream else 'recommend']
    lse = pnode.lse.cpu().numpy()
    lse = lse if stream else lse[rows]
    for n in range(3):
        tau = _taus(np.random.default_rng(60 + n), B, zero_every=5)
        ei, close = _model_oracle(dev, logits, tau, 80 + n, k)
        got = rec(model, sample_temperature=tau, sample_seed=80 + n)
        for i, (u, p, idx) in enumerate(got):
            assert int(u) == int(users[i])
            if not close[i]:
                np.testing.assert_array_equal(idx, ei[i], err_msg='call %d row %d' % (n, i))
            v = logits[i, idx].astype(np.float64)
            ref = np.exp(v - lse[i])
            # the strip bound (|key| <= |v| + tau * 16.64) carried through exp, the float32 difference and exp
            b = 2.0 ** -23 * (2 * np.abs(v) + tau[i] * 16.64) + 2.0 ** -23 * (1 + np.abs(v - lse[i]))
            assert (np.abs(p - ref) <= ref * (np.expm1(b) + 1e-7)).all(), (n, i)
            if tau[i] == 0:
                np.testing.assert_array_equal(idx, base[i][2])
                np.testing.assert_array_equal(p, base[i][1])
    again = rec(model)
    for i in range(B):
        np.testing.assert_array_equal(again[i][2], base[i][2])
        np.testing.assert_array_equal(again[i][1], base[i][1])


def test_seq_step_recommend_sampled_under_a_striped_wrapper_is_not_implemented(dev):
    syn, model = _seq(11)
    calls = []

    class _Wrapper(object):
        def step_recommend(self, *a):
            calls.append(a)
            return 'served'
    model.rt.dp = _Wrapper()
    try:
        for kw in (dict(sample_temperature=1.0), dict(sample_temperature=0, sample_seed=3)):
            with pytest.raises(NotImplementedError):
                model.step_recommend(None, list(range(16)), None, [0] * 16, 0, **kw)
        assert not calls
        assert model.step_recommend(None, list(range(16)), None, [0] * 16, 0) == 'served' and len(calls) == 1
    finally:
        model.rt.dp = None


# ---------------------------------------------------------------- 7. the law, on the device
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_device_law(dev, seed):
    """[4096, 8] logits of equal rows, tau = 1: the two statistics of the CPU test on the device's ids."""
    import torch
    from arx import graph as G
    from arx.topk import TopK
    from test_recommend_sample_cpu import SCORES
    rows = 4096
    rt = G.Runtime()
    x = torch.tensor(SCORES, dtype=torch.float32, device=dev).repeat(rows, 1).contiguous()
    sargs = _dev_sample(dev, np.ones(rows, dtype=np.float32), seed)
    node = TopK(rt, _const(rt, x), 3, sample=lambda: sargs)
    node.forward(False)
    ids = node.indices.cpu().numpy().astype(np.int64)
    chi2, z = S.law_stats(ids, SCORES, 1.0)
    print("seed %d: chi2 %.2f, inclusion %.2f sigma" % (seed, chi2, z))
    assert chi2 < 24.32 and z < 4.5
    assert all(len(set(r)) == 3 for r in ids.tolist())
    np.testing.assert_allclose(node.value.cpu().numpy(), np.asarray(SCORES, dtype=np.float32)[ids], atol=1e-5)
