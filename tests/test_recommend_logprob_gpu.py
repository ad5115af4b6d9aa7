"""recommend(sample_temperature=, return_logprob=True) on the GPU (include/arx_sample_logp.h).

The float64 oracle (tests/recommend_logprob_oracle.py) is evaluated on L -- the project's own scorer GEMM of the same
operands, materialised (the rig of tests/test_recommend_exclude_gpu.py) --, the masks and the DEVICE's own picks, so
near-tied keys exclude no row.  The tolerance is the slate sampler's with C read as the row's eligible count:
2^-20 (1 + (smax - smin) / tau) + 2^-22 |logp| + n_eligible 2^-24; every test prints its largest |error| / tolerance.
"""
import numpy as np
import pytest

import recommend_logprob_oracle as RL
import tags_oracle as T
from test_recommend_exclude_gpu import _Rig, _const, _hmf, _row_cols, _skipgram
from test_recommend_sample_gpu import _dev_sample, _dev_tags, _taus

pytestmark = pytest.mark.gpu


def _check(name, L, elig, tau, gi, gv, glp, extra_tol=None):
    """ids are the device's; logp within tolerance of the oracle on them; values the bits of L; zeros exact."""
    exp = RL.logp(L, elig, gi, tau)
    tol = RL.tolerance(L, elig, tau, exp)
    if extra_tol is not None:
        tol = tol + extra_tol
    live = gi >= 0
    assert (glp[~live] == 0).all() and (glp[tau == 0] == 0).all(), name
    assert np.isfinite(glp).all(), name
    w = RL.worst(glp, exp, tol)
    print("%s: largest |error| / tolerance %.3f" % (name, w))
    assert w <= 1, (name, w)
    sc = np.take_along_axis(L, np.maximum(gi, 0), 1)
    np.testing.assert_array_equal(gv[live].view(np.int32), sc[live].view(np.int32), err_msg=name)
    assert np.isneginf(gv[~live]).all(), name
    for r in range(len(gi)):                                          # distinct, eligible, -1 only at the tail
        ids = gi[r][live[r]]
        assert len(set(ids.tolist())) == len(ids) and elig[r][ids].all() and live[r][:len(ids)].all(), (name, r)
        assert len(ids) == min(gi.shape[1], elig[r].sum()), (name, r)
    return w


def _filters(rig, rng, B, V, mode, dev):
    filt, targs = {}, None
    if 'tags' in mode:
        tags = T.random_tags(rng, V)
        want_any, want_all = T.random_words(rng, B)
        filt.update(tags=tags, want_any=want_any, want_all=want_all)
        targs = _dev_tags(dev, tags, want_any, want_all)
    if 'ex' in mode:
        top = np.argpartition(-rig.logits, 50, axis=1)[:, :50]           # adversarial: each row's own top 50
        filt['ex_lists'] = rig.exclusions(np.arange(B, dtype=np.int32), [np.sort(t) for t in top])
    return filt, targs


def _nodes(rig, k, mode, targs, sargs, chunk=256):
    from arx.hmf import hmf_model as hm
    kw = dict(chunk=chunk, exclude=(lambda: rig.ex) if 'ex' in mode else None,
              tags=(lambda: targs) if targs is not None else None)
    plain = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, sample=lambda: sargs, **kw)
    node = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, sample=lambda: sargs, logp=True, **kw)
    return plain, node


# ---------------------------------------------------------------- 1. the smallest streaming shapes
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("k", [1, 30])
@pytest.mark.parametrize("mode", ["plain", "ex", "tags", "ex_tags"])
def test_stream_logp_smallest_shapes(dev, d, k, mode):
    B, V = 130, 256 + 5 * 64 + 17
    rig = _Rig(B, V, d, seed=5 * d + k)
    rng = np.random.default_rng(d + k)
    tau = _taus(rng, B)
    filt, targs = _filters(rig, rng, B, V, mode, dev)
    elig = RL.eligible(rig.logits, **filt)
    sargs = _dev_sample(dev, tau, 100 * d + k)
    plain, node = _nodes(rig, k, mode, targs, sargs)
    assert node.fused and plain.fused and (tau == 0).sum() >= 8
    for fused in (True, False):
        node.fused = plain.fused = fused
        node.forward(False)
        plain.forward(False)
        if fused:
            assert not node.overflowed()
        gi = node.indices.cpu().numpy()
        np.testing.assert_array_equal(gi, plain.indices.cpu().numpy(), err_msg='fused=%s' % fused)
        _check('d=%d k=%d %s fused=%s' % (d, k, mode, fused), rig.logits, elig, tau, gi, node.value.cpu().numpy(),
               node.logp.cpu().numpy())


# ---------------------------------------------------------------- 2. adversarial lists through the kernels
def _bias_rig(B, V, d, bias):
    """a zero latent: row r's scores are the bias itself, so the order is known"""
    import torch
    rig = _Rig(B, V, d, seed=1)
    dev = rig.rt.device
    rig.lat = torch.zeros((B, d), dtype=torch.float32, device=dev)
    rig.pl = torch.zeros((V, d), dtype=torch.float32, device=dev)
    rig.bias = torch.from_numpy(bias).to(dev)
    return rig


def _kernel_logp(rig, dev, V, picks, tau, ex=None, streaming=True, chunk=192):
    """sort + mass pass + finish on hand-made picks: (logp, values)"""
    import torch
    from arx import ops
    from arx.topk import LogpBuffers
    B, k = picks.shape
    idx = torch.from_numpy(picks.astype(np.int32)).to(dev)
    sargs = _dev_sample(dev, tau, 0)
    lb = LogpBuffers(B, k, dev)
    logp = torch.empty((B, k), dtype=torch.float32, device=dev)
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    ops.sample_logp_sort(idx, lb.pk_cols, lb.pk_slot)
    if streaming:
        P = ops.gemm_nt_topk_parts(B, V)
        mp, sp = lb.parts(P)
        ops.gemm_nt_rest_mass(rig.lat, rig.pl, rig.bias, 0, sargs, lb.picks, mp, sp, lb.pick_score, ex=ex)
        ops.sample_logp_finish(idx, lb.pick_score, mp, sp, P, sargs, logp, vals)
    else:
        buf = torch.empty((B, chunk), dtype=torch.float32, device=dev)
        for c0 in range(0, V, chunk):
            c1 = min(V, c0 + chunk)
            lg = buf[:, :c1 - c0]
            ops.gemm(rig.lat, rig.pl[c0:c1], lg, rig.rt.ws, transB=True, col_bias=rig.bias[c0:c1])
            if ex is not None:
                ops.topk_exclude_fill(lg, c0, ex)
            ops.rest_mass_chunk(lg, c0, sargs, lb.picks, c0 == 0, lb.m_run, lb.s_run, lb.pick_score)
        ops.sample_logp_finish(idx, lb.pick_score, lb.m_run, lb.s_run, 1, sargs, logp, vals)
    return logp.cpu().numpy(), vals.cpu().numpy()


def test_adversarial_lists(dev):
    from arx import ops
    B, d, k = 130, 64, 8
    V = 64 * 2000 + 17                       # more tiles than workgroups per row panel: ranges of several tiles
    P = ops.gemm_nt_topk_parts(B, V)
    tiles = -(-V // 64)
    tpb = -(-tiles // P)
    assert P < tiles and tpb >= 2
    rng = np.random.default_rng(3)
    bias = (rng.standard_normal(V) * 2).astype(np.float32)
    w0, w1 = tpb * 64, 2 * tpb * 64          # the second workgroup's range [w0, w1)
    spots = [0, 1, 63, 64, 65, 127, w0 - 1, w0, w0 + 1, w0 + 2, w1 - 1, w1, V - 17, V - 2, V - 1, 64 * 7 + 3,
             64 * 7 + 4, 64 * 7 + 40]
    picks = np.full((B, k), -1, dtype=np.int64)
    lists = []
    for r in range(B):
        mine = rng.permutation(spots)
        picks[r] = mine[:k]
        lists.append(np.sort(np.concatenate([mine[k:k + 6], rng.integers(0, V, 20)])))
        lists[r] = np.setdiff1d(lists[r], picks[r])
    # row 1: REST is empty (everything but its picks is excluded); row 2: fewer than k eligible
    lists[1] = np.setdiff1d(np.arange(V), picks[1])
    picks[2, 5:] = -1
    lists[2] = np.setdiff1d(np.arange(V), picks[2, :5])
    rig = _bias_rig(B, V, d, bias)
    rig.exclusions(np.arange(B, dtype=np.int32), lists)
    tau = _taus(rng, B)
    tau[[1, 2]] = 0.5
    L = np.broadcast_to(bias, (B, V)).copy()
    elig = RL.eligible(L, ex_lists=lists)
    for streaming in (True, False):
        glp, gv = _kernel_logp(rig, dev, V, picks, tau, ex=rig.ex, streaming=streaming, chunk=tpb * 64 + 64)
        _check('adversarial streaming=%s' % streaming, L, elig, tau, picks, gv, glp)
        assert glp[1, k - 1] == 0 and np.isfinite(glp[1]).all() and (glp[1, :k - 1] < 0).all()
        assert glp[2, 4] == 0 and (glp[2, 5:] == 0).all()
    # -inf biases only (the scores are the bias: every row of a rig of its own): nothing is eligible, every pick is -1
    bias3 = np.full(V, -np.inf, dtype=np.float32)
    rig3 = _bias_rig(B, V, d, bias3)
    none = np.full((B, k), -1, dtype=np.int64)
    for streaming in (True, False):
        glp, gv = _kernel_logp(rig3, dev, V, none, tau, streaming=streaming, chunk=tpb * 64 + 64)
        assert (glp == 0).all() and np.isneginf(gv).all()


# ---------------------------------------------------------------- 3. more than one tile per workgroup
def test_cursor_advances_across_tiles(dev):
    from arx import ops
    B, d, k, mode = 130, 32, 30, 'ex_tags'
    V = 64 * 1500 + 5
    assert ops.gemm_nt_topk_parts(B, V) < -(-V // 64)
    rig = _Rig(B, V, d, seed=77)
    rng = np.random.default_rng(8)
    tau = _taus(rng, B)
    filt, targs = _filters(rig, rng, B, V, mode, dev)
    more = [np.union1d(l, rng.integers(0, V, 400)) for l in filt['ex_lists']]
    filt['ex_lists'] = rig.exclusions(np.arange(B, dtype=np.int32), more)
    elig = RL.eligible(rig.logits, **filt)
    sargs = _dev_sample(dev, tau, 5)
    plain, node = _nodes(rig, k, mode, targs, sargs, chunk=4096)
    node.forward(False)
    plain.forward(False)
    assert node.fused and not node.overflowed()
    gi = node.indices.cpu().numpy()
    np.testing.assert_array_equal(gi, plain.indices.cpu().numpy())
    _check('several tiles per workgroup', rig.logits, elig, tau, gi, node.value.cpu().numpy(), node.logp.cpu().numpy())


# ---------------------------------------------------------------- 4. parity with the slate implementation
def test_parity_with_the_slate_sampler(dev):
    """V = 700 <= 1024: the slate sampler over candidates = arange(V) per row, on the same scores, temperatures and
    seed, draws the same ids (the noise is a function of the item) and gives the same logp within the sum of the two
    tolerances -- against the dense node and the streaming node."""
    import torch
    from arx import ops
    from arx.hmf import hmf_model as hm
    B, V, d, k = 64, 700, 64, 30
    rig = _Rig(B, V, d, seed=9)
    rng = np.random.default_rng(12)
    tau = _taus(rng, B)
    sargs = _dev_sample(dev, tau, 77)
    cand = torch.arange(V, dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
    scores = torch.from_numpy(rig.logits).to(dev)
    ids = torch.empty((B, k), dtype=torch.int32, device=dev)
    pos = torch.empty_like(ids)
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    slp = torch.empty_like(vals)
    ops.slate_sample(cand, scores, sargs, k, ids, vals, pos, slp)
    dense = hm.TopK(rig.rt, _const(rig.rt, scores.clone()), k, sample=lambda: sargs, logp=True)
    stream = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, chunk=256, sample=lambda: sargs, logp=True)
    elig = RL.eligible(rig.logits)
    for node in (dense, stream):
        node.forward(False)
        np.testing.assert_array_equal(node.indices.cpu().numpy(), ids.cpu().numpy())
        np.testing.assert_array_equal(node.value.cpu().numpy().view(np.int32), vals.cpu().numpy().view(np.int32))
        a, b = node.logp.cpu().numpy().astype(np.float64), slp.cpu().numpy().astype(np.float64)
        tol = RL.tolerance(rig.logits, elig, tau, a)                  # (C = V = the eligible count: the same bound)
        print("parity %s: largest |difference| / (2 tolerances) %.3f"
              % (type(node).__name__, (np.abs(a - b)[tol > 0] / (2 * tol[tol > 0])).max()))
        assert (np.abs(a - b) <= 2 * tol).all()


def test_parity_with_score_items_through_the_models(dev):
    """The two public calls held against each other on one model, V = 700, B = 64: score_items over candidates =
    arange(V) per row with the same temperatures and seed draws recommend's ids, and the two logprob agree within the
    sum of the two tolerances (both fed through att_emb.sample_args)."""
    import torch
    from arx.hmf.hmf_model import LatentProductModel
    from arx.utils.synthetic import SyntheticHMF
    B, V, k, d = 64, 700, 30, 32
    syn = SyntheticHMF(seed=31, n_users=300, n_items=800, logit_size=V)
    params = syn.glorot_params(d, seed=32, scale=0.5)
    model = LatentProductModel(syn.n_users, syn.n_items, d, 1, B, 0.5, 1.0, syn.u_attr, syn.i_attr,
                               syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind, loss_function='ce', params=params,
                               top_N_items=k)
    rng = np.random.default_rng(13)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    model.step(None, list(users), None, recommend=True)
    L = model.topk.inputs[0].value.cpu().numpy()
    assert L.shape == (B, V)
    elig = RL.eligible(L)
    cands = np.tile(np.arange(V, dtype=np.int32), (B, 1))
    for n in range(2):
        tau = _taus(np.random.default_rng(50 + n), B, zero_every=5)
        gi, glp = model.step(None, list(users), None, recommend=True, sample_temperature=tau, sample_seed=90 + n,
                             return_logprob=True)
        sid, sval, slp = model.score_items(list(users), cands, k, sample_temperature=tau, sample_seed=90 + n,
                                           return_logprob=True)
        np.testing.assert_array_equal(sid.cpu().numpy(), gi)
        a, b = glp.astype(np.float64), slp.cpu().numpy().astype(np.float64)
        tol = RL.tolerance(L, elig, tau, a)
        print("model parity call %d: largest |difference| / (2 tolerances) %.3f"
              % (n, (np.abs(a - b)[tol > 0] / (2 * tol[tol > 0])).max()))
        assert (np.abs(a - b) <= 2 * tol).all()
        _check('model parity call %d' % n, L, elig, tau, gi,
               model._recommend_node('recommend_sample_logp').value.cpu().numpy(), glp)
    assert model.att_emb.sample_draws == 0


def test_fewer_than_k_finite_scores_without_filters(dev):
    """-inf biases leave five finite columns and k = 8, no exclusion lists and no tags: through the nodes (dense,
    fused, chunked) the -inf picks become -1 with logp 0 and value -inf, the last finite pick is certain."""
    import torch
    from arx.hmf import hmf_model as hm
    B, V, d, k = 130, 256 + 5 * 64 + 17, 64, 8
    rig = _Rig(B, V, d, seed=3)
    keep = np.array([3, 300, 400, 590, 592])
    bias = np.full(V, -np.inf, dtype=np.float32)
    bias[keep] = rig.pool.bias_value.cpu().numpy()[keep]
    L = np.full((B, V), -np.inf, dtype=np.float32)
    L[:, keep] = rig.logits[:, keep]
    pool = _const(rig.rt, rig.pool.value, torch.from_numpy(bias).to(dev))
    elig = RL.eligible(L)
    assert (elig.sum(1) == 5).all()
    tau = _taus(np.random.default_rng(2), B)
    sargs = _dev_sample(dev, tau, 4)
    stream = hm.StreamTopK(rig.rt, rig.latent, pool, k, chunk=256, sample=lambda: sargs, logp=True)
    dense = hm.TopK(rig.rt, _const(rig.rt, torch.from_numpy(L).to(dev)), k, sample=lambda: sargs, logp=True)
    got = []
    for node, fused in ((dense, None), (stream, True), (stream, False)):
        if fused is not None:
            node.fused = fused
        node.forward(False)
        if fused:
            assert not node.overflowed()
        gi, gv, glp = node.indices.cpu().numpy(), node.value.cpu().numpy(), node.logp.cpu().numpy()
        assert (gi[:, :5] >= 0).all() and (gi[:, 5:] == -1).all()
        _check('five finite columns %s fused=%s' % (type(node).__name__, fused), L, elig, tau, gi, gv, glp)
        # (a nearly certain pick at a small tau rounds to 0 in float32: <= 0, and the oracle above holds the values)
        assert (glp[:, 4:] == 0).all() and (glp[:, :4] <= 0).all() and (glp[tau > 0][:, :4] < 0).any()
        got.append(gi)
    np.testing.assert_array_equal(got[0], got[1])
    np.testing.assert_array_equal(got[0], got[2])


# ---------------------------------------------------------------- 5. numerics
def test_numerics(dev):
    B, d, k = 130, 64, 10
    V = 64 * 9 + 17
    rng = np.random.default_rng(4)
    base = (np.round(rng.uniform(-15, 15, V) * 1024) / 1024).astype(np.float32)    # (+ 1000 is then exact in float32)
    L = np.broadcast_to(base, (B, V)).copy()
    elig = np.ones((B, V), dtype=bool)
    picks = np.stack([rng.choice(V, k, replace=False) for _ in range(B)])
    out = {}
    for name, bias, tau in (('plain', base, 1.0), ('shift', base + np.float32(1000), 1.0), ('cold', base, 1e-3),
                            ('hot', base, 1e6)):
        rig = _bias_rig(B, V, d, bias.astype(np.float32))
        t = np.full(B, tau, dtype=np.float32)
        Lb = np.broadcast_to(bias.astype(np.float32), (B, V)).copy()
        for streaming in (True, False):
            glp, gv = _kernel_logp(rig, dev, V, picks, t, streaming=streaming)
            _check('%s streaming=%s' % (name, streaming), Lb, elig, t, picks, gv, glp)
            out[name, streaming] = glp
    for streaming in (True, False):
        d_ = np.abs(out['shift', streaming].astype(np.float64) - out['plain', streaming])
        tol = RL.tolerance(L, elig, np.ones(B), out['plain', streaming].astype(np.float64))
        print("shift against plain: largest |difference| / tolerance %.3f" % (d_ / tol).max())
        assert (d_ <= tol).all()
        hot = out['hot', streaming]
        ref = -np.log(V - np.arange(k, dtype=np.float64))[None, :]
        assert (np.abs(hot - ref) <= RL.tolerance(L, elig, np.full(B, 1e6), ref.repeat(B, 0))).all()
        assert np.isfinite(out['cold', streaming]).all()


# ---------------------------------------------------------------- 6. the models
def test_hmf_return_logprob_dense_and_streamed(dev, monkeypatch):
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
    rec(mat)
    L = mat.topk.inputs[0].value.cpu().numpy()
    item_tags = T.random_tags(rng, syn.n_items)
    sets = {int(u): rng.integers(0, syn.n_items, 60).tolist() for u in users}
    want_any, want_all = T.random_words(rng, B, zero_every=5)
    col_tags = item_tags[np.asarray(syn.logit_ind2item_ind, dtype=np.int64)]
    for m in (mat, st):
        m.prepare_recommend_exclusions(sets)
        m.prepare_item_tags(item_tags)
    rows = _row_cols(syn, sets, users)
    for filt in (dict(), dict(exclude_seen=True, tags_any=want_any, tags_all=want_all)):
        elig = RL.eligible(L, col_tags, want_any, want_all, rows) if filt else RL.eligible(L)
        for n in range(3):                                            # eager, captured, replayed: new tau and seed
            tau = _taus(np.random.default_rng(30 + n), B, zero_every=5)
            kw = dict(sample_temperature=tau, sample_seed=40 + n, **filt)
            for m in (mat, st):
                ids = rec(m, **kw)
                out = rec(m, return_logprob=True, **kw)
                assert isinstance(out, tuple) and len(out) == 2
                gi, glp = out
                assert gi.dtype == np.int32 and glp.dtype == np.float32 and gi.shape == glp.shape == (B, k)
                np.testing.assert_array_equal(gi, ids)
                key = hm.recommend_key(bool(filt), bool(filt), True, True)
                gv = m._recommend_node(key).value.cpu().numpy()
                _check('hmf %s call %d %s' % (type(m.topk).__name__, n, sorted(filt)), L, elig, tau, gi, gv, glp)
                again = rec(m, return_logprob=True, **kw)              # the seed replays
                np.testing.assert_array_equal(again[0], gi)
                np.testing.assert_array_equal(again[1], glp)
    assert st._plans['recommend_sample_logp'].graph is not None
    assert mat.att_emb.sample_draws == 0
    one = rec(mat, sample_temperature=1.0, return_logprob=True)
    two = rec(mat, sample_temperature=1.0, return_logprob=True)
    assert mat.att_emb.sample_draws == 2 and (one[0] != two[0]).any()
    np.testing.assert_array_equal(one[0], rec(mat, sample_temperature=1.0, sample_seed=0))
    for bad in (dict(return_logprob=True), dict(return_logprob=True, sample_temperature=None)):
        with pytest.raises(ValueError):
            rec(mat, **bad)
    with pytest.raises(ValueError):
        mat.step(None, list(users), list(users), return_logprob=True, sample_temperature=1.0)
    assert mat.att_emb.sample_draws == 2


def test_hmf_overflow_rerun_redoes_the_mass_pass(dev, monkeypatch):
    """One user excludes the whole first chunk: its threshold is -inf, the fused candidate lists (segments of 8)
    overflow, and run_complete answers on the chunked path -- selection AND mass pass."""
    syn, mat = _hmf(4)
    monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '0')
    _, st = _hmf(4)
    st.topk.chunk = 1536
    st.topk._buf = st.topk._buf[:, :1536].contiguous()
    B = st.batch_size
    rng = np.random.default_rng(6)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    mat.step(None, list(users), None, recommend=True)
    L = mat.topk.inputs[0].value.cpu().numpy()
    sets = {int(u): rng.integers(0, syn.n_items, 60).tolist() for u in users}
    sets[int(users[0])] = [int(i) for i in syn.logit_ind2item_ind[:1536]]
    st.prepare_recommend_exclusions(sets)
    elig = RL.eligible(L, ex_lists=_row_cols(syn, sets, users))
    tau = np.full(B, 2.0, dtype=np.float32)
    kw = dict(recommend=True, exclude_seen=True, sample_temperature=tau, sample_seed=3)
    st._plan('recommend_ex_sample_logp')
    node = st._recommend_node('recommend_ex_sample_logp')
    node.slack, node.min_capp = 0.0, 8                                # segments shorter than the columns of a range
    gi, glp = st.step(None, list(users), None, return_logprob=True, **kw)
    assert int(node.overflow.item()) != 0 and node.fused             # (overflowed, re-ran chunked, restored)
    _check('overflow re-run', L, elig, tau, gi, node.value.cpu().numpy(), glp)
    np.testing.assert_array_equal(gi, st.step(None, list(users), None, **kw))


def test_linear_seq_return_logprob(dev):
    syn, model = _skipgram()
    B = model.batch_size
    rng = np.random.default_rng(9)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    ctx = syn.sample_batch(B, rng)[1][None, :]
    rec = lambda **kw: model.step(None, list(users), ctx.tolist(), recommend=True, **kw)
    rec()
    L = model.topk.inputs[0].value.cpu().numpy()
    elig = RL.eligible(L)
    for n in range(3):
        tau = _taus(np.random.default_rng(40 + n), B, zero_every=5)
        ids = rec(sample_temperature=tau, sample_seed=70 + n)
        gi, glp = rec(sample_temperature=tau, sample_seed=70 + n, return_logprob=True)
        np.testing.assert_array_equal(gi, ids)
        gv = model._sample_nodes['recommend_sample_logp'].value.cpu().numpy()
        _check('linear_seq call %d' % n, L, elig, tau, gi, gv, glp)
    with pytest.raises(ValueError):
        rec(return_logprob=True)
    with pytest.raises(ValueError):
        model.step(None, list(users), ctx.tolist(), list(users), return_logprob=True, sample_temperature=1.0)


def test_entries_without_propensities_say_so(dev):
    from test_recommend_exclude_gpu import _seq
    syn, seq = _seq(11)
    with pytest.raises(NotImplementedError, match='return_logprob'):
        seq.step_recommend(None, list(range(16)), None, [0] * 16, 0, sample_temperature=1.0, return_logprob=True)
    _, hmf = _hmf(4)
    for m in (seq, hmf):
        with pytest.raises(NotImplementedError, match='return_logprob'):
            m.similar_items([1, 2], 3, return_logprob=True)
    assert tuple(hmf.similar_items([1, 2], 3).shape) == (2, 3)
    assert seq.att_emb.sample_draws == 0


# ---------------------------------------------------------------- 7. the law
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_device_law_against_its_own_propensities(dev, seed):
    """4096 rows of one score vector, V = 12, k = 3: the chi^2 of the observed ordered triples against exp(sum logp)
    as the device reports it (RL.law_chi2: the statistic of tests/test_slate_sample_gpu.py for triples, the cells of
    exact expectation below 5 pooled), under the slate test's bound computed the same way for this cell count -- the
    0.999 quantile of chi^2 at cells - 1 degrees of freedom (58.30 at its 30 cells; 274.46 at the 207 here).  Seeds
    0-2 stay under it on the float64 oracle's own draws (tests/test_recommend_logprob_cpu.py)."""
    import torch
    from arx import graph as G
    from arx.topk import TopK
    from test_recommend_logprob_cpu import LAW_K, LAW_ROWS, LAW_SCORES, LAW_TAU
    rt = G.Runtime()
    x = torch.tensor(LAW_SCORES, dtype=torch.float32, device=dev).repeat(LAW_ROWS, 1).contiguous()
    tau = np.full(LAW_ROWS, LAW_TAU, dtype=np.float32)
    sargs = _dev_sample(dev, tau, seed)
    node = TopK(rt, _const(rt, x), LAW_K, sample=lambda: sargs, logp=True)
    node.forward(False)
    ids = node.indices.cpu().numpy().astype(np.int64)
    lp = node.logp.cpu().numpy().astype(np.float64)
    assert (ids >= 0).all() and np.isfinite(lp).all()
    chi2, cells, bound = RL.law_chi2(ids, lp, LAW_SCORES, LAW_TAU)
    print("seed %d: chi2 %.2f over %d cells, bound %.2f" % (seed, chi2, cells, bound))
    assert cells > 100 and chi2 < bound
    # the rows report the propensity of what they drew
    L = np.tile(LAW_SCORES, (LAW_ROWS, 1))
    elig = np.ones(L.shape, dtype=bool)
    want = RL.logp(L, elig, ids, tau)
    assert RL.worst(lp, want, RL.tolerance(L, elig, tau, want)) <= 1
