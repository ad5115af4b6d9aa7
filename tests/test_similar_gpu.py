"""similar_items on the GPU: TopKScan with the cosine scale (fused = chunked = oracle), the re-run after an overflow,
and model.similar_items of LatentProductModel (id-only and HET), LinearSeq and SeqModel.

Exact data (tests/similar_oracle.py) compares ids and values with the float64 oracle bit for bit, ties included.
Gaussian data follows the random rule (similar_oracle.check_random) at atol = 2 (d + 4) 2^-24: the running-error
bound of two normalisations and a length-d dot of unit vectors (similar_oracle.cos_atol).  The tables are small
(V ~ 1000) and the first chunk is 128 columns wide, so the fused filter GEMM runs behind it."""
import numpy as np
import pytest

import similar_oracle as S
from test_kernels_direct_gpu import _t

pytestmark = pytest.mark.gpu


def _scan(dev, table, queries, k, include_self, chunk=128, chunked=False, tweak=None):
    """-> (values, ids, scan) of topk.similar_scan over `table` (numpy) for the query rows."""
    import torch
    from arx import ops
    from arx.topk import TopKScan, similar_scan
    V, d = table.shape
    B = len(queries)
    scan = TopKScan(B, V, d, k, dev, chunk=chunk)
    if tweak:
        tweak(scan)
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    ids = torch.empty((B, k), dtype=torch.int32, device=dev)
    args = (scan, _t(dev, table), _t(dev, np.asarray(queries, dtype=np.int32)), vals, ids, ops.Workspace(dev),
            include_self)
    if chunked:
        with scan.chunked():
            similar_scan(*args)
    else:
        similar_scan(*args)
    return vals.cpu().numpy(), ids.cpu().numpy(), scan


@pytest.mark.parametrize("k", [1, 12])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_scan_fused_equals_chunked_equals_oracle_exact(dev, d, k):
    V = 1000
    E = S.exact_table(np.random.default_rng(d + k), V, d)
    q = np.concatenate([np.arange(8), np.arange(8, V, 9), [V - 1]]).astype(np.int32)   # 120 rows: the specials first
    C = S.cos64(E[q], E)
    for include_self in (False, True):
        fv, fi, scan = _scan(dev, E, q, k, include_self)
        assert scan.fused and int(scan.overflow.item()) == 0                            # the fused filter ran, complete
        cv, ci, _ = _scan(dev, E, q, k, include_self, chunked=True)
        assert np.array_equal(fv.view(np.int32), cv.view(np.int32)) and np.array_equal(fi, ci)
        wv, wi = S.topk_cos(C, k, None if include_self else q)
        np.testing.assert_array_equal(fi, wi)
        np.testing.assert_array_equal(fv.astype(np.float64), wv)
        if include_self:
            nz = q != S.ZERO_ROW
            assert (fv[nz, 0] == 1.0).all()
            assert fi[0, 0] == 0 and (k == 1 or fi[0, 1] == 1)                          # a tie at 1: the lower id first
    # the zero row as a query: cosine 0 with everything, ids ascending
    zv, zi, _ = _scan(dev, E, [S.ZERO_ROW], k, False)
    assert not zv.any() and zi[0].tolist() == [c for c in range(k + 1) if c != S.ZERO_ROW][:k]


@pytest.mark.parametrize("d", [32, 128])
def test_scan_gaussian_within_the_error_bound(dev, d):
    V, k = 1030, 12
    rng = np.random.default_rng(d)
    E = rng.standard_normal((V, d)).astype(np.float32)
    q = rng.choice(V, 70, replace=False).astype(np.int32)
    C = S.cos64(E[q], E)
    worst = 0.0
    for chunked in (False, True):
        for include_self in (False, True):
            v, i, scan = _scan(dev, E, q, k, include_self, chunked=chunked)
            assert chunked or int(scan.overflow.item()) == 0
            worst = max(worst, S.check_random(i, v, C, k, None if include_self else q, S.cos_atol(d)))
            if include_self:
                assert np.array_equal(i[:, 0], q)
    print("d=%d: largest |cosine - float64| = %.3g (bound %.3g)" % (d, worst, S.cos_atol(d)))


def test_scan_overflow_reruns_chunked(dev):
    """Columns ordered by rising cosine with query 0: every range behind the first chunk beats the threshold, the
    8-entry segments overflow, and similar_scan still returns the oracle's answer (the chunked re-run)."""
    V, d, k = 3000, 64, 12
    rng = np.random.default_rng(3)
    E = rng.standard_normal((V, d)).astype(np.float32)
    E = E[np.argsort(S.cos64(E[:1], E)[0], kind='stable')]                              # (row 0 itself ends last)
    q = np.array([V - 1, 5, 17, V - 2], dtype=np.int32)

    def short(scan):
        scan.slack, scan.min_capp = 0.0, 8
    v, i, scan = _scan(dev, E, q, k, False, tweak=short)
    assert int(scan.overflow.item()) != 0 and scan.fused                                # overflowed, re-ran, restored
    cv, ci, _ = _scan(dev, E, q, k, False, chunked=True)
    assert np.array_equal(v.view(np.int32), cv.view(np.int32)) and np.array_equal(i, ci)
    S.check_random(i, v, S.cos64(E[q], E), k, q, S.cos_atol(d))


def test_scan_refuses_lse_and_bias_with_col_scale(dev):
    import torch
    from arx import ops
    from arx.topk import TopKScan
    E = torch.zeros((300, 32), device=dev)
    v, i = torch.empty((4, 3), device=dev), torch.empty((4, 3), dtype=torch.int32, device=dev)
    inv = torch.ones(300, device=dev)
    with pytest.raises(ValueError):
        TopKScan(4, 300, 32, 3, dev, want_lse=True).run(E[:4], E, None, ops.Workspace(dev), v, i, col_scale=inv)
    with pytest.raises(ValueError):
        TopKScan(4, 300, 32, 3, dev).run(E[:4], E, inv, ops.Workspace(dev), v, i, col_scale=inv)


# ---------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------
V_MODEL = 1000


def _hmf(seed, d=64, het=False, B=16, loss='ce'):
    from arx.hmf.hmf_model import LatentProductModel
    from arx.utils.synthetic import SyntheticHMF
    kw = dict(item_mulhot=True, mulhot_vocab=300, avg_len=4, max_len=9) if het else {}
    syn = SyntheticHMF(seed=seed, n_users=120, n_items=1100, logit_size=V_MODEL, **kw)
    params = syn.glorot_params(d, seed=seed + 1, scale=0.5)
    model = LatentProductModel(syn.n_users, syn.n_items, d, 1, B, 0.5, 1.0, syn.u_attr, syn.i_attr,
                               syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind, loss_function=loss, params=params,
                               top_N_items=10)
    return syn, model


def _skipgram(d=32, output_feat=1):
    from arx.utils.synthetic import SyntheticHMF
    from arx.word2vec import skipgram_model
    syn = SyntheticHMF(seed=21, n_users=100, n_items=1100, logit_size=V_MODEL)
    syn.u_attr.set_model_size(d)
    syn.i_attr.set_model_size(d)
    params = syn.glorot_params(d, seed=22, item_output=True, scale=0.5)
    model = skipgram_model.Model(syn.n_users, syn.n_items, d, 16, 0.5, 1.0, syn.u_attr, syn.i_attr,
                                 syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind, n_input_items=1,
                                 loss_function='ce', use_sep_item=True, top_N_items=8, params=params,
                                 output_feat=output_feat)
    return syn, model


def _poke_exact(model, rng, output_feat=1):
    """Write an exact table into the rows the full pool looks up (id-only output feature: one injective map);
    returns it in logit order."""
    node = model.att_emb._pool_embed('full', output_feat)
    assert len(node.feats) == 1 and node.feats[0].kind == 'cat'
    f = node.feats[0]
    rows = f.maps[0].long()
    assert len(set(rows.cpu().tolist())) == V_MODEL
    E = S.exact_table(rng, V_MODEL, int(f.table.E.shape[1]))
    f.table.E[rows] = _t(f.table.E.device, E)
    return E


def _check_exact_model(model, E):
    q = np.array([0, 1, 2, 3, S.ZERO_ROW, 5, 400, 400, V_MODEL - 1], dtype=np.int32)     # specials, an id twice
    C = S.cos64(E[q], E)
    for include_self in (False, True):
        for k in (1, 12):
            ids, vals = model.similar_items(q, k, include_self=include_self, return_values=True, chunk=128)
            assert ids.dtype.is_floating_point is False and tuple(ids.shape) == (len(q), k)
            wv, wi = S.topk_cos(C, k, None if include_self else q)
            np.testing.assert_array_equal(ids.cpu().numpy(), wi)
            np.testing.assert_array_equal(vals.cpu().numpy().astype(np.float64), wv)
    ids, vals = model.similar_items(q, 3, include_self=True, return_values=True, chunk=128)
    ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
    nz = q != S.ZERO_ROW
    assert (vals[nz, 0] == 1.0).all() and ids[0].tolist() == [0, 1, 2] and ids[5, 0] == 5   # the query first, value 1
    assert not vals[4].any() and ids[4].tolist() == [0, 1, 2]                               # a zero query: all 0
    only = model.similar_items(q, 5, chunk=128)                                             # ids alone by default
    np.testing.assert_array_equal(only.cpu().numpy(), S.topk_cos(C, 5, q)[1])
    # k = V without the query: the last entry is empty
    ids, vals = model.similar_items(q[:3], V_MODEL, return_values=True, chunk=128)
    ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
    wv, wi = S.topk_cos(C[:3], V_MODEL, q[:3])
    np.testing.assert_array_equal(ids, wi)
    assert (ids[:, -1] == -1).all() and np.isneginf(vals[:, -1]).all() and (ids[:, :-1] >= 0).all()
    # the default first chunk (V < 65536: the chunked path alone) gives the same lists
    np.testing.assert_array_equal(model.similar_items(q, 12).cpu().numpy(), S.topk_cos(C, 12, q)[1])


def test_hmf_id_only_exact(dev):
    _, model = _hmf(3)
    E = _poke_exact(model, np.random.default_rng(1))
    _check_exact_model(model, E)
    with pytest.raises(ValueError):
        model.similar_items([V_MODEL], 3)
    with pytest.raises(ValueError):
        model.similar_items([-1], 3)
    with pytest.raises(ValueError):
        model.similar_items([], 3)
    with pytest.raises(ValueError):
        model.similar_items([1], 1025)
    with pytest.raises(ValueError):
        model.similar_items([1], 0)
    with pytest.raises(NotImplementedError):
        model.att_emb.similar_items([1], 3, output_feat=2)


def test_linear_seq_exact_and_output_feat_refusal(dev):
    _, model = _skipgram()
    E = _poke_exact(model, np.random.default_rng(2))
    _check_exact_model(model, E)
    model.output_feat = 2                     # (a model built with token-score pooling has no latent pool)
    with pytest.raises(NotImplementedError):
        model.similar_items([1], 3)


def test_hmf_het_items_within_the_error_bound(dev):
    """HET items: the latent is 1/2 (id row + bag mean).  The cosines are checked against float64 over the pool rows
    the device formed, and those rows against the host formula over the tables."""
    d, k = 64, 12
    syn, model = _hmf(5, d=d, het=True)
    q = np.random.default_rng(0).choice(V_MODEL, 40, replace=False).astype(np.int32)
    ids, vals = model.similar_items(q, k, return_values=True, chunk=128)
    node = model.att_emb._pool_embed('full', 1)
    assert [f.kind for f in node.feats] == ['cat', 'mulhot']
    pool = node.value.cpu().numpy()
    f0, f1 = node.feats
    vals_, starts, lens = (m.cpu().numpy().astype(np.int64) for m in f1.maps)
    Eid, Etok = f0.table.E.cpu().numpy().astype(np.float64), f1.table.E.cpu().numpy().astype(np.float64)
    cmap = f0.maps[0].cpu().numpy().astype(np.int64)
    assert lens.min() >= 1
    host = np.stack([0.5 * (Eid[cmap[j]] + Etok[vals_[starts[j]:starts[j] + lens[j]]].mean(0))
                     for j in range(V_MODEL)])
    np.testing.assert_allclose(pool, host, rtol=1e-5, atol=1e-6)
    worst = S.check_random(ids.cpu().numpy(), vals.cpu().numpy(), S.cos64(pool[q], pool), k, q, S.cos_atol(d))
    inc = model.similar_items(q, k, include_self=True).cpu().numpy()
    assert np.array_equal(inc[:, 0], q)
    print("HET d=%d: largest |cosine - float64| = %.3g (bound %.3g)" % (d, worst, S.cos_atol(d)))


def test_training_is_not_disturbed_by_similar_items(dev):
    """Two equal models train the same three steps; one answers similar_items between them.  Losses and tables stay
    equal bit for bit, and the train plan (captured after its first run) is the same object throughout."""
    syn, a = _hmf(7, d=32)
    _, b = _hmf(7, d=32)
    rng = np.random.default_rng(4)
    batches = [syn.sample_batch(16, rng) for _ in range(3)]
    plan = None
    for n, (users, items) in enumerate(batches):
        la = a.step(None, list(users), list(items))
        lb = b.step(None, list(users), list(items))
        assert la == lb, (n, la, lb)
        if plan is None:
            plan = a._plans['train']
        ids = a.similar_items([3, 7, 500], 10, chunk=128)
        assert tuple(ids.shape) == (3, 10) and a._plans['train'] is plan
    for name, ta in a.att_emb.tables.items():
        assert np.array_equal(ta.E.cpu().numpy(), b.att_emb.tables[name].E.cpu().numpy()), name
    # ... and the answer follows the tables as they are now
    node = a.att_emb._pool_embed('full', 1)
    ids, vals = a.similar_items([3, 7, 500], 10, return_values=True, chunk=128)
    pool = node.value.cpu().numpy()
    f = node.feats[0]
    assert np.array_equal(pool, f.table.E[f.maps[0].long()].cpu().numpy())
    S.check_random(ids.cpu().numpy(), vals.cpu().numpy(), S.cos64(pool[[3, 7, 500]], pool), 10, [3, 7, 500],
                   S.cos_atol(32))


def test_seq_model_similar_items(dev):
    """SeqModel.similar_items: the output item latents step_recommend scores against."""
    from arx.attributes.embed_attribute import EmbeddingAttribute
    from arx.lstm.seqModel import SeqModel
    from arx.utils.synthetic import SyntheticHMF
    size, B, L = 64, 16, 3
    syn = SyntheticHMF(seed=11, n_users=60, n_items=V_MODEL, logit_size=V_MODEL)
    syn.u_attr.set_model_size(size)
    syn.i_attr.set_model_size(size)
    params = syn.glorot_params(size, seed=12, scale=0.4)
    rng = np.random.default_rng(13)
    params['lstm_w'] = (rng.standard_normal((2 * size, 4 * size)) * 0.15).astype(np.float32)
    params['lstm_b'] = (rng.standard_normal((4 * size,)) * 0.05).astype(np.float32)
    i2l = syn.item_ind2logit_ind_dict()
    i2l[syn.n_items] = 0
    emb = EmbeddingAttribute(syn.u_attr, syn.i_attr, B, None, L, False, i2l, syn.logit_ind2item_ind, params=params)
    model = SeqModel([L], size, 1, 5.0, B, 0.5, 0.83, emb, loss='ce', START_ID=syn.n_items, params=params)
    q = rng.choice(V_MODEL, 20, replace=False).astype(np.int32)
    ids, vals = model.similar_items(q, 12, return_values=True, chunk=128)
    pool = model.att_emb._pool_embed('full', model.output_feat).value.cpu().numpy()
    assert pool.shape == (V_MODEL, size) and np.abs(pool).max() > 0
    S.check_random(ids.cpu().numpy(), vals.cpu().numpy(), S.cos64(pool[q], pool), 12, q, S.cos_atol(size))
    model.output_feat = 3
    with pytest.raises(NotImplementedError):
        model.similar_items(q, 12)
