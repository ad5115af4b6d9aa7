"""SeqModel(cell='gru') end to end: tiny vocabularies, size 64, B = 16, buckets [3, 5].

  * the model builds with loss 'mw' and 'ce'; the bucket's hs equals the float64 oracle's forward (tests/gru_oracle.py)
    applied to the values read off the GRU node's own input x and the four parameters, under the kernel bound of
    tests/test_gru_kernels_gpu.py (8 * e_ref + 1e-6 |ref|, e_ref from the oracle run in f32); with num_layers = 2 the
    second cell's hs is checked the same way from the first cell's output
  * thirty SGD steps on a task where the next item is a function of the last one end below the first step's loss
  * a forward_only step is bit-equal on repeat
  * step_recommend's ids are the numpy top-k of hs_rows @ pool^T + bias, computed from arrays read back from the model
    (two ids may swap only where their float64 scores are closer than the f32 product's rounding, 1e-5)
  * saver.save then restore into a fresh cell='gru' model: bit-equal parameters and Adagrad slots under TF's four
    names; a 'gru' checkpoint restored into an 'lstm' model fails loudly; cell='rnn' raises ValueError
  * SeqDataParallel and SeqHybridParallel at world 1 move every parameter as the plain model does
"""
import os

import numpy as np
import pytest

import gru_oracle as GO
from lstm_cases import FACTOR, ratio

pytestmark = pytest.mark.gpu

SIZE, B, BUCKETS = 64, 16, [3, 5]
CFG = dict(n_users=40, n_items=60, logit_size=60)
TF_NAMES = ['rnn/multi_rnn_cell/cell_%d/gru_cell/' + s for s in
            ('gates/weights', 'gates/biases', 'candidate/weights', 'candidate/biases')]
F32, F64 = np.float32, np.float64


def _build(loss, seed=4, num_layers=1, adagrad=True, cell='gru', lr=0.5, clip=5.0, S=32, gru_params=True, cfg=None):
    from arx.attributes.embed_attribute import EmbeddingAttribute
    from arx.lstm.seqModel import SeqModel
    from arx.utils.synthetic import SyntheticHMF
    syn = SyntheticHMF(seed=seed, **(cfg or CFG))
    syn.u_attr.set_model_size(SIZE)
    syn.i_attr.set_model_size(SIZE)
    params = syn.glorot_params(SIZE, seed=seed + 1, scale=0.4)
    rng = np.random.default_rng(seed + 2)
    if gru_params:
        for l in range(num_layers):
            sfx = '' if l == 0 else '_%d' % l
            params['gru_wg' + sfx] = (rng.standard_normal((2 * SIZE, 2 * SIZE)) * 0.15).astype(F32)
            params['gru_bg' + sfx] = (1.0 + rng.standard_normal((2 * SIZE,)) * 0.05).astype(F32)
            params['gru_wc' + sfx] = (rng.standard_normal((2 * SIZE, SIZE)) * 0.15).astype(F32)
            params['gru_bc' + sfx] = (rng.standard_normal((SIZE,)) * 0.05).astype(F32)
    i2l = syn.item_ind2logit_ind_dict()
    START = syn.n_items
    i2l[START] = 0
    n_s = S if loss in ('mw', 'mce') else None
    emb = EmbeddingAttribute(syn.u_attr, syn.i_attr, B, n_s, BUCKETS[-1], False, i2l, syn.logit_ind2item_ind,
                             params=params)
    model = SeqModel(BUCKETS, SIZE, num_layers, clip, B, lr, 0.83, emb, loss=loss, use_concat=False,
                     START_ID=START, params=params, withAdagrad=adagrad, cell=cell)
    pos = syn.positives_dict()
    emb.prepare_warp(pos, pos)
    return syn, emb, model


def _batch(syn, rng, L):
    users = rng.integers(0, syn.n_users, size=B).astype(np.int32)
    tg = np.stack([syn.sample_batch(B, rng)[1] for _ in range(L)], 0)
    inp = np.concatenate([np.full((1, B), syn.n_items, dtype=np.int32), tg[:-1]], 0)
    lens = rng.integers(1, L + 1, size=B)
    w = (np.arange(L)[:, None] < lens[None, :]).astype(np.float32)
    return users, inp, tg, w


def _pool(syn, rng, S=32):
    pool = syn.sample_pool(S, rng)
    return pool, {int(v): i for i, v in enumerate(pool)}


def _step(model, syn, rng, bucket, pool=None, id2idx=None, forward_only=False, batch=None):
    L = BUCKETS[bucket]
    users, inp, tg, w = batch if batch is not None else _batch(syn, rng, L)
    return model.step(None, list(users), inp.tolist(), tg.tolist(), w.tolist(), bucket, pool, id2idx,
                      forward_only=forward_only)


def _check_cell(node, L, what):
    """hs of one GRU node against the float64 oracle on the node's own input and parameters."""
    x = node.inputs[0].value.cpu().numpy().reshape(L, B, -1)
    p = [q.w.cpu().numpy() for q in (node.Wg, node.bg, node.Wc, node.bc)]
    got = node.value.cpu().numpy().reshape(L, B, SIZE)
    r_hs = GO.gru_fwd(x.astype(F64), *[a.astype(F64) for a in p])[0]
    f_hs = GO.gru_fwd(x, *p)[0]
    e_ref = float(np.max(np.abs(f_hs.astype(F64) - r_hs)))
    assert e_ref > 0.0 and np.abs(r_hs).max() > 1e-3, what
    r, err = ratio(got, r_hs, e_ref)
    print("  %s: e_ref %.3e  kernel err %.3e  ratio %.2f" % (what, e_ref, err, r))
    assert r <= FACTOR, (what, r, err, e_ref)


@pytest.mark.parametrize("loss", ['mw', 'ce'])
def test_gru_model_builds_and_hs_matches_oracle(dev, loss):
    from arx.lstm.seqModel import GRU
    syn, emb, model = _build(loss)
    assert model.cell == 'gru' and not model.Ws
    for l in range(1):
        for nm in TF_NAMES:
            assert nm % l in model.rt.dense
    assert not any('lstm_cell' in k for k in model.rt.dense)
    rng = np.random.default_rng(7)
    pool, id2idx = _pool(syn, rng) if loss == 'mw' else (None, None)
    print()
    for bucket in (1, 0):
        l0 = _step(model, syn, rng, bucket, pool, id2idx)              # a training step moves the parameters ...
        assert np.isfinite(l0)
        _step(model, syn, rng, bucket, forward_only=True)              # ... the forward-only one reads them as they are
        cells = model._bucket(bucket)['cells']
        assert len(cells) == 1 and isinstance(cells[0], GRU)
        _check_cell(cells[0], BUCKETS[bucket], "%s bucket %d" % (loss, bucket))
        pool = None


def test_gru_two_layers(dev):
    from arx.lstm.seqModel import GRU
    syn, emb, model = _build('mw', num_layers=2)
    for l in range(2):
        for nm in TF_NAMES:
            assert nm % l in model.rt.dense
    rng = np.random.default_rng(8)
    pool, id2idx = _pool(syn, rng)
    before = [q.w.clone() for layer in model.gru for q in layer]
    _step(model, syn, rng, 1, pool, id2idx)
    moved = [bool((q.w != b0).any()) for b0, q in zip(before, [q for layer in model.gru for q in layer])]
    assert all(moved), moved                                           # all eight parameters train
    _step(model, syn, rng, 1, forward_only=True)
    c0, c1 = model._bucket(1)['cells']
    assert isinstance(c0, GRU) and isinstance(c1, GRU) and c0.Wg is not c1.Wg
    assert np.array_equal(c1.inputs[0].value.cpu().numpy(), c0.value.cpu().numpy())   # keep probability 1
    print()
    _check_cell(c0, 5, "layer 1")
    _check_cell(c1, 5, "layer 2")


def test_gru_sgd_learns_next_item(dev):
    """Targets at t >= 1 are a fixed function of the input item at t (the weight of step 0, whose input is START, is
    zero).  Two batches alternate for thirty SGD steps; the loss of batch 0 afterwards is below its first-step loss."""
    syn, emb, model = _build('ce', adagrad=False, lr=0.5, gru_params=False)
    pop = np.asarray(syn.item_population, dtype=np.int64)
    rng = np.random.default_rng(5)
    L = 5

    def batch():
        idx = np.zeros((L, B), dtype=np.int64)
        idx[0] = rng.integers(0, len(pop), size=B)
        for t in range(1, L):
            idx[t] = (idx[t - 1] * 7 + 3) % len(pop)
        tg = pop[idx].astype(np.int32)
        inp = np.concatenate([np.full((1, B), syn.n_items, dtype=np.int32), tg[:-1]], 0)
        w = np.ones((L, B), dtype=np.float32)
        w[0] = 0.0
        return rng.integers(0, syn.n_users, size=B).astype(np.int32), inp, tg, w
    batches = [batch(), batch()]
    losses = [_step(model, syn, rng, 1, batch=batches[s % 2]) for s in range(30)]
    last = _step(model, syn, rng, 1, batch=batches[0], forward_only=True)
    print("\n  first %.4f  step 30 %.4f  batch 0 afterwards %.4f" % (losses[0], losses[-1], last))
    assert np.all(np.isfinite(losses))
    assert last < losses[0] and losses[-1] < losses[1]


def test_gru_forward_only_repeats_bit_equal(dev):
    syn, emb, model = _build('mw')
    rng = np.random.default_rng(9)
    pool, id2idx = _pool(syn, rng)
    bt = _batch(syn, rng, 5)
    _step(model, syn, rng, 1, pool, id2idx, batch=bt)
    a = _step(model, syn, rng, 1, batch=bt, forward_only=True)
    hs_a = model._bucket(1)['hs'].value.clone()
    b = _step(model, syn, rng, 1, batch=bt, forward_only=True)
    assert np.float64(a).tobytes() == np.float64(b).tobytes()
    assert bool((model._bucket(1)['hs'].value == hs_a).all())


@pytest.mark.parametrize("loss", ['mw', 'ce'])
def test_gru_step_recommend_ids(dev, loss):
    syn, emb, model = _build(loss, seed=11)
    model.topk_n = 7
    rng = np.random.default_rng(2)
    pool, id2idx = _pool(syn, rng) if loss == 'mw' else (None, None)
    _step(model, syn, rng, 0, pool, id2idx)
    L = BUCKETS[0]
    users, inp, tg, w = _batch(syn, rng, L)
    positions = rng.integers(0, L, size=B).tolist()
    got = model.step_recommend(None, list(users), inp.tolist(), positions, 0)
    bk = model._bucket(0)
    assert 'recommend_stream' not in bk
    latent, pe = bk['full'].inputs
    hs = latent.value.cpu().numpy().astype(F64)
    scores = hs @ pe.value.cpu().numpy().astype(F64).T + pe.bias_value.cpu().numpy().astype(F64)
    assert len(got) == B
    for i, (u, vals, idx) in enumerate(got):
        s = scores[int(positions[i]) * B + i]
        want = np.argsort(-s, kind='stable')[:7]
        idx = np.asarray(idx)
        assert int(u) == int(users[i]) and len(set(idx.tolist())) == 7
        for a, b_ in zip(idx, want):
            assert a == b_ or abs(s[a] - s[b_]) < 1e-5, (i, idx, want)
        p = np.exp(s - s.max())
        np.testing.assert_allclose(vals, (p / p.sum())[idx], rtol=1e-4, atol=1e-9)


def test_gru_recommend_options_and_similar_items(dev):
    """Downstream of hs nothing knows the cell: exclusions, tags, sampling and similar_items run."""
    syn, emb, model = _build('mw', seed=12)
    model.topk_n = 5
    rng = np.random.default_rng(3)
    pool, id2idx = _pool(syn, rng)
    _step(model, syn, rng, 0, pool, id2idx)
    users, inp, tg, w = _batch(syn, rng, 3)
    positions = [2] * B
    seen = {int(u): [int(v) for v in np.unique(tg[:, i])] for i, u in enumerate(users)}
    model.prepare_recommend_exclusions(seen)
    model.prepare_item_tags((np.arange(syn.n_items) % 4 + 1).astype(np.uint32))
    l2i = np.asarray(syn.logit_ind2item_ind)
    plain = model.step_recommend(None, list(users), inp.tolist(), positions, 0)
    ex = model.step_recommend(None, list(users), inp.tolist(), positions, 0, exclude_seen=True)
    for i, (u, vals, idx) in enumerate(ex):
        items = [int(l2i[j]) for j in idx if j >= 0]
        assert not set(items) & set(seen[int(u)]), (i, items)
    tagged = model.step_recommend(None, list(users), inp.tolist(), positions, 0, tags_any=1)
    for u, vals, idx in tagged:
        assert all((int(l2i[j]) % 4 + 1) & 1 for j in idx if j >= 0)
    drawn = model.step_recommend(None, list(users), inp.tolist(), positions, 0, sample_temperature=1.0, sample_seed=5)
    again = model.step_recommend(None, list(users), inp.tolist(), positions, 0, sample_temperature=1.0, sample_seed=5)
    for (u0, v0, i0), (u1, v1, i1) in zip(drawn, again):
        assert np.array_equal(i0, i1) and len(set(np.asarray(i0).tolist())) == 5
    assert len(plain) == B
    ids = model.similar_items(np.arange(4, dtype=np.int32), 3)
    assert tuple(ids.shape) == (4, 3)


def test_gru_streamed_dev_loss(dev, monkeypatch):
    """The streamed full-vocabulary dev loss of an 'mw' model (no [L*mb, V] logits) equals the materialised one."""
    cfg = dict(n_users=300, n_items=500, logit_size=500)
    losses = []
    for stream in (False, True):
        if stream:
            monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '1')
            monkeypatch.setenv('ARX_STREAM_EVAL_CHUNK', '200')
        syn, emb, model = _build('mw', seed=13, cfg=cfg)
        assert bool(model._bucket(1).get('eval_streamed')) == stream
        rng = np.random.default_rng(4)
        losses.append(_step(model, syn, rng, 1, batch=_batch(syn, rng, 5), forward_only=True))
    np.testing.assert_allclose(losses[1], losses[0], rtol=1e-4)


def test_gru_checkpoint_round_trip(dev, tmp_path):
    syn, emb, model = _build('mw', num_layers=2)
    rng = np.random.default_rng(6)
    pool, id2idx = _pool(syn, rng)
    for s in range(2):
        _step(model, syn, rng, 1, pool if s == 0 else None, id2idx)
    path = model.saver.save(None, str(tmp_path / "gru"))
    files = np.load(path + '.npz').files
    for l in range(2):
        for nm in TF_NAMES:
            assert nm % l in files and (nm % l) + '/Adagrad' in files
    syn2, emb2, fresh = _build('mw', seed=21, num_layers=2)
    assert any(bool((fresh.rt.dense[k].w != model.rt.dense[k].w).any()) for k in model.rt.dense)
    fresh.saver.restore(None, path)
    assert sorted(fresh.rt.dense) == sorted(model.rt.dense)
    for k, p in model.rt.dense.items():
        q = fresh.rt.dense[k]
        assert np.array_equal(p.w.cpu().numpy().view(np.uint32), q.w.cpu().numpy().view(np.uint32)), k
        assert np.array_equal(p.acc.cpu().numpy().view(np.uint32), q.acc.cpu().numpy().view(np.uint32)), k
        assert bool(p.acc.ne(0).any()) or 'w_input' in k, k            # the slots have moved
    for name, t in emb.tables.items():
        assert np.array_equal(t.E.cpu().numpy(), emb2.tables[name].E.cpu().numpy()), name
    # a 'gru' checkpoint does not fit an 'lstm' model
    _, _, lstm = _build('mw', seed=22, num_layers=2, cell='lstm')
    with pytest.raises(KeyError, match="lstm_cell"):
        lstm.saver.restore(None, path)


def test_gru_cell_keyword(dev):
    with pytest.raises(ValueError, match="cell"):
        _build('mw', cell='rnn')
    _, _, lstm = _build('mw', cell='lstm')
    assert lstm.cell == 'lstm' and lstm.Ws and not lstm.gru
    _, _, dflt = _build('ce', gru_params=False)                        # TF's initial values
    wg, bg, wc, bc = dflt.gru[0]
    assert tuple(wg.w.shape) == (2 * SIZE, 2 * SIZE) and tuple(wc.w.shape) == (2 * SIZE, SIZE)
    assert bool((bg.w == 1.0).all()) and bool((bc.w == 0.0).all())
    lim = np.sqrt(6.0 / (2 * SIZE + 2 * SIZE))
    assert float(wg.w.abs().max()) <= lim and float(wg.w.abs().max()) > 0.5 * lim


@pytest.mark.parametrize("wrapper", ['SeqDataParallel', 'SeqHybridParallel'])
def test_gru_data_parallel_world1(dev, wrapper):
    """One rank: the wrapper's step (eager, its own exchange and apply) moves every parameter as the plain model's
    does -- a dense parameter left out of the reduce list or the apply would stay behind."""
    import torch.distributed as dist
    from arx import dist as adist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(29650 + os.getpid() % 300)
    assert not dist.is_initialized()
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        syn, emb, plain = _build('mw', seed=4)
        _, emb_w, wrapped = _build('mw', seed=4)
        dp = getattr(adist, wrapper)(wrapped)
        assert dp.world == 1
        rng = np.random.default_rng(7)
        pool, id2idx = _pool(syn, rng)
        for s in range(3):
            bt = _batch(syn, rng, 5)
            ps = pool if s == 0 else None
            a = _step(plain, syn, rng, 1, ps, id2idx, batch=bt)
            b_ = _step(wrapped, syn, rng, 1, ps, id2idx, batch=bt)
            np.testing.assert_allclose(dp.global_loss(b_), a, rtol=1e-4)
            np.testing.assert_allclose(float(wrapped._gnorm.item()), float(plain._gnorm.item()), rtol=1e-4)
        start = _build('mw', seed=4)[2]
        for k, p in plain.rt.dense.items():
            got, want, w0 = wrapped.rt.dense[k].w.cpu().numpy(), p.w.cpu().numpy(), start.rt.dense[k].w.cpu().numpy()
            assert np.abs(want - w0).max() > 1e-4, k                   # it trains ...
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=3e-6, err_msg=k)     # ... the same under the wrapper
        tabs = dp.global_params() if hasattr(dp, 'global_params') else emb_w.get_params()
        for k, v in emb.get_params().items():
            np.testing.assert_allclose(tabs[k], v, rtol=1e-4, atol=3e-6, err_msg=k)
    finally:
        dist.destroy_process_group()
