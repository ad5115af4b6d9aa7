"""Sampled-pool training ('mw', 'mce') of the skip-gram / CBOW recommenders on the HIP path against
tests/w2v_sampled_ref.py (the oracle's pieces assembled for this family; its gradients are checked against finite
differences in test_w2v_sampled_cpu.py): three training steps, one dev loss, one recommend -- loss, every table and
every Adagrad slot.  Modelled on test_w2v_gpu.py::test_w2v_steps_match_oracle, same tolerances and configurations.

Shapes: d = 64, S = 128 at the smallest batch the fused scorer family takes that still has a row for each of the
mask situations below (asserted: the fused scorer is what ran), and d = 32, S = 64, B = 32 for the unfused route.
The pools and batches make the positive mask matter: a row whose target is in the pool, a row with another
training positive in the pool, context items equal to targets; the pool is redrawn between steps 2 and 3 (the
third step replays the captured graph on the new pool).
"""
import numpy as np
import pytest

from w2v_sampled_ref import RefW2VSampled

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 2e-6

CFG_ID = dict(n_users=300, n_items=500, logit_size=400)
CFG_HET = dict(n_users=300, n_items=500, logit_size=500, item_mulhot=True, user_mulhot=True,
               mulhot_vocab=150, avg_len=5, max_len=12)
MIN_ROWS = 5          # rows 0..2 carry the forced mask situations / context = target; two ordinary rows beside them


def _fused_shape():
    """(d, S, B) of the fused-scorer cases: the smallest B >= MIN_ROWS with ops.mw_scorer_supported(B, 128, 64)."""
    from arx import ops
    B = next((b for b in range(MIN_ROWS, 1025) if ops.mw_scorer_supported(b, 128, 64)), None)
    assert B is not None, "the fused 'mw' scorer takes no batch up to 1024 at S = 128, d = 64"
    return 64, 128, B


def _build(kind, cfg, loss, d, B, S, n_in, seed, sep=True, fuse=None, with_ref=True):
    from arx.utils.synthetic import SyntheticHMF
    from arx.word2vec import cbow_model, skipgram_model
    syn = SyntheticHMF(seed=seed, **cfg)
    syn.u_attr.set_model_size(d)
    syn.i_attr.set_model_size(d)
    params = syn.glorot_params(d, seed=seed + 1, item_output=sep, scale=0.5)
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind
    mod = skipgram_model if kind == 'skipgram' else cbow_model
    model = mod.Model(syn.n_users, syn.n_items, d, B, 0.5, 1.0, syn.u_attr, syn.i_attr, i2l, l2i,
                      n_input_items=n_in, loss_function=loss, use_sep_item=sep, top_N_items=8, n_sampled=S,
                      params=params, fuse_window=fuse)
    pos = syn.positives_dict()
    pos_eval = {u: its[:len(its) // 2] for u, its in pos.items()}       # (the dev loss must use THESE)
    model.prepare_warp(pos, pos_eval)
    ref = None
    if with_ref:
        ref = RefW2VSampled(kind, d, B, 0.5, syn.u_attr, syn.i_attr, i2l, l2i, S, n_input_items=n_in,
                            loss_function=loss, use_sep_item=sep, params=params, top_N_items=8)
        ref.prepare_warp(pos, pos_eval)
    return syn, model, ref


def _force(pool, slot, item):
    """item into the pool (swapped with what sits at `slot`; the pool stays duplicate-free)."""
    hit = np.nonzero(pool == item)[0]
    if len(hit):
        pool[hit[0]], pool[slot] = pool[slot], pool[hit[0]]
    else:
        pool[slot] = item


def _script(syn, B, S, n_in, seed):
    """Three training batches, the pool of steps 1-2 and the pool of step 3, one evaluation batch."""
    rng = np.random.default_rng(seed)
    pos = syn.positives_dict()
    steps = []
    for _ in range(4):
        users, targets = syn.sample_batch(B, rng)
        ctx = np.stack([syn.sample_batch(B, rng)[1] for _ in range(n_in)], 0)      # [n_in, B]
        ctx[0, :3] = targets[:3]                   # context items equal to targets (one table when shared)
        ctx[n_in - 1, 2] = ctx[0, 2]               # ... and an id twice inside one window
        steps.append((users, ctx, targets))
    pools = [syn.sample_pool(S, rng), syn.sample_pool(S, rng)]
    for pool, batches in ((pools[0], steps[:2]), (pools[1], steps[2:3])):
        slot = 0
        for users, _ctx, targets in batches:
            _force(pool, slot, int(targets[0]))                                    # row 0: its target in the pool
            other = next(v for v in pos[int(users[1])] if v != int(targets[1]))
            _force(pool, slot + 1, int(other))                                     # row 1: another positive in the pool
            slot += 2
        assert len(set(pool.tolist())) == S
        for users, _ctx, targets in batches:
            inpool = set(pool.tolist())
            assert int(targets[0]) in inpool
            assert any(v in inpool and v != int(targets[1]) for v in pos[int(users[1])])
    return steps, pools


def _check_tables(model, ref, what):
    got, slots = model.att_emb.get_params(), model.att_emb.get_slots()
    for name, val in got.items():
        np.testing.assert_allclose(val, ref.att_emb.params[name], rtol=RTOL, atol=ATOL, err_msg='%s %s' % (what, name))
        np.testing.assert_allclose(slots[name], ref.att_emb.slots[name], rtol=RTOL, atol=ATOL,
                                   err_msg='%s %s/Adagrad' % (what, name))


def _train3(model, ref, steps, pools):
    for step in range(3):
        users, ctx, targets = steps[step]
        pool = {0: pools[0], 2: pools[1]}.get(step)           # redrawn between steps 2 and 3
        id2idx = {int(v): i for i, v in enumerate(pool)} if pool is not None else None
        l_got = model.step(None, list(users), ctx.tolist(), list(targets), item_sampled=pool,
                           item_sampled_id2idx=id2idx)
        if ref is not None:
            l_ref = ref.step(list(users), ctx.tolist(), list(targets), item_sampled=pool, item_sampled_id2idx=id2idx)
            np.testing.assert_allclose(l_got, l_ref, rtol=RTOL, err_msg='step %d' % step)
            _check_tables(model, ref, 'step %d' % step)


CASES = [(kind, n_in, CFG_ID, loss, sep, shape)
         for kind, n_in in (('skipgram', 3), ('cbow', 4))
         for loss in ('mw', 'mce') for sep in (True, False) for shape in ('fused-scorer', 'unfused')]
CASES += [(kind, n_in, CFG_HET, loss, True, shape)           # HET items and users: today's lookups, silently
          for (kind, n_in), loss, shape in ((('skipgram', 3), 'mw', 'unfused'), (('cbow', 4), 'mce', 'unfused'),
                                            (('cbow', 4), 'mw', 'fused-scorer'), (('skipgram', 3), 'mce', 'fused-scorer'))]


@pytest.mark.parametrize("kind,n_in,cfg,loss,sep,shape", CASES,
                         ids=['%s%d-%s-%s-%s-%s' % (k, n, 'ID' if c is CFG_ID else 'HET', l, 'sep' if s else 'shared', sh)
                              for k, n, c, l, s, sh in CASES])
def test_w2v_sampled_steps_match_helper(dev, kind, n_in, cfg, loss, sep, shape):
    from conftest import assert_scorer_path
    from arx import graph as G, ops
    d, S, B = _fused_shape() if shape == 'fused-scorer' else (32, 64, 32)
    syn, model, ref = _build(kind, cfg, loss, d, B, S, n_in, seed=21, sep=sep)
    # the window is fused exactly where the context items are one one-hot feature
    assert model.fuse_window == (cfg is CFG_ID)
    assert any(isinstance(n, G.WindowEmbed) for n in model.rt.nodes) == (cfg is CFG_ID)
    steps, pools = _script(syn, B, S, n_in, seed=9)
    _train3(model, ref, steps, pools)
    plan = model._plan('train')
    want = assert_scorer_path(plan, B, S, d, loss)
    if shape == 'fused-scorer':
        assert (ops.mw_scorer_supported if loss == 'mw' else ops.mce_scorer_supported)(B, S, d) and want
    else:
        assert not want
    # no [mb, V] node on the training side
    V = model.logit_size
    assert not any(len(n.shape) == 2 and n.shape[1] == V for n in plan.order), "a [mb, V] node in the train plan"
    users, ctx, targets = steps[3]
    e_ref = ref.step(list(users), ctx.tolist(), list(targets), forward_only=True)
    # (the runner evaluates an 'mw' model with loss='warp', run_w2v.py:377)
    e_got = model.step(None, list(users), ctx.tolist(), list(targets), forward_only=True,
                       loss='warp' if loss == 'mw' else None)
    np.testing.assert_allclose(e_got, e_ref, rtol=RTOL)
    r_ref = ref.step(list(users), ctx.tolist(), recommend=True)
    r_got = model.step(None, list(users), ctx.tolist(), recommend=True)
    np.testing.assert_array_equal(r_got, r_ref)
    _check_tables(model, ref, 'after eval / recommend')          # neither touched a table


@pytest.mark.parametrize("sep", [True, False], ids=['sep', 'shared'])
def test_w2v_fused_window_matches_unfused(dev, sep):
    """The same CBOW model with and without the fused window: both match the helper, and each other, after three
    steps.  shared: the window site and the pool's / target's one-hot sites update ONE table in one pass."""
    from arx import graph as G
    d, S, B, n_in = 32, 64, 32, 4
    syn, fused, ref = _build('cbow', CFG_ID, 'mw', d, B, S, n_in, seed=21, sep=sep, fuse=True)
    _, plain, _ = _build('cbow', CFG_ID, 'mw', d, B, S, n_in, seed=21, sep=sep, fuse=False, with_ref=False)
    assert fused.fuse_window and not plain.fuse_window
    assert any(isinstance(n, G.WindowEmbed) for n in fused.rt.nodes)
    assert not any(isinstance(n, G.WindowEmbed) for n in plain.rt.nodes)
    steps, pools = _script(syn, B, S, n_in, seed=9)
    _train3(fused, ref, steps, pools)
    _train3(plain, None, steps, pools)
    _check_tables(plain, ref, 'unfused')
    a, b = fused.att_emb.get_params(), plain.att_emb.get_params()
    sa, sb = fused.att_emb.get_slots(), plain.att_emb.get_slots()
    for name in a:
        np.testing.assert_allclose(a[name], b[name], rtol=RTOL, atol=ATOL, err_msg=name)
        np.testing.assert_allclose(sa[name], sb[name], rtol=RTOL, atol=ATOL, err_msg=name + '/Adagrad')
    # the window's K7 site: one site of kind 'window', mb gradient rows, n * mb keys -- and no ring mode
    plan = fused._plan('train')
    sites = [s for _t, ss, _b, _n in plan.tables for s in ss if s.kind == 'window']
    assert len(sites) == 1 and sites[0].n == B and sites[0].cap == n_in * B
    assert sites[0].node.grad.shape == (B, d)
    assert not plan.ring_capable()


@pytest.mark.parametrize("loss", ['mw', 'mce'])
def test_w2v_sampled_streaming_eval_and_recommend(dev, monkeypatch, loss):
    """ARX_STREAM_TOPK_BYTES = 1: the dev loss and both recommend forms run without [mb, V] logits."""
    from arx import graph as G
    from arx.hmf.hmf_model import StreamTopK
    monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '1')
    d, S, B, n_in = 32, 64, 32, 4
    syn, model, ref = _build('cbow', CFG_ID, loss, d, B, S, n_in, seed=21)
    assert isinstance(model.loss_test.inputs[0], G.StreamEvalLoss)
    assert isinstance(model.topk, StreamTopK)
    steps, pools = _script(syn, B, S, n_in, seed=9)
    _train3(model, ref, steps, pools)
    users, ctx, targets = steps[3]
    e_ref = ref.step(list(users), ctx.tolist(), list(targets), forward_only=True)
    e_got = model.step(None, list(users), ctx.tolist(), list(targets), forward_only=True,
                       loss='warp' if loss == 'mw' else None)
    np.testing.assert_allclose(e_got, e_ref, rtol=RTOL)
    logits = ref.logits_test(list(users), ctx.tolist())
    r_got = model.step(None, list(users), ctx.tolist(), recommend=True)
    np.testing.assert_array_equal(r_got, np.argsort(-logits, axis=1, kind='stable')[:, :8])
    # exclude_seen: the same argsort with each user's exclusion list removed
    pos = syn.positives_dict()
    ex = {int(u): pos[int(u)][:7] for u in set(users.tolist())}
    model.prepare_recommend_exclusions(ex)
    cut = logits.copy()
    for r, u in enumerate(users):
        cols = [syn.item2logit[v] for v in ex[int(u)] if syn.item2logit[v] >= 0]
        cut[r, cols] = -np.inf
    x_got = model.step(None, list(users), ctx.tolist(), recommend=True, exclude_seen=True)
    np.testing.assert_array_equal(x_got, np.argsort(-cut, axis=1, kind='stable')[:, :8])
    assert isinstance(model.topk_ex, StreamTopK)
    assert any((x_got != r_got).any(axis=1))                     # the lists took something out of somebody's top 8


def test_w2v_sampled_refusals(dev):
    from arx.utils.synthetic import SyntheticHMF
    from arx.word2vec import cbow_model
    d, B = 32, 32
    syn = SyntheticHMF(seed=3, **CFG_ID)
    syn.u_attr.set_model_size(d)
    syn.i_attr.set_model_size(d)
    params = syn.glorot_params(d, seed=4, item_output=True, scale=0.5)
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind

    def make(**kw):
        return cbow_model.Model(syn.n_users, syn.n_items, d, B, 0.5, 1.0, syn.u_attr, syn.i_attr, i2l, l2i,
                                n_input_items=2, top_N_items=8, params=params, **kw)
    with pytest.raises(ValueError, match='n_sampled'):
        make(loss_function='mw')                                 # no pool size
    with pytest.raises(ValueError, match='n_sampled'):
        make(loss_function='mce', n_sampled=66)                  # not a multiple of 4
    with pytest.raises(NotImplementedError):
        make(loss_function='rs', n_sampled=64)                   # every other loss: as before
    model = make(loss_function='mw', n_sampled=64)
    pos = syn.positives_dict()
    model.prepare_warp(pos, pos)
    rng = np.random.default_rng(0)
    users, targets = syn.sample_batch(B, rng)
    ctx = np.stack([syn.sample_batch(B, rng)[1] for _ in range(2)], 0)
    with pytest.raises(ValueError, match='item_sampled'):
        model.step(None, list(users), ctx.tolist(), list(targets))          # first step, no pool
    pool = syn.sample_pool(64, rng)
    first = model.step(None, list(users), ctx.tolist(), list(targets), item_sampled=pool)
    again = model.step(None, list(users), ctx.tolist(), list(targets))      # later steps keep the pool
    assert np.isfinite(first) and np.isfinite(again)
