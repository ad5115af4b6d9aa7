"""score_items on the GPU: arx_slate_scores / arx_slate_merge_shards through arx.ops (exact on dyadic data, strided
views, bit-reproducibility, the float32 dot bound, the shard merge), the ordering of arx.slate.slate_order, and the
model methods -- LatentProductModel / LinearSeq (eager, captured, replayed), ShardedHMF and ShardedHetView at world
1 -- against the float64 oracle of tests/slate_oracle.py.

What this file does NOT reach: every entry of SHAPES ends at passes = 1 in arx_slate_scores (the largest,
(2, 5000, 700, 128), is 1250 units on 16 * cu * 4 waves), so there the unit loop takes one trip and a run is one pass
of the slot loop.  The 70000-row case below does stride the unit loop and plans passes = 8, but with one lane per
pair and C = 3: one run per row, which ends in its first pass.  The unit loop past two trips at d = 128 with two runs
per row and eight passes per run, the passes = 4 and 2 branches of the planner and the merge past its grid cap are in
tests/test_grid_stride_gpu.py (shapes from tests/grid_trips.py)."""
import numpy as np
import pytest

import slate_oracle as SO

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 5, 4), (3, 7, 50, 20), (5, 33, 300, 32), (2, 257, 300, 64), (4, 130, 1000, 128), (2, 65, 400, 256),
          (2, 5000, 700, 128)]
_CASES = {}


def _case(shape):
    """(U, P, b, cand, want with bias, want without) of one dyadic shape, computed once and left unchanged."""
    if shape not in _CASES:
        B, C, V, d = shape
        rng = np.random.default_rng(sum(shape))
        U, P, b = SO.dyadic(rng, B, V, d)
        cand = SO.slate(rng, B, C, V)
        _CASES[shape] = (U, P, b, cand, SO.scores(U, P, b, cand).astype(np.float32),
                         SO.scores(U, P, None, cand).astype(np.float32))
    return _CASES[shape]


def _t(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, U, P, b, cand):
    import torch
    from arx import ops
    out = torch.full(cand.shape, float('nan'), dtype=torch.float32, device=dev)
    ops.slate_scores(_t(dev, U), _t(dev, P), None if b is None else _t(dev, b), _t(dev, cand), out)
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_slate_scores_exact_on_dyadic_data(dev, shape):
    U, P, b, cand, want, want_nb = _case(shape)
    assert shape[0] == 1 or (cand[-1] == -1).all()
    assert np.isfinite(want[0, 0]) and (shape[1] < 4 or np.isneginf(want[0, 1:4]).all())
    np.testing.assert_array_equal(_run(dev, U, P, b, cand), want)
    np.testing.assert_array_equal(_run(dev, U, P, None, cand), want_nb)


@pytest.mark.parametrize("shape", SHAPES[1:6], ids=lambda s: "x".join(map(str, s)))
def test_slate_scores_strided_views(dev, shape):
    """U, P, cand and scores as column slices of wider buffers (ld = natural + 4 / + 8 / + 3 / + 5); the padding of
    scores keeps its NaN."""
    import torch
    from arx import ops
    U, P, b, cand, want, _ = _case(shape)
    B, C, V, d = shape
    Uw = torch.full((B, d + 4), 9.0, dtype=torch.float32, device=dev)
    Pw = torch.full((V, d + 8), 9.0, dtype=torch.float32, device=dev)
    cw = torch.full((B, C + 3), 1, dtype=torch.int32, device=dev)
    sw = torch.full((B, C + 5), float('nan'), dtype=torch.float32, device=dev)
    Uw[:, :d], Pw[:, :d], cw[:, :C] = _t(dev, U), _t(dev, P), _t(dev, cand)
    ops.slate_scores(Uw[:, :d], Pw[:, :d], _t(dev, b), cw[:, :C], sw[:, :C])
    got = sw.cpu().numpy()
    np.testing.assert_array_equal(got[:, :C], want)
    assert np.isnan(got[:, C:]).all()


def test_slate_scores_many_rows_second_trip_of_the_unit_loop(dev):
    B, C, V, d = 70000, 3, 64, 4
    rng = np.random.default_rng(8)
    U, P, b = SO.dyadic(rng, B, V, d)
    cand = SO.slate(rng, B, C, V)
    np.testing.assert_array_equal(_run(dev, U, P, b, cand), SO.scores(U, P, b, cand).astype(np.float32))


@pytest.mark.parametrize("d", [20, 128])
def test_slate_scores_bits_do_not_depend_on_slot_order_or_C(dev, d):
    rng = np.random.default_rng(d)
    B, V, C = 3, 2000, 40
    U = rng.standard_normal((B, d)).astype(np.float32)
    P = rng.standard_normal((V, d)).astype(np.float32)
    b = rng.standard_normal(V).astype(np.float32)
    cand = np.stack([rng.choice(V, C, replace=False) for _ in range(B)]).astype(np.int32)
    cand[:, 5] = cand[:, 0]
    cand[:, C - 1] = cand[:, 0]                          # the same item in slots 0, 5 and C - 1
    base = _bits(_run(dev, U, P, b, cand))
    assert (base[:, 0] == base[:, 5]).all() and (base[:, 0] == base[:, C - 1]).all()
    perm = rng.permutation(C)
    np.testing.assert_array_equal(_bits(_run(dev, U, P, b, cand[:, perm])), base[:, perm])
    big = rng.integers(0, V, size=(B, 1000)).astype(np.int32)
    where = np.sort(rng.choice(1000, C, replace=False))
    big[:, where] = cand                                 # the same 40 candidates embedded in C = 1000
    np.testing.assert_array_equal(_bits(_run(dev, U, P, b, big))[:, where], base)
    # and more rows in front change nothing either
    U2 = np.concatenate([rng.standard_normal((5, d)).astype(np.float32), U])
    cand2 = np.concatenate([rng.integers(0, V, size=(5, C)).astype(np.int32), cand])
    np.testing.assert_array_equal(_bits(_run(dev, U2, P, b, cand2))[5:], base)


@pytest.mark.parametrize("d", [20, 64, 128, 256])
def test_slate_scores_within_the_float32_dot_bound(dev, d):
    """|got - ref| <= 2 (d + 1) 2^-24 (sum_i |u_i p_i| + |b|): the textbook bound of a float32 dot in any order."""
    rng = np.random.default_rng(100 + d)
    B, V, C = 6, 3000, 200
    U = rng.standard_normal((B, d)).astype(np.float32)
    P = rng.standard_normal((V, d)).astype(np.float32)
    b = rng.standard_normal(V).astype(np.float32)
    cand = rng.integers(-1, V, size=(B, C)).astype(np.int32)
    cand[:, 3] = -1
    got = _run(dev, U, P, b, cand)
    ref = SO.scores(U, P, b, cand)
    dead = np.isneginf(ref)
    assert dead.any() and np.array_equal(np.isneginf(got), dead)
    err = np.abs(np.where(dead, 0.0, got.astype(np.float64) - np.where(dead, 0.0, ref)))
    lim = SO.bound(d) * SO.abs_scores(U, P, b, cand)
    print("d=%d: largest error / bound = %.3g" % (d, float((err[~dead] / lim[~dead]).max())))
    assert (err <= lim).all()


@pytest.mark.parametrize("W", [1, 3, 64])
def test_slate_merge_shards_keeps_the_owners_bits(dev, W):
    import torch
    from arx import ops
    rng = np.random.default_rng(W)
    B, C = 7, 45
    vals = rng.standard_normal((B, C)).astype(np.float32)
    vals[rng.random((B, C)) < 0.1] = -0.0
    owner = rng.integers(0, W, size=(B, C))
    dead = rng.random((B, C)) < 0.2                      # -inf everywhere
    parts = np.full((W, B, C), -np.inf, dtype=np.float32)
    r, j = np.nonzero(~dead)
    parts[owner[r, j], r, j] = vals[r, j]
    want = np.where(dead, np.float32(-np.inf), vals)
    out = torch.full((B, C + 3), float('nan'), dtype=torch.float32, device=dev)
    ops.slate_merge_shards(_t(dev, parts), out[:, :C])
    got = out.cpu().numpy()
    np.testing.assert_array_equal(_bits(got[:, :C]), _bits(want))
    assert np.isnan(got[:, C:]).all()


@pytest.mark.parametrize("C", [7, 300])
def test_slate_order_equals_the_oracle_on_the_devices_scores(dev, C):
    import torch
    from arx import ops
    from arx.slate import slate_order
    rng = np.random.default_rng(C)
    B, V, d = 5, 500, 20
    U = rng.standard_normal((B, d)).astype(np.float32)
    P = rng.standard_normal((V, d)).astype(np.float32)
    b = rng.standard_normal(V).astype(np.float32)
    cand = rng.integers(0, V, size=(B, C)).astype(np.int32)
    cand[:, 5] = cand[:, 0]
    cand[:, C - 1] = cand[:, 0]                          # real ties: one item in three slots
    cand[:, 2] = -1
    cand[1, 3:] = -1                                     # a row with two live slots
    cand[B - 1] = -1
    dcand = _t(dev, cand)
    sc = torch.empty((B, C), dtype=torch.float32, device=dev)
    ops.slate_scores(_t(dev, U), _t(dev, P), _t(dev, b), dcand, sc)
    host = sc.cpu().numpy()
    assert (_bits(host[0, 0]) == _bits(host[0, 5])).all()
    for k in (1, 5, C):
        vals = torch.empty((B, k), dtype=torch.float32, device=dev)
        pos = torch.empty((B, k), dtype=torch.int32, device=dev)
        ids = torch.empty((B, k), dtype=torch.int32, device=dev)
        slate_order(sc, dcand, k, vals, pos, ids)
        wi, wv = SO.order(host, cand, k)
        np.testing.assert_array_equal(ids.cpu().numpy(), wi, err_msg="k=%d" % k)
        np.testing.assert_array_equal(vals.cpu().numpy(), wv, err_msg="k=%d" % k)
    assert (wi[B - 1] == -1).all() and (wi[1, 2:] == -1).all() and (wi[1, :2] >= 0).all()


# ---------------------------------------------------------------- single-process models
def _slates(rng, rec, V, n_rand, n_dup, n_empty):
    """[B, C]: the row's own recommend output, random logit ids, duplicates of the first slots, -1."""
    B = rec.shape[0]
    cand = np.concatenate([rec, rng.integers(0, V, size=(B, n_rand)), rec[:, :n_dup],
                           np.full((B, n_empty), -1)], axis=1).astype(np.int64)
    return cand


def _check_scores(got, latent, pool, bias, cand, d):
    ref = SO.scores(latent, pool, bias, cand)
    dead = np.isneginf(ref)
    assert np.array_equal(np.isneginf(got), dead)
    err = np.abs(np.where(dead, 0.0, got.astype(np.float64) - np.where(dead, 0.0, ref)))
    assert (err <= SO.bound(d) * SO.abs_scores(latent, pool, bias, cand)).all()


def _model_rounds(model, twin, recommend, score, batches, V, d, top_n, shape):
    import torch
    n_rand, n_dup, n_empty = shape
    rng = np.random.default_rng(77)
    for n, batch in enumerate(batches):                  # eager, captured, replayed
        rec = recommend(model, batch)
        np.testing.assert_array_equal(rec, recommend(twin, batch))
        cand = _slates(rng, rec, V, n_rand, n_dup, n_empty)
        sc = score(batch, cand, None)
        assert isinstance(sc, torch.Tensor) and sc.is_cuda and sc.dtype == torch.float32
        assert tuple(sc.shape) == cand.shape
        out = model.output
        latent, pool, bias = (t.cpu().numpy() for t in (out.inputs[0].value, out.inputs[1].value,
                                                        out.inputs[1].bias_value))
        assert pool.shape == (V, d)
        host = sc.cpu().numpy()
        _check_scores(host, latent, pool, bias, cand, d)
        assert (_bits(host[:, :n_dup]) == _bits(host[:, top_n + n_rand:top_n + n_rand + n_dup])).all()
        ids, vals = score(batch, cand, 10)
        wi, wv = SO.order(host, cand, 10)
        np.testing.assert_array_equal(ids.cpu().numpy(), wi, err_msg="call %d" % n)
        np.testing.assert_array_equal(vals.cpu().numpy(), wv, err_msg="call %d" % n)
        ids, _ = score(batch, rec, top_n)                # recommend's own ids come back in recommend's order
        np.testing.assert_array_equal(ids.cpu().numpy(), rec, err_msg="call %d" % n)
        np.testing.assert_array_equal(recommend(model, batch), recommend(twin, batch))
    keys = [q for q in model._plans if isinstance(q, tuple)]
    C = top_n + n_rand + n_dup + n_empty
    assert keys == [('score_items', C, None), ('score_items', C, 10), ('score_items', top_n, top_n)]
    for bad in (0, C + 1, 1025, 2.5):
        with pytest.raises(ValueError):
            score(batches[0], cand, bad)
    bad = cand.copy()
    bad[3, 1] = V
    with pytest.raises(ValueError):
        score(batches[0], bad, None)
    with pytest.raises(ValueError):
        score(batches[0], cand[:-1], None)


def test_hmf_score_items_eager_captured_replayed(dev):
    from test_recommend_exclude_gpu import _hmf
    syn, model = _hmf(3)
    _, twin = _hmf(3)                                    # the same model, never asked for a slate
    B, V, d, top_n = model.batch_size, model.logit_size, 32, 30
    rng = np.random.default_rng(5)
    batches = [rng.choice(syn.n_users, B, replace=False).astype(np.int32) for _ in range(3)]
    _model_rounds(model, twin, lambda m, u: m.step(None, list(u), None, recommend=True),
                  lambda u, c, k: model.score_items(list(u), c, k=k), batches, V, d, top_n, (12, 4, 4))
    # at most eight slate plans are kept: the oldest goes first
    for C in range(1, 8):
        model.score_items(list(batches[0]), np.zeros((B, C), dtype=np.int64))
    keys = [q for q in model._plans if isinstance(q, tuple)]
    assert len(keys) == 8 and ('score_items', 50, None) not in keys and ('score_items', 7, None) in keys
    np.testing.assert_array_equal(model.step(None, list(batches[0]), None, recommend=True),
                                  twin.step(None, list(batches[0]), None, recommend=True))


def test_linear_seq_score_items_and_output_feat_refusal(dev):
    from test_recommend_exclude_gpu import _skipgram
    syn, model = _skipgram()
    _, twin = _skipgram()
    B, V, d, top_n = model.batch_size, model.logit_size, 32, 8
    rng = np.random.default_rng(9)
    batches = [(rng.choice(syn.n_users, B, replace=False).astype(np.int32), syn.sample_batch(B, rng)[1][None, :])
               for _ in range(3)]
    _model_rounds(model, twin, lambda m, b: m.step(None, list(b[0]), b[1].tolist(), recommend=True),
                  lambda b, c, k: model.score_items(list(b[0]), b[1].tolist(), c, k=k), batches, V, d, top_n,
                  (10, 2, 2))

    # a model built with output_feat 2 over HET items pools token SCORES: there is no item latent
    from arx.utils.synthetic import SyntheticHMF
    from arx.word2vec import skipgram_model
    from arx import graph as G
    het = SyntheticHMF(seed=23, n_users=60, n_items=200, logit_size=150, item_mulhot=True, mulhot_vocab=50, avg_len=3,
                       max_len=6)
    het.u_attr.set_model_size(d)
    het.i_attr.set_model_size(d)
    params = het.glorot_params(d, seed=24, item_output=True, scale=0.5)
    pooled = skipgram_model.Model(het.n_users, het.n_items, d, 16, 0.5, 1.0, het.u_attr, het.i_attr,
                                  het.item_ind2logit_ind_dict(), het.logit_ind2item_ind, n_input_items=1,
                                  loss_function='ce', use_sep_item=True, top_N_items=8, params=params, output_feat=2)
    assert type(pooled.output) is not G.Prediction
    with pytest.raises(NotImplementedError, match="output_feat"):
        pooled.score_items(list(range(16)), [[0] * 16], np.zeros((16, 3), dtype=np.int64))


# ---------------------------------------------------------------- sharded models, world 1
def test_sharded_hmf_world1_exact_and_buffer_cache(dev):
    from arx.dist import ShardedHMF
    n_users, n_items, d, B_loc = 23, 301, 32, 8
    rng = np.random.default_rng(7)
    U, I, b = SO.dyadic(rng, n_users, n_items, d)
    model = ShardedHMF(n_users, n_items, d, B_loc, 8, 0.5, 0, 1, dev, tables={'user': U, 'item': I, 'item_bias': b})
    users = np.array([3, 0, 22, 7, 7])                   # fewer than B_loc; one user twice

    def check(C, k):
        cand = rng.integers(-1, n_items, size=(len(users), C))
        cand[:, 1] = cand[:, 0]
        cand[2] = -1
        want = SO.scores(U[users], I, b, cand).astype(np.float32)
        got = model.score_items(users, cand)
        assert tuple(got.shape) == (len(users), C)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        ids, vals = model.score_items(users, cand, k=k)
        wi, wv = SO.order(want, cand, k)
        np.testing.assert_array_equal(ids.cpu().numpy(), wi)
        np.testing.assert_array_equal(vals.cpu().numpy(), wv)
        assert (wi[2] == -1).all()
    check(9, 5)
    check(20, 20)
    check(9, 5)                                          # the first (C, k) again: its cached buffers
    assert sorted(model._sl_k, key=str) == sorted([(9, None), (9, 5), (20, None), (20, 20)], key=str)
    with pytest.raises(ValueError):
        model.score_items(users, np.zeros((len(users), 4), dtype=np.int64), k=5)
    with pytest.raises(ValueError):
        model.score_items(users, np.full((len(users), 4), n_items))
    assert tuple(model.score_items([], np.zeros((0, 4), dtype=np.int64)).shape) == (0, 4)


def test_het_view_scores_its_own_latents_and_refreshes_after_a_step(dev):
    import torch.distributed as dist
    from arx import dist as adist
    from arx.utils.synthetic import SyntheticHMF
    from test_sharded_het_view_gpu import _init_world1
    _init_world1(dev, 29791)
    try:
        n_users, n_items, V, d, B, S = 100, 200, 60, 32, 16, 32
        syn = SyntheticHMF(n_users=n_users, n_items=n_items, seed=1, permute_logits=False, n_pos=8,
                           item_mulhot=True, mulhot_vocab=V, avg_len=4, max_len=8)
        ia = syn.i_attr
        n_tok = ia._embedding_classes_list_mulhot[0]
        params = syn.glorot_params(d, seed=2, scale=0.5)
        tables = {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
                  'item_bias': params['item_bias_cat_0'][2:], 'token': params['itemembed_mulhot_0'],
                  'token_bias': params['item_bias_mulhot_0']}
        bags = (np.asarray(ia.features_mulhot[0]), np.asarray(ia.mulhot_starts[0]), np.asarray(ia.mulhot_lengths[0]))
        ptr = np.concatenate([syn.pos_ptr[:n_users + 1], [syn.pos_ptr[n_users]]]).astype(np.int32)
        model = adist.ShardedHMFRepTokens(n_users, n_items, d, B, S, 0.5, 0, 1, dev, bags, n_tok, tables=tables)
        with pytest.raises(NotImplementedError, match="item_view"):
            model.score_items([0], [[0]])
        rng = np.random.default_rng(3)
        model.set_positives(ptr, syn.pos_items)
        model.set_pool(syn.sample_pool(S, rng))
        view = model.item_view()
        ask = rng.choice(n_users, size=B - 3, replace=False)
        cand = rng.integers(-1, n_items, size=(len(ask), 25))

        def check():
            got = view.score_items(ask, cand).cpu().numpy()
            ni = model.ni_loc
            _check_scores(got, model.E_user.cpu().numpy()[ask], view.E_item[:ni].cpu().numpy(),
                          view.b_item[:ni].cpu().numpy(), cand, d)
            ids, vals = view.score_items(ask, cand, k=6)
            wi, wv = SO.order(got, cand, 6)
            np.testing.assert_array_equal(ids.cpu().numpy(), wi)
            np.testing.assert_array_equal(vals.cpu().numpy(), wv)
            return got
        first = check()
        assert view.n_refresh == 1
        users, items = syn.sample_batch(B, rng)
        model.step(users, items)
        second = check()
        assert view.n_refresh == 2 and not np.array_equal(first, second)
    finally:
        dist.destroy_process_group()
