"""Recommend within item tags (tags_any / tags_all), on the GPU.

The oracle (tests/tags_oracle.py) ranks the DEVICE's own logits in numpy: ineligible and excluded columns set to
-inf, a stable sort by (-value, column), the first k, -inf entries -> index -1.  Indices are compared exactly, values
to rtol 1e-6 (the figure of the exclusion tests for this path).  The rig, the models and the adversarial histories
are those of tests/test_recommend_exclude_gpu.py.
"""
import numpy as np
import pytest

import tags_oracle as T
from test_recommend_exclude_gpu import _Rig, _adversarial, _const, _hmf, _row_cols, _seq, _skipgram

pytestmark = pytest.mark.gpu


def _dev_tags(dev, tags, want_any, want_all):
    import torch
    up = lambda a: torch.from_numpy(T.i32(a)).to(dev)
    return (up(tags), up(want_any), up(want_all), len(want_any))


# ---------------------------------------------------------------- kernels
def test_tags_fill_matches_numpy(dev):
    import torch
    from arx import ops
    rng = np.random.default_rng(0)
    B, V, want_rows = 96, 3000, 40                   # want_rows < B: row r uses want_*[r % want_rows]
    tags = T.random_tags(rng, V)
    want_any, want_all = T.random_words(rng, want_rows)
    want_any[1], want_all[1] = 0, 0                  # (0, 0)
    want_any[2], want_all[2] = 1 << 6, 0             # any only
    want_any[3], want_all[3] = 0, (1 << 0) | (1 << 1)                 # all only
    want_any[4], want_all[4] = (1 << 2) | (1 << 3), 1 << 31           # both (bit 31: the int32 sign bit)
    tags[5::7] &= np.uint32(~(1 << 30) & 0xffffffff)
    want_any[5], want_all[5] = 0, 0xffffffff         # a pair no column satisfies
    assert not T.eligible(tags, want_any[5:6], want_all[5:6]).any()
    args = _dev_tags(dev, tags, want_any, want_all)
    x0 = rng.standard_normal((B, V)).astype(np.float32)
    rows = np.arange(B) % want_rows
    el = T.eligible(tags, want_any[rows], want_all[rows])
    assert el[1].all() and 0 < el[2].sum() < V and 0 < el[3].sum() < V and not el[5].any()
    for col0, ncols in ((0, V), (0, 1000), (1000, 1000), (1777, 1223), (2999, 1), (1500, 0)):
        sub = torch.from_numpy(x0).to(dev)[:, col0:col0 + ncols]          # a strided view: ld = V
        ops.topk_tags_fill(sub, col0, args)
        exp = x0[:, col0:col0 + ncols].copy()
        exp[~el[:, col0:col0 + ncols]] = -np.inf
        np.testing.assert_array_equal(sub.cpu().numpy(), exp, err_msg=str((col0, ncols)))


@pytest.mark.parametrize("with_ex", [False, True])
def test_materialised_topk_with_tags(dev, with_ex):
    """TopK with tags: ties across a row, a row with nothing eligible, one with exactly three, one with fifty."""
    import torch
    from arx.hmf import hmf_model as hm
    B, V, k = 64, 300, 100
    rig = _Rig(B, V, 32, seed=1)
    rig.logits[:, 200:220] = rig.logits[:, 10:11]                       # ties across the row
    rng = np.random.default_rng(1)
    tags = T.random_tags(rng, V) & np.uint32(0x0fffffff)                 # bits 28..31 set by hand below
    tags[[17, 250, 3]] |= np.uint32(1 << 28)                             # exactly three columns
    tags[100:150] |= np.uint32(1 << 29)                                  # fifty, ten of them inside the ties
    tags[205:215] |= np.uint32(1 << 29)
    tags[100:110] &= np.uint32(~(1 << 29) & 0xffffffff)
    want_any, want_all = T.random_words(rng, B)
    want_any[5], want_all[5] = 1 << 31, 0                                # nothing carries bit 31
    want_any[6], want_all[6] = 0, 1 << 28
    want_any[7], want_all[7] = 1 << 29, 0
    el = T.eligible(tags, want_any, want_all)
    assert el[5].sum() == 0 and el[6].sum() == 3 and el[7].sum() == 50
    row_lists = None
    if with_ex:
        lists = [np.unique(rng.integers(0, V, 40)) for _ in range(B)]
        lists[6] = np.array([250])                                       # two of the three are left
        row_lists = rig.exclusions(np.arange(B, dtype=np.int32), lists)
    args = _dev_tags(dev, tags, want_any, want_all)
    x = torch.from_numpy(rig.logits).to(dev)
    node = hm.TopK(rig.rt, _const(rig.rt, x), k, exclude=(lambda: rig.ex) if with_ex else None, tags=lambda: args)
    node.forward(False)
    ev, ei = T.topk(rig.logits, k, tags, want_any, want_all, row_lists)
    gv, gi = node.value.cpu().numpy(), node.indices.cpu().numpy()
    np.testing.assert_array_equal(gi, ei)
    np.testing.assert_array_equal(gv, ev)
    assert (gi[5] == -1).all() and np.isneginf(gv[5]).all()
    left = [3, 17] if with_ex else [3, 17, 250]
    assert sorted(gi[6][:len(left)].tolist()) == left and (gi[6][len(left):] == -1).all()
    if not with_ex:
        assert (gi[7][:50] >= 0).all() and (gi[7][50:] == -1).all()


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("k", [1, 30])
@pytest.mark.parametrize("with_ex", [False, True])
def test_stream_topk_tags_smallest_shapes(dev, d, k, with_ex):
    """The fused kernel at its smallest failing shapes: a first chunk of 256, five full tiles and a ragged one of 17
    columns behind it, two row panels (the second ragged), with bias; eligibility from ~50 % down to ~2 %; every
    17th row (0, 0).  Fused and chunked give the oracle; the (0, 0) rows equal the plain node's bit for bit."""
    from arx.hmf import hmf_model as hm
    B, V = 130, 256 + 5 * 64 + 17
    rig = _Rig(B, V, d, seed=3 * d + k)
    rng = np.random.default_rng(d + k)
    tags = T.random_tags(rng, V)
    want_any, want_all = T.random_words(rng, B)
    share = T.eligible(tags, want_any, want_all).mean(1)
    assert share.max() == 1.0 and 0.35 < np.sort(share)[-20] and share.min() < 0.06
    row_lists = None
    if with_ex:
        top = np.argpartition(-rig.logits, 50, axis=1)[:, :50]           # adversarial: each row's own top 50
        row_lists = rig.exclusions(np.arange(B, dtype=np.int32), [np.sort(t) for t in top])
    args = _dev_tags(dev, tags, want_any, want_all)
    ex = (lambda: rig.ex) if with_ex else None
    plain = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, chunk=256, exclude=ex)
    node = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, chunk=256, exclude=ex, tags=lambda: args)
    assert node.fused and plain.fused
    ev, ei = T.topk(rig.logits, k, tags, want_any, want_all, row_lists)
    zero = np.arange(0, B, 17)
    assert not want_any[zero].any() and not want_all[zero].any()
    for fused in (True, False):
        node.fused = plain.fused = fused
        node.forward(False)
        plain.forward(False)
        if fused:
            assert not node.overflowed()
        gv, gi = node.value.cpu().numpy(), node.indices.cpu().numpy()
        np.testing.assert_array_equal(gi, ei, err_msg='fused=%s' % fused)
        np.testing.assert_allclose(gv, ev, rtol=1e-6, err_msg='fused=%s' % fused)
        np.testing.assert_array_equal(gi[zero], plain.indices.cpu().numpy()[zero])
        np.testing.assert_array_equal(gv[zero], plain.value.cpu().numpy()[zero])


@pytest.fixture(scope="module")
def big_rig(dev):
    """V = 200 000, B = 256, d = 128 and its device logits, computed once (read-only)."""
    return _Rig(256, 200000, 128, seed=77)


def test_default_chunk_dense_tags_do_not_overflow(dev, big_rig):
    """The default chunk (65 536) once: k = 100, with exclusions, every row's eligible share >= 25 %.  Every row has
    >= k eligible columns inside the first chunk (checked here on the CPU), so its threshold is finite and the
    candidate segments are sized for it: the fused run must not overflow."""
    from arx.hmf import hmf_model as hm
    rig, k = big_rig, 100
    B, V = rig.logits.shape
    rng = np.random.default_rng(5)
    tags = T.random_tags(rng, V)
    want_any = np.zeros(B, dtype=np.uint32)
    want_all = np.zeros(B, dtype=np.uint32)
    for r in range(B):
        if r % 3 == 0:
            want_any[r] = 1 << (6 * (r % 5))                             # one bit of p = 1/2
        elif r % 3 == 1:
            want_all[r] = 1 << (1 + 6 * (r % 5))                         # one bit of p = 1/4
    row_lists = rig.exclusions(np.arange(B, dtype=np.int32), _adversarial(rig.logits, rng))
    el = T.eligible(tags, want_any, want_all)
    assert el.mean(1).min() >= 0.24
    first = T.masked(rig.logits[:, :65536], tags[:65536], want_any, want_all,
                     [c[c < 65536] for c in row_lists])
    assert (np.isfinite(first).sum(1) >= k).all()
    args = _dev_tags(dev, tags, want_any, want_all)
    node = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, exclude=lambda: rig.ex, tags=lambda: args)
    assert node.fused and node.chunk == 65536
    node.forward(False)
    assert not node.overflowed()
    ev, ei = T.topk(rig.logits, k, tags, want_any, want_all, row_lists)
    np.testing.assert_array_equal(node.indices.cpu().numpy(), ei)
    np.testing.assert_allclose(node.value.cpu().numpy(), ev, rtol=1e-6)


def test_tag_absent_from_the_first_chunk_takes_the_chunked_route(dev, big_rig):
    """A tag carried by every column >= 65 536 and by none below: the first chunk gives no row a threshold, every
    column range then holds far more survivors than its segment -- the fused run reports overflowed(), the chunked
    re-run gives the oracle, and run_complete gets there on its own."""
    from arx.hmf import hmf_model as hm
    from arx.topk import run_complete
    rig, k = big_rig, 30
    B, V = rig.logits.shape
    tags = np.zeros(V, dtype=np.uint32)
    tags[65536:] = 1 << 9
    tags[::2] |= np.uint32(1)
    want_any = np.full(B, 1 << 9, dtype=np.uint32)
    want_all = np.zeros(B, dtype=np.uint32)
    args = _dev_tags(dev, tags, want_any, want_all)
    node = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, tags=lambda: args)
    assert node.fused
    node.forward(False)
    assert node.overflowed()
    ev, ei = T.topk(rig.logits, k, tags, want_any, want_all)
    assert (ei >= 65536).all()
    with node.chunked():
        node.forward(False)
    np.testing.assert_array_equal(node.indices.cpu().numpy(), ei)
    np.testing.assert_allclose(node.value.cpu().numpy(), ev, rtol=1e-6)
    node.indices.fill_(-7)
    run_complete(node, lambda: node.forward(False))
    assert node.fused and int(node.overflow.item()) != 0                 # (overflowed, re-ran chunked, restored)
    np.testing.assert_array_equal(node.indices.cpu().numpy(), ei)


@pytest.mark.parametrize("with_ex", [False, True])
def test_lse_stays_over_all_columns(dev, with_ex):
    """want_lse with tags: the log-sum-exp equals the unfiltered node's bit for bit, fused and chunked."""
    from arx.hmf import hmf_model as hm
    B, V, k = 130, 256 + 5 * 64 + 17, 30
    rig = _Rig(B, V, 64, seed=9)
    rng = np.random.default_rng(9)
    tags = T.random_tags(rng, V)
    want_any, want_all = T.random_words(rng, B)
    row_lists = None
    if with_ex:
        row_lists = rig.exclusions(np.arange(B, dtype=np.int32),
                                   [np.unique(rng.integers(0, V, 60)) for _ in range(B)])
    args = _dev_tags(dev, tags, want_any, want_all)
    ex = (lambda: rig.ex) if with_ex else None
    plain = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, chunk=256, want_lse=True)
    node = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, chunk=256, want_lse=True, exclude=ex, tags=lambda: args)
    _, ei = T.topk(rig.logits, k, tags, want_any, want_all, row_lists)
    for fused in (True, False):
        node.fused = plain.fused = fused
        plain.forward(False)
        node.forward(False)
        np.testing.assert_array_equal(node.lse.cpu().numpy(), plain.lse.cpu().numpy(), err_msg='fused=%s' % fused)
        np.testing.assert_array_equal(node.indices.cpu().numpy(), ei, err_msg='fused=%s' % fused)
    x = rig.logits.astype(np.float64)
    ref = np.log(np.exp(x - x.max(1, keepdims=True)).sum(1)) + x.max(1)
    np.testing.assert_allclose(node.lse.cpu().numpy(), ref, rtol=1e-5)


def test_cosine_form_refuses_tags(dev):
    import torch
    from arx.topk import TopKScan
    from arx import ops
    scan = TopKScan(4, 300, 32, 5, dev)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    zi = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        scan.run(z(4, 32), z(300, 32), None, ops.Workspace(dev), z(4, 5), zi(4, 5), col_scale=z(300),
                 tags=(zi(300), zi(4), zi(4), 4))
    with pytest.raises(ValueError):                                      # tag words for another vocabulary
        scan.run(z(4, 32), z(300, 32), None, ops.Workspace(dev), z(4, 5), zi(4, 5), tags=(zi(299), zi(4), zi(4), 4))


# ---------------------------------------------------------------- models
def _words(rng, B):
    """per-row words for the model tests: (0, 0), dense, sparse and one nothing satisfies"""
    want_any, want_all = T.random_words(rng, B, zero_every=5)
    want_all[3] = (1 << 4) | (1 << 5) | (1 << 10) | (1 << 11) | (1 << 17) | (1 << 23)      # ~ nothing eligible
    return want_any, want_all


def _col_tags(syn, item_tags):
    return item_tags[np.asarray(syn.logit_ind2item_ind, dtype=np.int64)]


@pytest.mark.parametrize("exclude_seen", [False, True])
def test_hmf_tags_end_to_end(dev, exclude_seen):
    """LatentProductModel.step(recommend, tags_any, tags_all): eager, captured, replayed with other words; a call
    without words is what it was before prepare_item_tags and builds no tag plan; a second prepare replaces."""
    from arx.hmf import hmf_model as hm
    syn, model = _hmf(3)
    assert isinstance(model.topk, hm.TopK)
    B, k = model.batch_size, model.topk.k
    rng = np.random.default_rng(5)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    item_tags = T.random_tags(rng, syn.n_items)
    rec = lambda **kw: model.step(None, list(users), None, recommend=True, exclude_seen=exclude_seen, **kw)
    sets = {int(u): rng.integers(0, syn.n_items, 60).tolist() for u in users}
    if exclude_seen:
        model.prepare_recommend_exclusions(sets)
    with pytest.raises(ValueError):
        rec(tags_any=1)                                           # no tags prepared
    base = rec()
    logits = model.topk.inputs[0].value.cpu().numpy()
    model.prepare_item_tags(item_tags)
    np.testing.assert_array_equal(rec(), base)
    assert 'recommend_tags' not in model._plans and 'recommend_ex_tags' not in model._plans
    rows = _row_cols(syn, sets, users) if exclude_seen else None
    key = 'recommend_ex_tags' if exclude_seen else 'recommend_tags'
    col_tags = _col_tags(syn, item_tags)
    plan = None
    for n in range(4):                                            # eager, captured, then replays with other words
        want_any, want_all = _words(np.random.default_rng(20 + max(n, 1)), B)
        got = rec(tags_any=want_any, tags_all=want_all)
        _, exp = T.topk(logits, k, col_tags, want_any, want_all, rows)
        np.testing.assert_array_equal(got, exp, err_msg='call %d' % n)
        assert (got[3] == -1).any() and (got[0] >= 0).all()
        if n >= 2:
            assert model._plans[key] is plan                      # one captured plan, new words
        plan = model._plans[key]
    # one word for every row; python ints
    got = rec(tags_any=int(1 << 6), tags_all=None)
    _, exp = T.topk(logits, k, col_tags, np.full(B, 1 << 6), np.zeros(B), rows)
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(rec(tags_any=0, tags_all=0), base)          # (0, 0): the unfiltered answer
    np.testing.assert_array_equal(rec(), base)
    # the dict form, replacing the words
    d = {i: [b for b in range(32) if (int(item_tags[i]) >> b) & 1 and b != 6] for i in range(syn.n_items)}
    model.prepare_item_tags(d)
    tags2 = col_tags & np.uint32(~(1 << 6) & 0xffffffff)
    got = rec(tags_any=want_any, tags_all=want_all)
    _, exp = T.topk(logits, k, tags2, want_any, want_all, rows)
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("exclude_seen", [False, True])
def test_hmf_tags_streamed_equals_materialised(dev, monkeypatch, exclude_seen):
    """The streaming node (a first chunk of 1536 + the tags filter GEMM; then the chunked path) against the
    materialised one, through LatentProductModel.step."""
    from arx.hmf import hmf_model as hm
    syn, mat = _hmf(4)
    monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '0')
    _, st = _hmf(4)
    assert isinstance(st.topk, hm.StreamTopK) and isinstance(mat.topk, hm.TopK)
    st.topk.chunk = 1536
    st.topk._buf = st.topk._buf[:, :1536].contiguous()
    rng = np.random.default_rng(6)
    B = mat.batch_size
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    item_tags = T.random_tags(rng, syn.n_items)
    sets = {int(u): rng.integers(0, syn.n_items, 60).tolist() for u in users}
    for m in (mat, st):
        m.prepare_item_tags(item_tags)
        if exclude_seen:
            m.prepare_recommend_exclusions(sets)
    key = 'recommend_ex_tags' if exclude_seen else 'recommend_tags'
    twin = lambda: st.topk_ex_tags if exclude_seen else st.topk_tags
    for n in range(3):
        want_any, want_all = T.random_words(np.random.default_rng(30 + n), B, zero_every=5)
        kw = dict(recommend=True, exclude_seen=exclude_seen, tags_any=want_any, tags_all=want_all)
        exp = mat.step(None, list(users), None, **kw)
        got = st.step(None, list(users), None, **kw)
        assert isinstance(twin(), hm.StreamTopK) and twin().fused and twin().chunk == 1536
        np.testing.assert_array_equal(got, exp, err_msg='call %d' % n)
    twin().fused = False
    st._plans.pop(key, None)
    np.testing.assert_array_equal(st.step(None, list(users), None, **kw), exp)


@pytest.mark.parametrize("exclude_seen", [False, True])
def test_linear_seq_tags(dev, exclude_seen):
    syn, model = _skipgram()
    B, l2i = model.batch_size, syn.logit_ind2item_ind
    rng = np.random.default_rng(9)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    ctx = syn.sample_batch(B, rng)[1][None, :]
    rec = lambda **kw: model.step(None, list(users), ctx.tolist(), recommend=True, exclude_seen=exclude_seen, **kw)
    sets = {int(u): rng.integers(0, syn.n_items, 50).tolist() for u in users}
    if exclude_seen:
        model.prepare_recommend_exclusions(sets)
    with pytest.raises(ValueError):
        rec(tags_all=1)
    plain = rec()
    logits = model.topk.inputs[0].value.cpu().numpy()
    item_tags = T.random_tags(rng, syn.n_items)
    model.prepare_item_tags(item_tags)
    rows = _row_cols(syn, sets, users) if exclude_seen else None
    for n in range(3):
        want_any, want_all = T.random_words(np.random.default_rng(40 + n), B, zero_every=5)
        got = rec(tags_any=want_any, tags_all=want_all)
        _, exp = T.topk(logits, 8, _col_tags(syn, item_tags), want_any, want_all, rows)
        np.testing.assert_array_equal(got, exp, err_msg='run %d' % n)
    np.testing.assert_array_equal(rec(), plain)
    assert 'recommend_tags' in model._plans or 'recommend_ex_tags' in model._plans


@pytest.mark.parametrize("exclude_seen", [False, True])
@pytest.mark.parametrize("stream", [False, True])
def test_seq_step_recommend_tags(dev, monkeypatch, stream, exclude_seen):
    """SeqModel.step_recommend(tags_any, tags_all): the softmax normaliser stays over the full vocabulary, so the
    probability of a winner is the one the unfiltered call reports; materialised and streamed follow the oracle."""
    syn, mat = _seq(11)
    mat._bucket(0)                                   # (materialised: built before the streaming switch below)
    if stream:
        monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '0')
    _, model = _seq(11)
    B, L = 16, 4
    if stream:
        bk = model._bucket(0)
        assert 'recommend_stream' in bk
        bk['recommend_stream'].chunk = 128
        bk['recommend_stream']._buf = bk['recommend_stream']._buf[:, :128].contiguous()
    rng = np.random.default_rng(2)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    tg = np.stack([syn.sample_batch(B, rng)[1] for _ in range(L)], 0)
    inp = np.concatenate([np.full((1, B), syn.n_items, dtype=np.int32), tg[:-1]], 0)
    positions = rng.integers(0, L, size=B).tolist()
    rec = lambda m, **kw: m.step_recommend(None, list(users), inp.tolist(), positions, 0, exclude_seen=exclude_seen,
                                           **kw)
    sets = {int(u): rng.integers(0, syn.n_items, 30).tolist() for u in users}
    if exclude_seen:
        for m in (mat, model):
            m.prepare_recommend_exclusions(sets)
    mat.step_recommend(None, list(users), inp.tolist(), positions, 0)
    logits = mat._bucket(0)['full'].value.cpu().numpy()
    with pytest.raises(ValueError):
        rec(model, tags_any=1)
    base = rec(model)
    item_tags = T.random_tags(rng, syn.n_items)
    model.prepare_item_tags(item_tags)
    col_tags = _col_tags(syn, item_tags)
    rows = [int(p) * B + i for i, p in enumerate(positions)]
    ex_rows = _row_cols(syn, sets, users) if exclude_seen else None
    for n in range(3):
        want_any, want_all = T.random_words(np.random.default_rng(50 + n), B, zero_every=5)
        want_all[3] = 0xffffffff                                   # nothing eligible: -1 tails of probability 0
        got = rec(model, tags_any=want_any, tags_all=want_all)
        _, exp = T.topk(logits[rows], 7, col_tags, want_any, want_all, ex_rows)
        for i, (u, p, idx) in enumerate(got):
            assert int(u) == int(users[i])
            np.testing.assert_array_equal(idx, exp[i], err_msg='call %d row %d' % (n, i))
            assert (p[idx < 0] == 0).all()
            both, a, b = np.intersect1d(idx, base[i][2], return_indices=True)
            if not stream:
                np.testing.assert_array_equal(p[a], base[i][1][b])     # the very same probability
            else:
                np.testing.assert_allclose(p[a], base[i][1][b], rtol=1e-6)
        assert (got[3][2] == -1).all()
    again = rec(model)
    for i in range(B):
        np.testing.assert_array_equal(again[i][2], base[i][2])
        np.testing.assert_array_equal(again[i][1], base[i][1])


def test_seq_step_recommend_tags_under_a_striped_wrapper_is_not_implemented(dev):
    """A SeqModel whose runtime carries a wrapper with its own step_recommend (arx.dist.SeqHybridParallel): tags raise
    NotImplementedError before the wrapper is called; the call without tags still goes to it."""
    syn, model = _seq(11)
    calls = []

    class _Wrapper(object):
        def step_recommend(self, *a):
            calls.append(a)
            return 'served'
    model.rt.dp = _Wrapper()
    try:
        for kw in (dict(tags_any=1), dict(tags_all=[1] * 16), dict(tags_any=0, tags_all=0)):
            with pytest.raises(NotImplementedError):
                model.step_recommend(None, list(range(16)), None, [0] * 16, 0, **kw)
        assert not calls
        assert model.step_recommend(None, list(range(16)), None, [0] * 16, 0) == 'served' and len(calls) == 1
    finally:
        model.rt.dp = None


def test_tag_argument_errors(dev):
    syn, model = _hmf(3)
    B = model.batch_size
    users = list(range(B))
    rec = lambda **kw: model.step(None, users, None, recommend=True, **kw)
    with pytest.raises(ValueError):
        rec(tags_any=1)                                           # before prepare_item_tags
    with pytest.raises(ValueError):
        model.prepare_item_tags(np.full(syn.n_items, -1))
    with pytest.raises(ValueError):
        model.prepare_item_tags({0: [32]})
    model.prepare_item_tags(np.zeros(syn.n_items, dtype=np.int64))
    before = model.att_emb.u_indices['input'].value.clone()
    for bad in (dict(tags_any=-1), dict(tags_all=2 ** 32), dict(tags_any=[1] * (B - 1)), dict(tags_all=[1] * (B + 1)),
                dict(tags_any=0.5), dict(tags_any=[2 ** 32] + [0] * (B - 1))):
        with pytest.raises(ValueError):
            rec(**bad)
    assert (model.att_emb.u_indices['input'].value == before).all()          # refused before any feed
    with pytest.raises(ValueError):
        rec(tags_any=1, exclude_seen=True)                        # no exclusion lists prepared
    got = rec(tags_any=1)                                         # every tag word is 0: nothing eligible
    assert (got == -1).all()
