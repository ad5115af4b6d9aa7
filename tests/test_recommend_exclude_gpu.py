"""Recommend without each user's seen items (exclude_seen), on the GPU.

The oracle ranks the DEVICE's own logits in numpy: the row's excluded columns set to -inf, a stable sort by
(-value, column), the first k, -inf entries -> index -1.  Indices are compared exactly.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ml1m_small')


def oracle_topk(logits, ex_lists, k):
    """logits [B, V] numpy; ex_lists[r]: the excluded columns of row r -> (values [B, k], indices [B, k])."""
    x = np.array(logits, dtype=np.float32, copy=True)
    for r, cols in enumerate(ex_lists):
        if len(cols):
            x[r, np.asarray(cols, dtype=np.int64)] = -np.inf
    B, V = x.shape
    kth = np.partition(x, V - k, axis=1)[:, V - k]
    vals = np.empty((B, k), dtype=np.float32)
    inds = np.empty((B, k), dtype=np.int64)
    for r in range(B):
        c = np.nonzero(x[r] >= kth[r])[0]
        o = np.lexsort((c, -x[r, c]))[:k]
        vals[r], inds[r] = x[r, c[o]], c[o]
    inds[np.isneginf(vals)] = -1
    return vals, inds


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    cols = np.concatenate([np.sort(np.asarray(x, dtype=np.int32)) for x in lists] + [np.zeros(1, np.int32)])
    return ptr, cols


def _const(rt, t, bias=None):
    """a graph node holding a given device tensor (and a column bias, for a pool)"""
    from arx import graph as G

    class _Const(G.Node):
        def forward(self, train):
            pass
    n = _Const(rt, tuple(t.shape))
    n.value, n.bias_value = t, bias
    return n


class _Rig(object):
    """A latent [B, d] and an item pool [V, d] + bias as graph nodes, the device logits of the chunked scorer and
    the exclusion lists of the rows."""

    def __init__(self, B, V, d, seed):
        import torch
        from arx import graph as G
        from arx import ops
        self.rt = rt = G.Runtime()
        g = torch.Generator(device='cpu').manual_seed(seed)
        lat = torch.randn(B, d, generator=g).to(rt.device)
        pool = (torch.randn(V, d, generator=g) * 0.5).to(rt.device)
        bias = (torch.randn(V, generator=g) * 0.5).to(rt.device)
        self.latent, self.pool = _const(rt, lat), _const(rt, pool, bias)
        # logits the way the streaming node's chunks compute them (the fused GEMM's values are bit-identical)
        ch = 65536
        buf = torch.empty((B, min(ch, V)), dtype=torch.float32, device=rt.device)
        out = np.empty((B, V), dtype=np.float32)
        for c0 in range(0, V, ch):
            c1 = min(V, c0 + ch)
            ops.gemm(lat, pool[c0:c1], buf[:, :c1 - c0], rt.ws, transB=True, col_bias=bias[c0:c1])
            out[:, c0:c1] = buf[:, :c1 - c0].cpu().numpy()
        self.logits = out

    def exclusions(self, keys, lists):
        """rows keyed by user keys[r] (-1: none); lists[u]: user u's excluded columns."""
        import torch
        ptr, cols = _csr(lists)
        dev = self.rt.device
        self.ex = (torch.from_numpy(np.asarray(keys, dtype=np.int32)).to(dev), len(keys),
                   torch.from_numpy(ptr).to(dev), torch.from_numpy(cols).to(dev))
        return [lists[u] if u >= 0 else [] for u in keys]


def _adversarial(logits, rng, n_top=50, n_first=20, n_rest=20, first=65536):
    """per row: its own n_top best columns + random ones inside the first chunk and after it"""
    B, V = logits.shape
    top = np.argpartition(-logits, n_top, axis=1)[:, :n_top]
    out = []
    for r in range(B):
        extra = [rng.integers(0, min(first, V), n_first)]
        if V > first:
            extra.append(rng.integers(first, V, n_rest))
        out.append(np.unique(np.concatenate([top[r]] + extra)))
    return out


# ---------------------------------------------------------------- kernels
def test_exclude_fill_matches_numpy(dev):
    import torch
    from arx import ops
    rng = np.random.default_rng(0)
    B, V, key_rows = 96, 3000, 40                    # key_rows < B: row r uses row_keys[r % key_rows]
    n_users = 30
    lists = [np.unique(rng.integers(0, V, rng.integers(0, 200))) for _ in range(n_users)]
    lists[3] = np.zeros(0, dtype=np.int64)           # an empty list
    lists[4] = np.arange(0, V, 3)                    # a long one, cut by every range
    keys = rng.integers(0, n_users, key_rows).astype(np.int32)
    keys[[1, 7, 20]] = -1                            # negative keys: nothing excluded
    keys[2] = 3
    keys[5] = 4
    ptr, cols = _csr(lists)
    d_keys, d_ptr, d_cols = (torch.from_numpy(a).to(dev) for a in (keys, ptr, cols))
    x0 = rng.standard_normal((B, V)).astype(np.float32)
    for col0, ncols in ((0, V), (0, 1000), (1000, 1000), (1777, 1223), (2999, 1), (1500, 0)):
        sub = torch.from_numpy(x0).to(dev)[:, col0:col0 + ncols]          # a strided view: ld = V
        ops.topk_exclude_fill(sub, col0, (d_keys, key_rows, d_ptr, d_cols))
        got = sub.cpu().numpy()
        exp = x0[:, col0:col0 + ncols].copy()
        for r in range(B):
            u = keys[r % key_rows]
            if u < 0:
                continue
            c = lists[u]
            c = c[(c >= col0) & (c < col0 + ncols)]
            exp[r, c - col0] = -np.inf
        np.testing.assert_array_equal(got, exp, err_msg=str((col0, ncols)))


def test_materialised_topk_short_rows_end_in_minus_one(dev):
    """TopK with exclusions: rows with fewer than k eligible columns get -inf / -1 tails; the others follow the
    oracle, ties included."""
    import torch
    from arx.hmf import hmf_model as hm
    rig = _Rig(64, 300, 32, seed=1)
    rig.logits[:, 200:220] = rig.logits[:, 10:11]                       # ties across the row
    x = torch.from_numpy(rig.logits).to(dev)
    rng = np.random.default_rng(1)
    lists = [np.unique(rng.integers(0, 300, 40)) for _ in range(64)]
    lists[5] = np.arange(0, 300)                                         # nothing left
    lists[6] = np.setdiff1d(np.arange(300), [17, 250, 3])                # three left
    lists[7] = np.arange(0, 250)                                         # fifty left
    keys = np.arange(64)[::-1].copy()
    keys[9] = -1
    row_lists = rig.exclusions(keys, lists)
    k = 100
    node = hm.TopK(rig.rt, _const(rig.rt, x), k, exclude=lambda: rig.ex)
    node.forward(False)
    ev, ei = oracle_topk(rig.logits, row_lists, k)
    gv, gi = node.value.cpu().numpy(), node.indices.cpu().numpy()
    np.testing.assert_array_equal(gi, ei)
    np.testing.assert_array_equal(gv, ev)
    assert (gi[58] == -1).all() and np.isneginf(gv[58]).all()           # (row 58 is user 5)
    assert sorted(gi[57][:3].tolist()) == [3, 17, 250] and (gi[57][3:] == -1).all()


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("k", [1, 30, 100])
def test_stream_topk_excluding_equals_oracle(dev, d, k):
    """StreamTopK at V = 200 000 (a first chunk + the fused filter GEMM), B = 256, with bias; adversarial
    histories (each row's own top 50 + random columns in and after the first chunk): fused (no overflow) and
    chunked both give the oracle's indices, values to 1e-6."""
    from arx.hmf import hmf_model as hm
    B, V = 256, 200000
    rig = _Rig(B, V, d, seed=d + k)
    rng = np.random.default_rng(k)
    user_lists = _adversarial(rig.logits, rng)
    keys = rng.permutation(B + 20)[:B].astype(np.int32)                # users; the ones >= B have no history
    lists = [np.zeros(0, np.int64)] * (B + 20)
    for r in range(B):
        if keys[r] < B:
            lists[keys[r]] = user_lists[r]
    keys[::17] = -1
    row_lists = rig.exclusions(keys, lists)
    ev, ei = oracle_topk(rig.logits, row_lists, k)
    node = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, exclude=lambda: rig.ex)
    assert node.fused
    for fused in (True, False):
        node.fused = fused
        node.forward(False)
        if fused:
            assert not node.overflowed()
        gv, gi = node.value.cpu().numpy(), node.indices.cpu().numpy()
        np.testing.assert_array_equal(gi, ei, err_msg='fused=%s' % fused)
        np.testing.assert_allclose(gv, ev, rtol=1e-6, err_msg='fused=%s' % fused)
        for r in range(0, B, 31):
            assert not np.isin(gi[r], row_lists[r]).any()


def test_history_covering_the_first_chunk_takes_the_chunked_route(dev):
    """A user whose history covers the whole first chunk leaves that row's threshold at -inf: the fused run
    overflows, and the chunked path (what LatentProductModel.step re-runs) gives the oracle's answer."""
    from arx.hmf import hmf_model as hm
    B, V, k = 128, 150000, 30
    rig = _Rig(B, V, 64, seed=7)
    rng = np.random.default_rng(7)
    lists = _adversarial(rig.logits, rng)
    lists[3] = np.arange(0, 65536 - 10)                                 # more than chunk - k columns
    row_lists = rig.exclusions(np.arange(B, dtype=np.int32), lists)
    node = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, exclude=lambda: rig.ex)
    node.forward(False)
    assert node.overflowed()
    node.fused = False
    node.forward(False)
    ev, ei = oracle_topk(rig.logits, row_lists, k)
    np.testing.assert_array_equal(node.indices.cpu().numpy(), ei)
    np.testing.assert_allclose(node.value.cpu().numpy(), ev, rtol=1e-6)


# ---------------------------------------------------------------- models
CFG = dict(n_users=200, n_items=5000, logit_size=4800)


def _hmf(seed, B=32, top_n=30, d=32):
    from arx.utils.synthetic import SyntheticHMF
    from arx.hmf.hmf_model import LatentProductModel
    syn = SyntheticHMF(seed=seed, **CFG)
    params = syn.glorot_params(d, seed=seed + 1, scale=0.5)
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind
    model = LatentProductModel(syn.n_users, syn.n_items, d, 1, B, 0.5, 1.0, syn.u_attr, syn.i_attr, i2l, l2i,
                               loss_function='ce', params=params, top_N_items=top_n)
    return syn, model


def _item_lists(syn, model, users, rng, n_rand=40):
    """{user: items}: the user's positives, random items (some without a logit), and the items of the user's
    own 10 best logit columns (what a trained model would recommend)"""
    top = model.step(None, list(users), None, recommend=True)
    l2i = syn.logit_ind2item_ind
    pos = syn.positives_dict()
    out = {}
    for r, u in enumerate(users):
        its = list(pos.get(int(u), [])) + rng.integers(0, syn.n_items, n_rand).tolist()
        its += [int(l2i[c]) for c in top[r][:10]]
        out[int(u)] = its
    return out


def _row_cols(syn, item_sets, users):
    i2l = syn.item_ind2logit_ind_dict()
    return [sorted({i2l[i] for i in item_sets.get(int(u), []) if i in i2l}) for u in users]


def test_hmf_exclude_seen_end_to_end(dev):
    from arx.hmf import hmf_model as hm
    syn, model = _hmf(3)
    _, plain = _hmf(3)                                         # the same model, no exclusions ever prepared
    assert isinstance(model.topk, hm.TopK)
    B = model.batch_size
    rng = np.random.default_rng(5)
    batches = [rng.choice(syn.n_users, B, replace=False).astype(np.int32) for _ in range(4)]
    sets = {}
    for users in batches:
        sets.update(_item_lists(syn, model, users, rng))
    with pytest.raises(ValueError):
        model.step(None, list(batches[0]), None, recommend=True, exclude_seen=True)
    model.prepare_recommend_exclusions(sets)
    for n, users in enumerate(batches[:3]):                    # eager, captured, replayed
        base = model.step(None, list(users), None, recommend=True)
        np.testing.assert_array_equal(base, plain.step(None, list(users), None, recommend=True))
        logits = model.topk.inputs[0].value.cpu().numpy()
        got = model.step(None, list(users), None, recommend=True, exclude_seen=True)
        rows = _row_cols(syn, sets, users)
        _, exp = oracle_topk(logits, rows, model.topk.k)
        np.testing.assert_array_equal(got, exp, err_msg='batch %d' % n)
        for r in range(B):
            assert not np.isin(got[r], rows[r]).any()
    # without the flag: still the plain result, bit for bit
    users = batches[3]
    np.testing.assert_array_equal(model.step(None, list(users), None, recommend=True),
                                  plain.step(None, list(users), None, recommend=True))
    # a second prepare replaces the lists (the captured plan with the old pointers is dropped)
    sets2 = {int(u): rng.integers(0, syn.n_items, 300).tolist() for u in users}
    model.prepare_recommend_exclusions(sets2)
    model.step(None, list(users), None, recommend=True)
    logits = model.topk.inputs[0].value.cpu().numpy()
    got = model.step(None, list(users), None, recommend=True, exclude_seen=True)
    _, exp = oracle_topk(logits, _row_cols(syn, sets2, users), model.topk.k)
    np.testing.assert_array_equal(got, exp)


def test_hmf_exclude_seen_streamed_equals_materialised(dev, monkeypatch):
    """The streaming node (fused: a first chunk of 1536 + the filter GEMM; and the chunked fallback) against the
    materialised one, through LatentProductModel.step."""
    from arx.hmf import hmf_model as hm
    syn, mat = _hmf(4)
    monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '0')
    _, st = _hmf(4)
    assert isinstance(st.topk, hm.StreamTopK) and isinstance(mat.topk, hm.TopK)
    st.topk.chunk = 1536
    st.topk._buf = st.topk._buf[:, :1536].contiguous()
    rng = np.random.default_rng(6)
    users = rng.choice(syn.n_users, mat.batch_size, replace=False).astype(np.int32)
    sets = _item_lists(syn, mat, users, rng)
    for m in (mat, st):
        m.prepare_recommend_exclusions(sets)
    exp = mat.step(None, list(users), None, recommend=True, exclude_seen=True)
    for rep in range(2):
        got = st.step(None, list(users), None, recommend=True, exclude_seen=True)
        assert st.topk_ex.fused and int(st.topk_ex.overflow.item()) == 0
        np.testing.assert_array_equal(got, exp, err_msg='replay %d' % rep)
    st.topk_ex.fused = False
    st._plans.pop('recommend_ex', None)
    np.testing.assert_array_equal(st.step(None, list(users), None, recommend=True, exclude_seen=True), exp)
    # the chunked fallback after an overflow: one user excludes all of the first chunk
    st.topk_ex.fused = True
    st.topk_ex.slack, st.topk_ex.min_capp = 0.0, 8          # segments shorter than the columns of a range
    st._plans.pop('recommend_ex', None)
    sets[int(users[0])] = [int(i) for i in syn.logit_ind2item_ind[:1536]]
    for m in (mat, st):
        m.prepare_recommend_exclusions(sets)
    exp = mat.step(None, list(users), None, recommend=True, exclude_seen=True)
    got = st.step(None, list(users), None, recommend=True, exclude_seen=True)
    np.testing.assert_array_equal(got, exp)
    assert int(st.topk_ex.overflow.item()) != 0 and st.topk_ex.fused     # (overflowed, re-ran chunked, restored)


def _seq(seed, B=16, L=4, size=64):
    from arx.attributes.embed_attribute import EmbeddingAttribute
    from arx.lstm.seqModel import SeqModel
    from arx.utils.synthetic import SyntheticHMF
    syn = SyntheticHMF(seed=seed, n_users=300, n_items=500, logit_size=500)
    syn.u_attr.set_model_size(size)
    syn.i_attr.set_model_size(size)
    params = syn.glorot_params(size, seed=seed + 1, scale=0.4)
    rng = np.random.default_rng(seed + 2)
    params['lstm_w'] = (rng.standard_normal((2 * size, 4 * size)) * 0.15).astype(np.float32)
    params['lstm_b'] = (rng.standard_normal((4 * size,)) * 0.05).astype(np.float32)
    i2l = syn.item_ind2logit_ind_dict()
    i2l[syn.n_items] = 0
    emb = EmbeddingAttribute(syn.u_attr, syn.i_attr, B, None, L, False, i2l, syn.logit_ind2item_ind, params=params)
    model = SeqModel([L], size, 1, 5.0, B, 0.5, 0.83, emb, loss='ce', START_ID=syn.n_items, params=params)
    model.topk_n = 7
    return syn, model


@pytest.mark.parametrize("stream", [False, True])
def test_seq_step_recommend_exclude_seen(dev, monkeypatch, stream):
    """SeqModel.step_recommend(exclude_seen=True): the softmax normaliser stays over the full vocabulary, so the
    probability of every item is the one the non-excluding call reports; materialised and streamed agree."""
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
    plain = mat.step_recommend(None, list(users), inp.tolist(), positions, 0)
    logits = mat._bucket(0)['full'].value.cpu().numpy()
    lse = mat._bucket(0)['recommend'].lse.cpu().numpy()
    l2i = syn.logit_ind2item_ind
    sets = {int(u): [int(l2i[c]) for c in plain[i][2][:4]] + rng.integers(0, syn.n_items, 30).tolist()
            for i, u in enumerate(users)}
    sets[int(users[1])] = [int(x) for x in l2i[:497]]                 # three items left: -1 / 0 tails
    with pytest.raises(ValueError):
        model.step_recommend(None, list(users), inp.tolist(), positions, 0, exclude_seen=True)
    for m in (mat, model):
        m.prepare_recommend_exclusions(sets)
    base = model.step_recommend(None, list(users), inp.tolist(), positions, 0)
    for rep in range(2):
        got = model.step_recommend(None, list(users), inp.tolist(), positions, 0, exclude_seen=True)
        rows = [int(p) * B + i for i, p in enumerate(positions)]
        _, exp = oracle_topk(logits[rows], _row_cols(syn, sets, users), 7)
        for i, (u, p, idx) in enumerate(got):
            assert int(u) == int(users[i])
            np.testing.assert_array_equal(idx, exp[i], err_msg='row %d' % i)
            ok = idx >= 0
            ref_p = np.exp(logits[rows[i], idx[ok]] - lse[rows[i]])
            np.testing.assert_allclose(p[ok], ref_p, rtol=1e-5 if stream else 0, atol=0)
            assert (p[~ok] == 0).all()
            both, a, b = np.intersect1d(idx, base[i][2], return_indices=True)
            if not stream:
                np.testing.assert_array_equal(p[a], base[i][1][b])     # the very same probability
            else:
                np.testing.assert_allclose(p[a], base[i][1][b], rtol=1e-6)
        assert (got[1][2][3:] == -1).all() and (got[1][2][:3] >= 0).all()


def test_seq_overflow_reruns_on_the_chunked_path(dev, monkeypatch):
    """SeqModel.step_recommend when the fused candidate lists overflow: one user excludes the whole first chunk, so
    that row's threshold is -inf and every 64-column range behind the chunk exceeds its 8-entry segment -- the call
    runs once more on the chunked path and gives what the materialised model gives."""
    syn, mat = _seq(11)
    mat._bucket(0)                                   # (materialised: built before the streaming switch below)
    monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '0')
    _, model = _seq(11)
    B, L = 16, 4
    bk = model._bucket(0)
    assert 'recommend_stream' in bk and 'recommend_stream' not in mat._bucket(0)
    bk['recommend_stream'].chunk = 128
    bk['recommend_stream']._buf = bk['recommend_stream']._buf[:, :128].contiguous()
    rng = np.random.default_rng(2)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    tg = np.stack([syn.sample_batch(B, rng)[1] for _ in range(L)], 0)
    inp = np.concatenate([np.full((1, B), syn.n_items, dtype=np.int32), tg[:-1]], 0)
    positions = rng.integers(0, L, size=B).tolist()
    l2i = syn.logit_ind2item_ind
    sets = {int(u): rng.integers(0, syn.n_items, 30).tolist() for u in users}
    for m in (mat, model):
        m.prepare_recommend_exclusions(sets)
    rec = lambda m: m.step_recommend(None, list(users), inp.tolist(), positions, 0, exclude_seen=True)
    rec(model)                                       # (builds the excluding twin)
    node = bk['recommend_ex']
    node.slack, node.min_capp = 0.0, 8               # segments shorter than the columns of a range
    bk['plans'].pop('recommend_ex', None)
    sets[int(users[0])] = [int(i) for i in l2i[:128]]
    for m in (mat, model):
        m.prepare_recommend_exclusions(sets)
    exp, got = rec(mat), rec(model)
    assert int(node.overflow.item()) != 0 and node.fused     # (overflowed, re-ran chunked, restored)
    for i in range(B):
        assert int(got[i][0]) == int(exp[i][0]) == int(users[i])
        np.testing.assert_array_equal(got[i][2], exp[i][2], err_msg='row %d' % i)
        np.testing.assert_allclose(got[i][1], exp[i][1], rtol=1e-5, atol=0, err_msg='row %d' % i)
    assert (got[0][2] >= 128).all()


def _skipgram():
    from arx.utils.synthetic import SyntheticHMF
    from arx.word2vec import skipgram_model
    syn = SyntheticHMF(seed=21, n_users=300, n_items=500, logit_size=400)
    d, B = 32, 32
    syn.u_attr.set_model_size(d)
    syn.i_attr.set_model_size(d)
    params = syn.glorot_params(d, seed=22, item_output=True, scale=0.5)
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind
    model = skipgram_model.Model(syn.n_users, syn.n_items, d, B, 0.5, 1.0, syn.u_attr, syn.i_attr, i2l, l2i,
                                 n_input_items=1, loss_function='ce', use_sep_item=True, top_N_items=8,
                                 params=params)
    return syn, model


def test_linear_seq_exclude_seen(dev):
    syn, model = _skipgram()
    B, l2i = model.batch_size, syn.logit_ind2item_ind
    rng = np.random.default_rng(9)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    ctx = syn.sample_batch(B, rng)[1][None, :]
    with pytest.raises(ValueError):
        model.step(None, list(users), ctx.tolist(), recommend=True, exclude_seen=True)
    plain = model.step(None, list(users), ctx.tolist(), recommend=True)
    logits = model.topk.inputs[0].value.cpu().numpy()
    sets = {int(u): [int(l2i[c]) for c in plain[i][:3]] + rng.integers(0, syn.n_items, 50).tolist()
            for i, u in enumerate(users)}
    model.prepare_recommend_exclusions(sets)
    for rep in range(3):
        got = model.step(None, list(users), ctx.tolist(), recommend=True, exclude_seen=True)
        _, exp = oracle_topk(logits, _row_cols(syn, sets, users), 8)
        np.testing.assert_array_equal(got, exp, err_msg='run %d' % rep)
    np.testing.assert_array_equal(model.step(None, list(users), ctx.tolist(), recommend=True), plain)


def test_linear_seq_overflow_reruns_on_the_chunked_path(dev, monkeypatch):
    """LinearSeq.step(recommend, exclude_seen) when the fused candidate lists overflow (the construction of
    test_hmf_exclude_seen_streamed_equals_materialised): the streamed model against the materialised twin."""
    from arx.hmf import hmf_model as hm
    syn, mat = _skipgram()
    monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '0')
    _, st = _skipgram()
    assert isinstance(st.topk, hm.StreamTopK) and isinstance(mat.topk, hm.TopK)
    st.topk.chunk = 128
    st.topk._buf = st.topk._buf[:, :128].contiguous()
    B, l2i = mat.batch_size, syn.logit_ind2item_ind
    rng = np.random.default_rng(9)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    ctx = syn.sample_batch(B, rng)[1][None, :]
    sets = {int(u): rng.integers(0, syn.n_items, 50).tolist() for u in users}
    for m in (mat, st):
        m.prepare_recommend_exclusions(sets)
    rec = lambda m: m.step(None, list(users), ctx.tolist(), recommend=True, exclude_seen=True)
    np.testing.assert_array_equal(rec(st), rec(mat))         # (builds the excluding twin)
    assert isinstance(st.topk_ex, hm.StreamTopK) and st.topk_ex.fused
    st.topk_ex.slack, st.topk_ex.min_capp = 0.0, 8           # segments shorter than the columns of a range
    st._plans.pop('recommend_ex', None)
    sets[int(users[0])] = [int(i) for i in l2i[:128]]        # all of the first chunk: that row's threshold is -inf
    for m in (mat, st):
        m.prepare_recommend_exclusions(sets)
    exp, got = rec(mat), rec(st)
    assert int(st.topk_ex.overflow.item()) != 0 and st.topk_ex.fused     # (overflowed, re-ran chunked, restored)
    np.testing.assert_array_equal(got, exp)
    assert (got[0] >= 128).all()


def test_ml1m_excluding_equals_host_side_removal(dev, tmp_path):
    """The set-up of test_train_recommend_evaluate_loop: after training, recommending top_n with the training
    history excluded equals recommending top_n + max|history| without it, dropping the history on the host and
    keeping the first top_n -- for every user, top_n distinct unseen items each."""
    import shutil
    from arx.attributes.input_attribute import read_data
    from arx.hmf.hmf_model import LatentProductModel
    from arx.utils.evaluate import Evaluation
    raw = str(tmp_path / 'raw')
    shutil.copytree(DATA, raw)
    V, d, B, top_n = 400, 32, 32, 30
    (data_tr, data_va, u_attr, i_attr, i2l, l2i, user_index, item_index) = read_data(
        raw, str(tmp_path / 'cache'), 'het', V, 1, mylog=lambda m: None)
    data_tr = [p for p in data_tr if p[1] in i2l]
    hist = {}
    for u, i, _ in data_tr:
        hist.setdefault(u, set()).add(i)
    k_wide = min(top_n + max(len(h) for h in hist.values()), len(l2i))
    models = [LatentProductModel(len(user_index), len(item_index), d, 1, B, 1.0, 1.0, u_attr, i_attr, i2l, l2i,
                                 loss_function='ce', top_N_items=k, seed=3) for k in (top_n, k_wide)]
    np.random.seed(0)
    for step in range(400):
        users, items, _ = models[0].get_permuted_batch(data_tr)
        models[0].step(None, users, items, loss='ce')
    _copy_tables(models[0], models[1])
    models[0].prepare_recommend_exclusions(hist)
    uids = Evaluation(raw, test=False).get_uids()
    uinds = [user_index[u] for u in uids]
    n_checked = 0
    for s in range(0, len(uinds), B):
        chunk = uinds[s:s + B]
        users = chunk + [0] * (B - len(chunk))
        ex = models[0].step(None, users, None, None, forward_only=True, recommend=True, exclude_seen=True)
        wide = models[1].step(None, users, None, None, forward_only=True, recommend=True)
        for r, u in enumerate(chunk):
            seen = {i2l[i] for i in hist.get(u, ())}
            host = [int(c) for c in wide[r] if int(c) not in seen][:top_n]
            assert ex[r].tolist() == host, u
            assert len(set(host)) == top_n and not seen & set(host)
            n_checked += 1
    assert n_checked == len(uinds) > 0


def _copy_tables(src, dst):
    """dst's tables := src's (the wide model recommends with the trained parameters)."""
    assert list(src.att_emb.tables) == list(dst.att_emb.tables)
    for name, a in src.att_emb.tables.items():
        b = dst.att_emb.tables[name]
        b.E.copy_(a.E)
        if a.bias is not None:
            b.bias.copy_(a.bias)
