"""explain_items on the GPU: arx_explain_slate through arx.ops against the float64 oracle of tests/explain_oracle.py --
bit for bit on exact-arithmetic inputs (where most bags hold tied tokens: the test of the tie rule), within the
float32 bounds on continuous ones --, its launch-shape invariance, and the model methods of LatentProductModel (HET
and MIX items) and a CBOW LinearSeq: eager, captured, replayed, after a training step, past the plan limit.

The launcher does not cap its grid (arx_explain.h: one group per (row, slot) pair, no loop over pairs), so there is no
second trip to reach and no trip rule to restate.

Shapes: B = 5 rows, C in {1, 7, 33} slots, V = 97 logit columns, 211 token rows, d in {4, 32, 64, 128, 256}; bag
lengths forced to include 1, 2, L - 1, L, L + 1 (L the lanes of a group), 64, 65 and 300."""
import types

import numpy as np
import pytest

import explain_oracle as EO

pytestmark = pytest.mark.gpu

B, V, N_TOK = 5, 97, 211
_CASES = {}


def _t(dev, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32) + np.float32(0.0)).view(np.uint32)   # (-0 -> +0)


def _device_feats(dev, feats):
    """The oracle's feature dicts as what ops.ExplainSet reads (graph.Feature's fields), tables on the device."""
    out = []
    for ft in feats:
        table = types.SimpleNamespace(E=_t(dev, ft['E']), bias=_t(dev, ft.get('b')), name='t%d' % len(out))
        maps = (_t(dev, ft.get('map')),) if ft['kind'] == 'cat' else tuple(_t(dev, ft[k]) for k in ('vals', 'starts', 'lens'))
        out.append(types.SimpleNamespace(kind=ft['kind'], table=table, maps=maps))
    return out


def _run(dev, U, dfeats, cand, T, pad=(3, 2, 5)):
    """arx_explain_slate into views of wider buffers that start from a sentinel (NaN / -7); returns the views as numpy
    after checking that the padding is intact and no sentinel is left in a view."""
    import torch
    from arx import ops
    Bq, C = cand.shape
    F = len(dfeats)
    es = ops.ExplainSet(dfeats, V)

    def wide(last, extra, dtype, fill):
        w = torch.full((Bq, C * last + extra), fill, dtype=dtype, device=dev)
        return w, torch.as_strided(w, (Bq, C, last), (C * last + extra, last, 1))
    fw, feat = wide(F, pad[0], torch.float32, float('nan'))
    bw = torch.full((Bq, C + pad[1]), float('nan'), dtype=torch.float32, device=dev)
    toks = [(None, None)] * 3
    if T:
        toks = [wide(T, pad[2], torch.float32, float('nan')), wide(T, pad[2], torch.int32, -7),
                wide(T, pad[2], torch.int32, -7)]
    ops.explain_slate(_t(dev, U), _t(dev, cand), es, T, feat, bw[:, :C], toks[0][1], toks[1][1], toks[2][1])
    got = dict(feat=feat.cpu().numpy(), bias=bw[:, :C].cpu().numpy())
    assert np.isnan(fw.cpu().numpy()[:, C * F:]).all() and np.isnan(bw.cpu().numpy()[:, C:]).all()
    assert not np.isnan(got['feat']).any() and not np.isnan(got['bias']).any()
    if T:
        for name, (w, v) in zip(('tok_val', 'tok_id', 'tok_feat'), toks):
            got[name] = v.cpu().numpy()
            tail = w.cpu().numpy()[:, C * T:]
            assert np.isnan(tail).all() if name == 'tok_val' else (tail == -7).all(), name
        assert not np.isnan(got['tok_val']).any() and (got['tok_id'] != -7).all() and (got['tok_feat'] != -7).all()
    return got


def _check_dead(got, cand, T):
    dead = (cand < 0) | (cand >= V)
    assert (got['feat'][dead] == 0).all() and (got['bias'][dead] == 0).all()
    if T:
        assert np.isneginf(got['tok_val'][dead]).all() and (got['tok_id'][dead] == -1).all() \
            and (got['tok_feat'][dead] == -1).all()
    return dead


# ---------------------------------------------------------------- 1. exact-arithmetic inputs
POW2 = [1, 2, 4, 8, 16, 32, 64, 256]


def _exact_case(d, name, C=33):
    """(U, feats, cand, oracle parts) of one dyadic case, computed once and left unchanged."""
    key = ('exact', d, name, C)
    if key not in _CASES:
        rng = np.random.default_rng(1000 + d + len(name))
        forced = {}

        def lens_of():
            lens, where = EO.forced_lengths(rng, V, POW2, 0, 0, choices=[1, 2, 4, 8])
            forced.setdefault('cols', where)
            return lens
        feats = EO.layout(rng, name, V, N_TOK, d, lens_of, dyadic=True)
        U = EO.users(rng, B, d, dyadic=True)
        cand = EO.slate(rng, B, C, V, must=forced.get('cols', ()))
        _CASES[key] = (U, feats, cand, EO.parts(U, feats, cand))
    return _CASES[key]


@pytest.mark.parametrize("name", ['id', 'mix', 'het', 'ccmm'])
@pytest.mark.parametrize("d", [4, 32, 64, 128, 256])
def test_exact_inputs_equal_the_oracle_bit_for_bit(dev, d, name):
    """Entries k / 2, biases k / 4, bag lengths powers of two (1 .. 256), F in {1, 2, 4}: every sum and product is
    exact in float32, so feat, bias and the top 16 with their ids equal the float64 oracle whatever the order of the
    adds -- and most bags hold tied contributions, which only the tie rule orders."""
    U, feats, cand, p = _exact_case(d, name)
    C, T = cand.shape[1], 16
    got = _run(dev, U, _device_feats(dev, feats), cand, T)
    dead = _check_dead(got, cand, T)
    assert dead[B - 1].all() and dead[:B - 1].any() and not dead[:B - 1].all()
    np.testing.assert_array_equal(_bits(got['feat']), _bits(p['feat']))
    np.testing.assert_array_equal(_bits(got['bias']), _bits(p['bias']))
    val, ids, fts, order = EO.top_tokens(p, B, C, T)
    if name == 'id':
        assert (ids == -1).all()
    else:
        lens = np.unique(p['len'][..., EO.LAYOUTS[name].index('mulhot')][~dead])
        assert set(POW2) <= set(lens.tolist()), lens              # every forced length stands in the slate
        tied = short = 0
        for (r, j), (v, i, f, pos, _) in p['tok'].items():
            o = order[(r, j)][:T + 1]
            tied += bool((np.diff(v[o]) == 0).any())
            short += len(v) < T
        assert tied >= 10 and short >= 10, (tied, short)          # ties to order; bags shorter than T: the -1 tail
    np.testing.assert_array_equal(_bits(got['tok_val']), _bits(val))
    np.testing.assert_array_equal(got['tok_id'], ids)
    np.testing.assert_array_equal(got['tok_feat'], fts)


@pytest.mark.parametrize("d,name", [(32, 'het'), (128, 'ccmm'), (4, 'mix')])
def test_exact_inputs_every_C_and_top(dev, d, name):
    """C in {1, 7, 33} x top in {0, 1, 3, 16} (the three register lists of the kernel: none, 4, 16); outputs left out
    one at a time."""
    import torch
    from arx import ops
    dfeats = None
    for C in (1, 7, 33):
        U, feats, cand, p = _exact_case(d, name, C)
        dfeats = _device_feats(dev, feats)
        if C == 1:
            cand = cand.copy()
            cand[:B - 1, 0] = [3, V - 1, 0, 50]                  # (a one-slot slate: all live but the last row)
            p = EO.parts(U, feats, cand)
        for T in (0, 1, 3, 16):
            got = _run(dev, U, dfeats, cand, T)
            _check_dead(got, cand, T)
            np.testing.assert_array_equal(_bits(got['feat']), _bits(p['feat']))
            np.testing.assert_array_equal(_bits(got['bias']), _bits(p['bias']))
            if T:
                val, ids, fts, _ = EO.top_tokens(p, B, C, T)
                np.testing.assert_array_equal(_bits(got['tok_val']), _bits(val))
                np.testing.assert_array_equal(got['tok_id'], ids)
                np.testing.assert_array_equal(got['tok_feat'], fts)
    # any output may be left out
    es = ops.ExplainSet(dfeats, V)
    Ud, cd = _t(dev, U), _t(dev, cand)
    only_bias = torch.full(cand.shape, float('nan'), dtype=torch.float32, device=dev)
    ops.explain_slate(Ud, cd, es, 3, None, only_bias)
    np.testing.assert_array_equal(_bits(only_bias.cpu().numpy()), _bits(p['bias']))
    only_feat = torch.full(cand.shape + (len(feats),), float('nan'), dtype=torch.float32, device=dev)
    ops.explain_slate(Ud, cd, es, 0, only_feat)
    np.testing.assert_array_equal(_bits(only_feat.cpu().numpy()), _bits(p['feat']))
    tv = torch.full(cand.shape + (2,), float('nan'), dtype=torch.float32, device=dev)
    ti = torch.full(cand.shape + (2,), -7, dtype=torch.int32, device=dev)
    tf = torch.full(cand.shape + (2,), -7, dtype=torch.int32, device=dev)
    ops.explain_slate(Ud, cd, es, 2, None, None, tv, ti, tf)
    val, ids, fts, _ = EO.top_tokens(p, B, cand.shape[1], 2)
    np.testing.assert_array_equal(_bits(tv.cpu().numpy()), _bits(val))
    np.testing.assert_array_equal(ti.cpu().numpy(), ids)
    np.testing.assert_array_equal(tf.cpu().numpy(), fts)
    with pytest.raises(ValueError):
        ops.explain_slate(Ud, cd, es, 2, None, None, tv, None, tf)


def test_a_nan_never_enters_and_a_repeat_counts_twice(dev):
    E = np.zeros((4, 4), dtype=np.float32)
    E[:, 0] = [1.0, 2.0, np.nan, -np.inf]
    feats = [dict(kind='mulhot', E=E, b=None, vals=np.array([1, 2, 0, 1, 3, 2, 2], dtype=np.int32),
                  starts=np.array([0, 5], dtype=np.int32), lens=np.array([5, 2], dtype=np.int32))]
    U = np.array([[1.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    import torch
    from arx import ops
    es = ops.ExplainSet(_device_feats(dev, feats), 2)
    tv = torch.zeros((1, 2, 6), dtype=torch.float32, device=dev)
    ti = torch.zeros((1, 2, 6), dtype=torch.int32, device=dev)
    tf = torch.zeros((1, 2, 6), dtype=torch.int32, device=dev)
    ops.explain_slate(_t(dev, U), _t(dev, np.array([[0, 1]], dtype=np.int32)), es, 6, None, None, tv, ti, tf)
    assert ti.cpu().numpy()[0].tolist() == [[1, 1, 0, 3, -1, -1], [-1] * 6]
    assert tf.cpu().numpy()[0].tolist() == [[0, 0, 0, 0, -1, -1], [-1] * 6]
    np.testing.assert_array_equal(tv.cpu().numpy()[0, 0], np.array([0.4, 0.4, 0.2, -np.inf, -np.inf, -np.inf],
                                                                  dtype=np.float32))
    assert np.isneginf(tv.cpu().numpy()[0, 1]).all()


# ---------------------------------------------------------------- 2. continuous inputs
# (d, layout, seed): the seeds were picked with the oracle alone (no device) so that at most 2 % of the B * C = 165
# slots have a near-tie among their first T + 1 tokens: with seed 0 none of them has one (seeds 1 .. 3 leave out 0 .. 3
# slots at d = 64 and 256); the count is asserted below all the same
CONT = [(4, 'het', 0), (32, 'het', 0), (64, 'het', 0), (128, 'het', 0), (256, 'het', 0), (32, 'f3', 0),
        (64, 'ccmm', 0), (128, 'mix', 0), (32, 'id', 0)]
T_CONT = 3
MAX_LEFT_OUT = 0.02


def _cont_case(d, name, seed, C=33):
    key = ('cont', d, name, seed, C)
    if key not in _CASES:
        rng = np.random.default_rng([seed, d, len(name)])
        L = EO.lanes(d)
        forced_len = sorted({n for n in (1, 2, L - 1, L, L + 1, 64, 65, 300, 15, 16, 17, 70) if n > 0})
        forced = {}

        def lens_of():
            lens, where = EO.forced_lengths(rng, V, forced_len, 1, 40)
            forced.setdefault('cols', where)
            return lens
        feats = EO.layout(rng, name, V, N_TOK, d, lens_of)
        U = EO.users(rng, B, d)
        cand = EO.slate(rng, B, C, V, must=forced.get('cols', ()))
        p = EO.parts(U, feats, cand)
        _CASES[key] = (U, feats, cand, p, forced_len)
    return _CASES[key]


def _pool_on_device(dev, dfeats):
    """(P [V, d], pbias [V]) as EntityEmbed.forward forms the item pool: the gather kernels, 1 / F each."""
    import torch
    from arx import ops
    F, d = len(dfeats), int(dfeats[0].table.E.shape[1])
    ids = torch.arange(V, dtype=torch.int32, device=dev)
    P = torch.empty((V, d), dtype=torch.float32, device=dev)
    pb = torch.empty(V, dtype=torch.float32, device=dev)
    for k, f in enumerate(dfeats):
        if f.kind == 'cat':
            ops.gather_onehot(f.table.E, f.table.bias, f.maps[0], ids, P, scale=1.0 / F, accumulate=k > 0, bias_out=pb)
        else:
            ops.gather_mulhot_mean(f.table.E, f.table.bias, f.maps[0], f.maps[1], f.maps[2], ids, P, scale=1.0 / F,
                                   accumulate=k > 0, bias_out=pb)
    return P, pb


def _check_against_oracle(got, p, cand, d, T, score=None, what=''):
    """feat, its sum, bias and (given) the pooled score within their bounds of the float64 oracle; the token ids on
    every slot without a near-tie.  Returns the number of slots left out of the id comparison."""
    Bq, C = cand.shape
    F = p['feat'].shape[2]
    dead = _check_dead(got, cand, T)
    n = np.maximum(p['len'], 1)
    lim = EO.bound_feat(d, n) * p['abs_feat']
    err = np.abs(got['feat'].astype(np.float64) - p['feat'])
    print("%s d=%d: feat error / bound <= %.3g" % (what, d, float((err[~dead] / lim[~dead]).max())))
    assert (err <= lim).all()
    ref = p['feat'].sum(-1)
    assert (np.abs(got['feat'].astype(np.float64).sum(-1) - ref) <= lim.sum(-1)).all()
    # bias: len - 1 adds of the running sum, the rounded coef, the product and F - 1 adds over the features
    blim = 2.0 * (n.max(-1) + F + 1) * 2.0 ** -24 * p['abs_bias']
    assert (np.abs(got['bias'].astype(np.float64) - p['bias']) <= blim).all()
    if score is not None:
        assert np.array_equal(np.isneginf(score), dead)
        slim = EO.bound_pool_score(d, n.max(-1), F) * p['abs_feat'].sum(-1)
        serr = np.abs(np.where(dead, 0.0, score.astype(np.float64)) - ref)
        print("%s d=%d: score error / bound <= %.3g" % (what, d, float((serr[~dead] / slim[~dead]).max())))
        assert (serr <= slim).all()
    left_out = 0
    if T:
        val, ids, fts, order = EO.top_tokens(p, Bq, C, T)
        for (r, j), (v, i, f, pos, s) in p['tok'].items():
            if EO.near_tie(p, order, r, j, T, d):
                left_out += 1
                continue
            np.testing.assert_array_equal(got['tok_id'][r, j], ids[r, j], err_msg="slot %d, %d" % (r, j))
            np.testing.assert_array_equal(got['tok_feat'][r, j], fts[r, j], err_msg="slot %d, %d" % (r, j))
            o = order[(r, j)][:T]
            assert (np.abs(got['tok_val'][r, j, :len(o)].astype(np.float64) - v[o]) <= EO.bound_tok(d) * s[o]).all()
            assert np.isneginf(got['tok_val'][r, j, len(o):]).all()
    return left_out


@pytest.mark.parametrize("d,name,seed", CONT, ids=lambda x: str(x))
def test_continuous_inputs_within_the_float32_bounds(dev, d, name, seed):
    """U ~ N(0, 1), tables 0.5 N(0, 1), lengths 1 .. 40 plus 1, 2, L - 1, L, L + 1, 15, 16, 17, 64, 65, 70, 300."""
    from arx import ops
    import torch
    U, feats, cand, p, forced_len = _cont_case(d, name, seed)
    dfeats = _device_feats(dev, feats)
    got = _run(dev, U, dfeats, cand, T_CONT)
    if name != 'id':
        live = (cand >= 0) & (cand < V)
        assert set(forced_len) <= set(np.unique(p['len'][..., EO.LAYOUTS[name].index('mulhot')][live]).tolist())
    P, pb = _pool_on_device(dev, dfeats)
    sc = torch.empty(cand.shape, dtype=torch.float32, device=dev)
    ops.slate_scores(_t(dev, U), P, pb, _t(dev, cand), sc)
    left_out = _check_against_oracle(got, p, cand, d, T_CONT, sc.cpu().numpy(), name)
    print("%s d=%d: %d of %d slots left out of the id comparison" % (name, d, left_out, cand.size))
    assert left_out <= MAX_LEFT_OUT * cand.size


# ---------------------------------------------------------------- 4. launch-shape invariance
@pytest.mark.parametrize("d,name", [(32, 'f3'), (128, 'het'), (256, 'ccmm'), (4, 'het')])
def test_bits_do_not_depend_on_the_launch_shape(dev, d, name):
    """Row r alone, the slate reversed and C cut to one slot each give the bits of the big call for the same (row,
    item); every output is a view of a wider canary-filled buffer (_run checks the padding and the sentinels)."""
    U, feats, cand, p, _ = _cont_case(d, name, 0)
    dfeats = _device_feats(dev, feats)
    T = 3
    base = _run(dev, U, dfeats, cand, T)
    keys = ('feat', 'bias', 'tok_val', 'tok_id', 'tok_feat')

    def same(a, b, what):
        for k in keys:
            x, y = (a[k].view(np.uint32), b[k].view(np.uint32)) if a[k].dtype == np.float32 else (a[k], b[k])
            np.testing.assert_array_equal(x, y, err_msg="%s: %s" % (what, k))
    for r in range(B):
        one = _run(dev, U[r:r + 1], dfeats, cand[r:r + 1], T, pad=(1, 4, 2))
        same(one, {k: base[k][r:r + 1] for k in keys}, "row %d alone" % r)
    rev = _run(dev, U, dfeats, cand[:, ::-1].copy(), T, pad=(0, 1, 0))
    same(rev, {k: base[k][:, ::-1] for k in keys}, "reversed")
    for j in range(cand.shape[1]):
        cut = _run(dev, U, dfeats, cand[:, j:j + 1].copy(), T)
        same(cut, {k: base[k][:, j:j + 1] for k in keys}, "slot %d alone" % j)
    # the same item twice in a row, and more rows in front, change nothing either
    twice = np.concatenate([cand[:, :5], cand[:, :5]], axis=1)
    got = _run(dev, U, dfeats, twice, T)
    same({k: got[k][:, :5] for k in keys}, {k: got[k][:, 5:] for k in keys}, "twice")
    front = _run(dev, np.concatenate([U[::-1], U]), dfeats, np.concatenate([cand[::-1], cand]), 16)
    b16 = _run(dev, U, dfeats, cand, 16)
    same({k: front[k][B:] for k in keys}, b16, "rows in front")
    np.testing.assert_array_equal(b16['tok_id'][..., :T], base['tok_id'])      # top 3 = the head of top 16
    np.testing.assert_array_equal(b16['tok_val'][..., :T].view(np.uint32), base['tok_val'].view(np.uint32))


# ---------------------------------------------------------------- 3. against the model
def _hmf(seed, mix):
    """test_recommend_exclude_gpu._hmf at this file's sizes, with HET (id row + bag) or MIX (one bag) items."""
    from arx.utils.synthetic import SyntheticHMF
    from arx.hmf.hmf_model import LatentProductModel
    d = 32
    kw = dict(item_mix=True) if mix else dict(item_mulhot=True)
    syn = SyntheticHMF(seed=seed, n_users=60, n_items=120, logit_size=V, mulhot_vocab=N_TOK, avg_len=5, max_len=12, **kw)
    params = syn.glorot_params(d, seed=seed + 1, scale=0.5)
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind
    model = LatentProductModel(syn.n_users, syn.n_items, d, 1, B, 0.5, 1.0, syn.u_attr, syn.i_attr, i2l, l2i,
                               loss_function='ce', params=params, top_N_items=8)
    return syn, model, d


def _cbow(seed):
    """test_recommend_exclude_gpu._skipgram as a CBOW model over HET items, at this file's sizes."""
    from arx.utils.synthetic import SyntheticHMF
    from arx.word2vec import cbow_model
    d = 32
    syn = SyntheticHMF(seed=seed, n_users=60, n_items=120, logit_size=V, item_mulhot=True, mulhot_vocab=N_TOK,
                       avg_len=5, max_len=12)
    syn.u_attr.set_model_size(d)
    syn.i_attr.set_model_size(d)
    params = syn.glorot_params(d, seed=seed + 1, item_output=True, scale=0.5)
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind
    model = cbow_model.Model(syn.n_users, syn.n_items, d, B, 0.5, 1.0, syn.u_attr, syn.i_attr, i2l, l2i,
                             n_input_items=3, loss_function='ce', use_sep_item=True, top_N_items=8, params=params)
    return syn, model, d


def _model_feats(model):
    """The oracle's feature dicts read back from the pool node of the model (its tables as they are NOW)."""
    pool = model.output.inputs[1]
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    feats = []
    for f in pool.feats:
        b = host(f.table.bias) if pool.with_bias else None
        ft = dict(kind=f.kind, E=host(f.table.E), b=None if b is None else b.reshape(-1))
        if f.kind == 'cat':
            ft['map'] = host(f.maps[0])
        else:
            ft['vals'], ft['starts'], ft['lens'] = (host(m) for m in f.maps)
        feats.append(ft)
    return feats


def _slates(rng, C):
    items = rng.integers(0, V, size=(B, C)).astype(np.int64)
    if C >= 4:
        items[:, C - 1] = items[:, 0]
        items[rng.random((B, C)) < 0.1] = -1
        items[B - 1, 1:] = -1
    return items


def _check_model_call(model, explain, score, batch, items, top, d):
    import torch
    ex = explain(model, batch, items, top)
    for t, dt in ((ex.score, torch.float32), (ex.feature, torch.float32), (ex.bias, torch.float32)):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt
    F = len(ex.features)
    assert tuple(ex.score.shape) == items.shape and tuple(ex.feature.shape) == items.shape + (F,)
    pool = model.output.inputs[1]
    assert ex.features == tuple((f.kind, f.table.name) for f in pool.feats)
    got = dict(feat=ex.feature.cpu().numpy(), bias=ex.bias.cpu().numpy())
    if top:
        assert tuple(ex.token_id.shape) == items.shape + (top,) and ex.token_id.dtype == torch.int32
        got.update(tok_val=ex.token_value.cpu().numpy(), tok_id=ex.token_id.cpu().numpy(),
                   tok_feat=ex.token_feature.cpu().numpy())
    else:
        assert ex.token_value is None and ex.token_id is None and ex.token_feature is None
    sc = ex.score.cpu().numpy()
    np.testing.assert_array_equal(sc.view(np.uint32), score(model, batch, items).cpu().numpy().view(np.uint32))
    latent = model.output.inputs[0].value.cpu().numpy()
    p = EO.parts(latent, _model_feats(model), items)
    left_out = _check_against_oracle(got, p, items, d, top, sc, 'model')
    assert left_out <= max(1, MAX_LEFT_OUT * items.size)
    # the bias part is the pool bias of the item
    live = items >= 0
    pb = pool.bias_value.cpu().numpy().astype(np.float64)
    assert (np.abs(got['bias'][live] - pb[items[live]]) <= 2 * 2.0 ** -24 * p['sum_abs_b'][live]).all()
    assert (p['sum_abs_b'][live] > 0).all()
    return ex


def _same_explanation(a, b):
    assert a.features == b.features
    for x, y in zip(a[:6], b[:6]):
        assert (x is None) == (y is None)
        if x is not None:
            x, y = x.cpu().numpy(), y.cpu().numpy()
            np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                          y.view(np.uint32) if y.dtype == np.float32 else y)


def _model_rounds(make, explain, score, batch_of, train):
    syn, model, d = make()
    rng = np.random.default_rng(11)
    n_nodes = None
    for n in range(3):                                   # eager, captured, replayed: other users and items each time
        batch, items = batch_of(syn, rng), _slates(rng, 7)
        ex = _check_model_call(model, explain, score, batch, items, 3, d)
        if n == 0:
            n_nodes = len(model.rt.nodes)
    assert len(model.rt.nodes) == n_nodes                # a replay adds no node
    _, twin, _ = make()                                  # a fresh model, asked once: the replay's bits
    _same_explanation(ex, explain(twin, batch, items, 3))
    ex0 = _check_model_call(model, explain, score, batch, items, 0, d)
    np.testing.assert_array_equal(ex0.feature.cpu().numpy().view(np.uint32), ex.feature.cpu().numpy().view(np.uint32))
    keys = [q for q in model._plans if isinstance(q, tuple) and q[0] == 'explain_items']
    assert keys == [('explain_items', 7, 3), ('explain_items', 7, 0)]
    if train is not None:                                # after one training step the explanation follows the tables
        train(syn, model, rng)
        ex2 = _check_model_call(model, explain, score, batch, items, 3, d)
        assert not np.array_equal(ex2.feature.cpu().numpy(), ex.feature.cpu().numpy())
        assert not np.array_equal(ex2.bias.cpu().numpy(), ex.bias.cpu().numpy())
    # at most four plans are kept: the oldest goes first, with its nodes
    sizes = []
    for C in range(1, 8):
        explain(model, batch, np.zeros((B, C), dtype=np.int64), 1)
        sizes.append(len(model.rt.nodes))
    keys = [q for q in model._plans if isinstance(q, tuple) and q[0] == 'explain_items']
    assert keys == [('explain_items', C, 1) for C in (4, 5, 6, 7)]
    assert len(set(sizes[1:])) == 1, sizes               # (two more plans fill the four; then one out, one in)
    with pytest.raises(ValueError, match="top"):
        explain(model, batch, items, 17)
    bad = items.copy()
    bad[0, 0] = V
    with pytest.raises(ValueError):
        explain(model, batch, bad, 3)
    _check_model_call(model, explain, score, batch, items, 3, d)     # and a rebuilt plan answers as before


def _hmf_batch(syn, rng):
    return rng.choice(syn.n_users, B, replace=False).astype(np.int32)


def _hmf_train(syn, model, rng):
    users, items = syn.sample_batch(B, rng)
    model.step(None, list(users), list(items))


@pytest.mark.parametrize("mix", [False, True], ids=['het', 'mix'])
def test_hmf_explain_items_eager_captured_replayed_trained(dev, mix):
    _model_rounds(lambda: _hmf(31, mix), lambda m, u, it, top: m.explain_items(list(u), it, top=top),
                  lambda m, u, it: m.score_items(list(u), it), _hmf_batch, _hmf_train)


def test_cbow_explain_items(dev):
    def batch_of(syn, rng):
        return (rng.choice(syn.n_users, B, replace=False).astype(np.int32),
                np.stack([syn.sample_batch(B, rng)[1] for _ in range(3)]))
    _model_rounds(lambda: _cbow(41), lambda m, b, it, top: m.explain_items(list(b[0]), b[1].tolist(), it, top=top),
                  lambda m, b, it: m.score_items(list(b[0]), b[1].tolist(), it), batch_of, None)
