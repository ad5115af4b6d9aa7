"""score_items(diversify=) on the GPU: arx_slate_mmr through arx.ops against the float64 oracle of tests/mmr_oracle.py
-- exactly on data whose every float32 intermediate is representable (with and without group caps), bit for bit against
the top-k order at lambda = 1, within a derived tolerance of the float64 best on random data, independent of the
leading dimensions, of B and of the grid -- and the model methods (eager, captured, replayed with lambda and the cap
changed between replays of one plan).

On an MI355X every pick of test_random_data_picks_within_tol_of_the_float64_best and of the model tests was the float64
best itself (largest shortfall / tol = 0, printed per case), with 2.5 % / 3.25 % / 3.75 % of the steps at d = 20 / 64 /
128 inside 2 tol of a tie; the bound is 2 (3 d + 16) 2^-24, built in _tol below."""
import numpy as np
import pytest

import mmr_oracle as MO
import slate_oracle as SO

pytestmark = pytest.mark.gpu

LAMS = np.array([0.0, 0.25, 0.5, 0.75, 1.0], dtype=np.float32)
EXACT = [(1, 1, 5, 4, 1), (3, 7, 50, 20, 7), (4, 64, 300, 32, 20), (2, 256, 600, 128, 100), (2, 512, 900, 64, 100),
         (2, 300, 400, 108, 300)]
_CASES, _WANT = {}, {}
_ID = lambda s: "x".join(map(str, s))


def _t(dev, a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).to(dev)      # (a copy: broadcast views are read-only)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _mmr(dev, P, cand, sc, lam, k, groups=None, m=None):
    """(ids, values, pos) of ops.slate_mmr as numpy; the outputs start as (7777, NaN, 7777): every entry is written."""
    import torch
    from arx import ops
    B = cand.shape[0]
    ids = torch.full((B, k), 7777, dtype=torch.int32, device=dev)
    pos = torch.full((B, k), 7777, dtype=torch.int32, device=dev)
    vals = torch.full((B, k), float('nan'), dtype=torch.float32, device=dev)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float32), (B,))
    ops.slate_mmr(_t(dev, P), _t(dev, cand), _t(dev, sc), _t(dev, lam), None if groups is None else _t(dev, groups),
                  None if groups is None else _t(dev, np.broadcast_to(np.asarray(m, dtype=np.int32), (B,))), k, ids,
                  vals, pos)
    return ids.cpu().numpy(), vals.cpu().numpy(), pos.cpu().numpy()


def _tol(d):
    """What two float32 objectives may differ by against their float64 values, in units of u = 2^-24 (every term of
    the objective is at most 1 in size): 2 (d + 1) u for a float32 dot of unit rows (slate_oracle.bound), (d + 4) u for
    the two norms behind them, a few u (<= 11) for the division of rel, 1 - lambda and the combine -- (3 d + 16) u
    together --, doubled because two objectives are compared."""
    return 2.0 * (3 * d + 16) * 2.0 ** -24


# ---------------------------------------------------------------- exact data
def _axis_pool(rng, V, d):
    """Rows 2^e times one signed axis vector, e in {-1, 0, 1, 2}; row 0 is the zero row.  Norms are exact
    (similar.hip) and every cosine is exactly -1, 0 or 1 (a -1 never shows: pen starts at 0)."""
    P = np.zeros((V, d), dtype=np.float32)
    P[np.arange(V), rng.integers(0, d, V)] = (2.0 ** rng.integers(-1, 3, V)) * rng.choice([1.0, -1.0], V, p=[0.8, 0.2])
    P[0] = 0.0
    return P


def _eighths(rng, cand, V, tie=()):
    """Scores k / 8 in [0, 8]; the slots `tie` of row 0 share one score; 0 and 8 on two other live slots of every row
    with two or more, so that rel = s / 8 exactly."""
    sc = (rng.integers(0, 65, size=cand.shape) / 8.0).astype(np.float32)
    sc[rng.random(cand.shape) < 0.05] = -np.inf                      # a dead slot with a valid id
    sc[0, list(tie)] = 4.0
    for r in range(cand.shape[0]):
        live = np.nonzero((cand[r] >= 0) & (cand[r] < V) & np.isfinite(sc[r]))[0]
        if r == 0:
            live = live[~np.isin(live, list(tie))]
        if len(live) >= 2:
            a, b = rng.choice(live, 2, replace=False)
            sc[r, a], sc[r, b] = 0.0, 8.0
    return sc


def _exact(shape):
    """(P, cand, sc, lam, groups, m) of one shape, built once and left unchanged.  Row 0 is an ordinary row; with two
    or more rows, row 1 has fewer than k live slots; with three or more the last row is all dead."""
    if shape not in _CASES:
        B, C, V, d, k = shape
        rng = np.random.default_rng(sum(shape))
        P = _axis_pool(rng, V, d)
        cand = rng.integers(0, V, size=(B, C)).astype(np.int32)
        kind = rng.random((B, C))
        cand[kind < 0.08] = -1
        cand[(kind >= 0.08) & (kind < 0.12)] = V + 2
        cand[(kind >= 0.12) & (kind < 0.14)] = V
        cand[(kind >= 0.14) & (kind < 0.16)] = SO.KEY_NONE
        if C >= 4:
            cand[0, 1] = cand[0, 3] = 1 + (V - 1) // 2               # one item in two slots
            cand[0, 2] = 0                                           # the zero row
        if C == 1:
            cand[0, 0] = V - 1
        if B >= 2:
            cand[1, max(1, k // 2):] = -1
        if B >= 3:
            cand[B - 1, ::2] = -1
        sc = _eighths(rng, cand, V, (1, 3) if C >= 4 else ())        # ... with one score
        if B >= 3:
            sc[B - 1, 1::2] = -np.inf
        lam = LAMS[(np.arange(B) + sum(shape)) % 5]
        groups = rng.integers(0, 4, V).astype(np.int32)
        groups[rng.random(V) < 0.15] = -1
        groups[rng.random(V) < 0.03] = -9                            # (any negative id is 'no group')
        m = np.array([1, 3, 2], dtype=np.int32)[np.arange(B) % 3]
        _CASES[shape] = (P, cand, sc, lam, groups, m)
    return _CASES[shape]


def _want(shape, capped):
    if (shape, capped) not in _WANT:
        P, cand, sc, lam, groups, m = _exact(shape)
        _WANT[shape, capped] = MO.select(cand, sc, P, lam, shape[4], groups if capped else None, m if capped else None)
    return _WANT[shape, capped]


def _live(shape):
    P, cand, sc = _exact(shape)[:3]
    return (cand >= 0) & (cand < shape[2]) & np.isfinite(sc)


@pytest.mark.parametrize("shape", EXACT, ids=_ID)
def test_exact_data_equals_the_oracle(dev, shape):
    B, C, V, d, k = shape
    P, cand, sc, lam, _, _ = _exact(shape)
    live = _live(shape)
    assert live[0].any() and (B < 2 or live[1].sum() < k) and (B < 3 or not live[B - 1].any())
    assert ((cand >= V) & np.isfinite(sc)).any() or C < 64           # (an id past the pool with a finite score)
    wi, wv, wp = _want(shape, False)
    ids, vals, pos = _mmr(dev, P, cand, sc, lam, k)
    np.testing.assert_array_equal(pos, wp)
    np.testing.assert_array_equal(ids, wi)
    np.testing.assert_array_equal(_bits(vals), _bits(wv))
    # the first pick is the best-scored live slot; a row short of live slots ends in (-1, -inf, -1)
    for r in range(B):
        n = int(live[r].sum())
        if n:
            assert vals[r, 0] == sc[r][live[r]].max()
        assert (ids[r, min(n, k):] == -1).all() and (pos[r, min(n, k):] == -1).all()
        assert np.isneginf(vals[r, min(n, k):]).all() and (pos[r, :min(n, k)] >= 0).all()


@pytest.mark.parametrize("shape", EXACT, ids=_ID)
def test_exact_data_with_group_caps(dev, shape):
    B, C, V, d, k = shape
    P, cand, sc, lam, groups, m = _exact(shape)
    live = _live(shape)
    wi, wv, wp = _want(shape, True)
    ids, vals, pos = _mmr(dev, P, cand, sc, lam, k, groups, m)
    np.testing.assert_array_equal(pos, wp)
    np.testing.assert_array_equal(ids, wi)
    np.testing.assert_array_equal(_bits(vals), _bits(wv))
    assert m[0] == 1 and len(set(m.tolist())) == min(B, 3)
    for r in range(B):
        got = ids[r][ids[r] >= 0]
        g = groups[got]
        for q in set(g[g >= 0].tolist()):
            assert (g == q).sum() <= m[r], (r, q)
    if C >= 64:
        # row 0, m = 1: four groups and the ungrouped items run out although more slots are live, and the ungrouped
        # items are taken more than once
        got = ids[0][ids[0] >= 0]
        assert 0 < len(got) < min(k, live[0].sum()) and (pos[0, len(got):] == -1).all()
        assert np.isneginf(vals[0, len(got):]).all() and (groups[got] < 0).sum() > 1


# ---------------------------------------------------------------- lambda = 1 is the top-k order
@pytest.mark.parametrize("shape", [(3, 100, 500, 20, 50), (2, 512, 900, 64, 100), (2, 256, 600, 128, 256)], ids=_ID)
def test_lambda_one_equals_topk_bit_for_bit(dev, shape):
    import torch
    from arx.slate import slate_order
    B, C, V, d, k = shape
    rng = np.random.default_rng(sum(shape) + 1)
    P = rng.standard_normal((V, d)).astype(np.float32)
    cand = rng.integers(-1, V, size=(B, C)).astype(np.int32)
    sc = rng.standard_normal((B, C)).astype(np.float32)
    sc[:, 5] = sc[:, 0]                                              # ties ...
    sc[:, C - 1] = sc[:, 0]
    sc[:, 7] = np.nextafter(sc[:, 6], np.float32(4))                 # ... and neighbours one ulp apart
    sc[:, 9] = np.nextafter(sc[:, 8], np.float32(-4))
    sc[0, 20:30] = sc[0, 20]
    cand[:, [0, 5, 6, 7, 8, 9, C - 1]] = 3
    cand[B - 1, 40:] = -1                                            # fewer than k live
    sc[cand < 0] = -np.inf                                           # (as arx_slate_scores leaves an empty slot)
    ids, vals, pos = _mmr(dev, P, cand, sc, 1.0, k)
    dsc, dcand = _t(dev, sc), _t(dev, cand)
    tv = torch.empty((B, k), dtype=torch.float32, device=dev)
    tp = torch.empty((B, k), dtype=torch.int32, device=dev)
    ti = torch.empty((B, k), dtype=torch.int32, device=dev)
    slate_order(dsc, dcand, k, tv, tp, ti)
    np.testing.assert_array_equal(ids, ti.cpu().numpy())
    np.testing.assert_array_equal(_bits(vals), _bits(tv.cpu().numpy()))
    full = ids >= 0
    np.testing.assert_array_equal(pos[full], tp.cpu().numpy()[full])
    assert (~full[B - 1]).any() and (pos[~full] == -1).all()
    wi, wv = SO.order(sc, cand, k)
    np.testing.assert_array_equal(ids, wi)


# ---------------------------------------------------------------- random data
def _normal(seed, B, C, V, d):
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((B, d)).astype(np.float32)
    P = rng.standard_normal((V, d)).astype(np.float32)
    b = rng.standard_normal(V).astype(np.float32)
    cand = np.stack([rng.choice(V, C, replace=False) for _ in range(B)]).astype(np.int32)
    cand[:, 3] = -1
    cand[:, 11] = cand[:, 10]                                        # one item in two slots
    groups = rng.integers(-1, 12, V).astype(np.int32)
    return U, P, b, cand, groups


def _judge(cand, sc, P, lam, groups, m, ids, vals, pos, d, what):
    """The picks against the float64 replay: eligible, within tol of the best, and THE best wherever the best is
    clear.  Returns the share of steps with a float64 top-two gap <= 2 tol."""
    tol = _tol(d)
    pick, best, gap, want, ok = MO.replay(cand, sc, P, lam, groups, m, pos)
    assert ok.all(), what
    took = pos >= 0
    assert (np.take_along_axis(cand, np.where(took, pos, 0), 1)[took] == ids[took]).all()
    assert (_bits(np.take_along_axis(sc, np.where(took, pos, 0), 1)[took]) == _bits(vals[took])).all()
    assert (ids[~took] == -1).all() and np.isneginf(vals[~took]).all()
    for r in range(pos.shape[0]):
        assert len(set(pos[r][took[r]].tolist())) == took[r].sum()
    short = (best - pick)[took]
    print("%s: largest shortfall / tol = %.3g" % (what, float(short.max() / tol)))
    assert (short <= tol).all(), what
    clear = took & (gap > 2 * tol)
    np.testing.assert_array_equal(pos[clear], want[clear], err_msg=what)
    return float((took & ~clear).sum()) / max(1, int(took.sum()))


@pytest.mark.parametrize("case", [(20, 100, 50, 0.3), (64, 512, 100, 0.5), (128, 256, 100, 0.7)], ids=_ID)
def test_random_data_picks_within_tol_of_the_float64_best(dev, case):
    """At every step the float64 objective of the device's pick is within _tol(d) of the float64 best over the
    eligible slots, given the device's own earlier picks; where the float64 top two are more than 2 tol apart the pick
    is the oracle's.  So that the tolerance hides nothing, fewer than 10 % of the steps may be that close (a numpy
    run of these seeds: 0 - 4 %)."""
    import torch
    from arx import ops
    d, C, k, lam = case
    B, V = 4, 3000
    U, P, b, cand, groups = _normal(1000 + d, B, C, V, d)
    dsc = torch.empty((B, C), dtype=torch.float32, device=dev)
    ops.slate_scores(_t(dev, U), _t(dev, P), _t(dev, b), _t(dev, cand), dsc)
    sc = dsc.cpu().numpy()
    ids, vals, pos = _mmr(dev, P, cand, sc, lam, k)
    share = _judge(cand, sc, P, lam, None, None, ids, vals, pos, d, "d=%d" % d)
    print("d=%d: steps with a top-two gap <= 2 tol: %.2f %%" % (d, 100 * share))
    assert share < 0.10
    m = np.array([1, 2, 3, 50], dtype=np.int32)
    ids, vals, pos = _mmr(dev, P, cand, sc, lam, k, groups, m)
    _judge(cand, sc, P, lam, groups, m, ids, vals, pos, d, "d=%d capped" % d)
    assert (pos[0] == -1).any() and (pos[3] >= 0).all()              # (twelve groups, m = 1: the row runs out)


# ---------------------------------------------------------------- a row's outputs depend on that row only
@pytest.mark.parametrize("case", [(20, 100, 40), (128, 256, 60)], ids=_ID)
def test_outputs_do_not_depend_on_leading_dimensions_or_other_rows(dev, case):
    import torch
    from arx import ops
    d, C, k = case
    B, V = 3, 1500
    U, P, b, cand, groups = _normal(2000 + d, B, C, V, d)
    rng = np.random.default_rng(d)
    sc = rng.standard_normal((B, C)).astype(np.float32)
    sc[cand < 0] = -np.inf
    lam = np.array([0.3, 0.6, 0.9], dtype=np.float32)
    m = np.array([2, 1, 3], dtype=np.int32)
    base = _mmr(dev, P, cand, sc, lam, k, groups, m)
    # strided views, the padding kept
    Pw = torch.full((V, d + 8), 9.0, dtype=torch.float32, device=dev)
    cw = torch.full((B, C + 3), 1, dtype=torch.int32, device=dev)
    sw = torch.full((B, C + 5), 9.0, dtype=torch.float32, device=dev)
    iw = torch.full((B, k + 3), 7777, dtype=torch.int32, device=dev)
    vw = torch.full((B, k + 5), float('nan'), dtype=torch.float32, device=dev)
    pw = torch.full((B, k + 4), 7777, dtype=torch.int32, device=dev)
    Pw[:, :d], cw[:, :C], sw[:, :C] = _t(dev, P), _t(dev, cand), _t(dev, sc)
    ops.slate_mmr(Pw[:, :d], cw[:, :C], sw[:, :C], _t(dev, lam), _t(dev, groups), _t(dev, m), k, iw[:, :k], vw[:, :k],
                  pw[:, :k])
    iw, vw, pw = iw.cpu().numpy(), vw.cpu().numpy(), pw.cpu().numpy()
    for got, want in zip((iw[:, :k], vw[:, :k], pw[:, :k]), base):
        np.testing.assert_array_equal(_bits(got), _bits(want))
    assert (iw[:, k:] == 7777).all() and np.isnan(vw[:, k:]).all() and (pw[:, k:] == 7777).all()
    # five other rows in front
    cand2 = np.concatenate([rng.integers(0, V, size=(5, C)).astype(np.int32), cand])
    sc2 = np.concatenate([rng.standard_normal((5, C)).astype(np.float32), sc])
    lam2 = np.concatenate([np.full(5, 0.5, dtype=np.float32), lam])
    m2 = np.concatenate([np.full(5, 2, dtype=np.int32), m])
    for got, want in zip(_mmr(dev, P, cand2, sc2, lam2, k, groups, m2), base):
        np.testing.assert_array_equal(_bits(got[5:]), _bits(want))
    # inside a larger B
    where = np.array([7, 300, 611])
    n = 700
    cand3 = rng.integers(-1, V, size=(n, C)).astype(np.int32)
    sc3 = rng.standard_normal((n, C)).astype(np.float32)
    lam3 = rng.random(n).astype(np.float32)
    m3 = rng.integers(1, 4, n).astype(np.int32)
    cand3[where], sc3[where], lam3[where], m3[where] = cand, sc, lam, m
    for got, want in zip(_mmr(dev, P, cand3, sc3, lam3, k, groups, m3), base):
        np.testing.assert_array_equal(_bits(got[where]), _bits(want))


# ---------------------------------------------------------------- the row loop past the grid cap
def _mmr_grid_cap():
    """diverse.hip, arx_slate_mmr: one workgroup per row, `cap = cu_count() * 8` workgroups at most."""
    from arx import ops
    return ops.device_info()["cu_count"] * 8


def test_rows_past_the_grid_cap_take_further_trips(dev):
    cap = _mmr_grid_cap()
    C, V, d, k = 8, 20, 4, 3
    B = 2 * cap + 3
    assert B > 2 * cap                                               # (third trip of the row loop for three blocks)
    rng = np.random.default_rng(6)
    P = _axis_pool(rng, V, d)
    cand = rng.integers(-1, V + 1, size=(B, C)).astype(np.int32)
    cand[:, 0] = rng.integers(0, V, B)
    cand[:, 1] = rng.integers(0, V, B)
    cand[5] = -1
    sc = (rng.integers(0, 65, size=(B, C)) / 8.0).astype(np.float32)
    sc[:, 0], sc[:, 1] = 8.0, 0.0                                    # (rel = s / 8 exactly)
    lam = LAMS[rng.integers(0, 5, B)]
    wi, wv, wp = MO.select(cand, sc, P, lam, k)
    ids, vals, pos = _mmr(dev, P, cand, sc, lam, k)
    np.testing.assert_array_equal(pos, wp)
    np.testing.assert_array_equal(ids, wi)
    np.testing.assert_array_equal(_bits(vals), _bits(wv))
    assert (ids[5] == -1).all() and (ids[B - 1] >= 0).any() and (ids[cap:] >= 0).any()


# ---------------------------------------------------------------- models
def _node(model, C, k, capped):
    return model._plans[('score_items', C, k, 'mmr', capped)].fetch[0]


def _model_rounds(model, recommend, score, batches, V, d, top_n, n_items):
    """score(batch, cand, k, **kw).  Four calls of one uncapped plan (eager, captured, two replays with another
    lambda) and four of one capped plan (lambda and the cap changed between replays), each judged against the replay
    of the device's own scores; recommend's output as the slate; the refusals."""
    import torch
    from arx.slate import item_group_ids
    rng = np.random.default_rng(31)
    B, k = model.batch_size, 10
    slates = []
    for batch in batches:
        rec = recommend(batch)
        slates.append(np.concatenate([rec, rng.integers(0, V, size=(B, 12)), rec[:, :4], np.full((B, 4), -1)],
                                     axis=1).astype(np.int64))
    C = slates[0].shape[1]
    pool = model.output.inputs[1].value.cpu().numpy()                # (the item latents recommend just scored against)
    assert pool.shape == (V, d)
    with pytest.raises(ValueError, match="prepare_item_groups"):
        score(batches[0], slates[0], k, max_per_group=2)
    before = score(batches[0], slates[0], k)
    lams = [0.7, 0.7, 0.3, np.linspace(0.0, 1.0, B).astype(np.float32)]
    for n, lam in enumerate(lams):
        batch, cand = batches[n % len(batches)], slates[n % len(batches)]
        sc = score(batch, cand, None).cpu().numpy()
        ids, vals = score(batch, cand, k, diversify=lam)
        assert isinstance(ids, torch.Tensor) and ids.is_cuda and ids.dtype == torch.int32 and tuple(ids.shape) == (B, k)
        node = _node(model, C, k, False)
        assert node.pos is not None and tuple(node.top_ids.shape) == (B, k)
        _judge(cand.astype(np.int32), sc, pool, lam, None, None, ids.cpu().numpy(), vals.cpu().numpy(),
               node.pos.cpu().numpy(), d, "uncapped call %d" % n)
    # groups per ITEM index, mapped to logit columns
    g_items = rng.integers(-1, 5, n_items)
    model.prepare_item_groups(g_items)
    groups = model._item_groups.cpu().numpy()
    np.testing.assert_array_equal(groups, item_group_ids(g_items, model.att_emb._item2logit_np, V))
    assert groups.dtype == np.int32 and groups.shape == (V,)
    caps = [2, 2, 1, rng.integers(1, 4, B)]
    for n, (lam, m) in enumerate(zip([0.7, 0.4, 0.4, lams[3]], caps)):
        batch, cand = batches[n % len(batches)], slates[n % len(batches)]
        sc = score(batch, cand, None).cpu().numpy()
        ids, vals = score(batch, cand, k, diversify=lam, max_per_group=m)
        ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
        _judge(cand.astype(np.int32), sc, pool, lam, groups, m, ids, vals, _node(model, C, k, True).pos.cpu().numpy(),
               d, "capped call %d" % n)
        mm = np.broadcast_to(np.asarray(m), (B,))
        for r in range(B):
            g = groups[ids[r][ids[r] >= 0]]
            assert all((g == q).sum() <= mm[r] for q in set(g[g >= 0].tolist()))
    # a cap alone is lambda = 1: the best k by score under the cap
    batch, cand = batches[0], slates[0]
    sc = score(batch, cand, None).cpu().numpy()
    ids, vals = score(batch, cand, k, max_per_group=1)
    wi, wv, _ = MO.select(cand, sc, pool, 1.0, k, groups, 1)
    np.testing.assert_array_equal(ids.cpu().numpy(), wi)
    np.testing.assert_array_equal(vals.cpu().numpy(), wv)
    # and lambda = 1 alone is the plain order
    ids, vals = score(batch, cand, k, diversify=1.0)
    np.testing.assert_array_equal(ids.cpu().numpy(), before[0].cpu().numpy())
    np.testing.assert_array_equal(vals.cpu().numpy(), before[1].cpu().numpy())
    # recommend's output is a slate as it stands
    rec = recommend(batch)
    sc = score(batch, rec, None).cpu().numpy()
    ids, vals = score(batch, rec, 5, diversify=0.7)
    _judge(rec.astype(np.int32), sc, pool, 0.7, None, None, ids.cpu().numpy(), vals.cpu().numpy(),
           _node(model, top_n, 5, False).pos.cpu().numpy(), d, "recommend as the slate")
    # new groups: the capped plans go, the others stay
    keys = [q for q in model._plans if isinstance(q, tuple)]
    assert ('score_items', C, k, 'mmr', True) in keys and ('score_items', C, k, 'mmr', False) in keys
    model.prepare_item_groups({i: int(g) for i, g in enumerate(rng.integers(0, 3, n_items))})
    keys = [q for q in model._plans if isinstance(q, tuple)]
    assert not [q for q in keys if len(q) == 5 and q[4]] and ('score_items', C, k, 'mmr', False) in keys
    groups2 = model._item_groups.cpu().numpy()
    assert not np.array_equal(groups, groups2)
    sc = score(batch, cand, None).cpu().numpy()
    ids, vals = score(batch, cand, k, diversify=0.5, max_per_group=2)
    _judge(cand.astype(np.int32), sc, pool, 0.5, groups2, 2, ids.cpu().numpy(), vals.cpu().numpy(),
           _node(model, C, k, True).pos.cpu().numpy(), d, "after new groups")
    # diversify=None is the call it was
    after = score(batches[0], slates[0], k)
    np.testing.assert_array_equal(after[0].cpu().numpy(), before[0].cpu().numpy())
    np.testing.assert_array_equal(_bits(after[1].cpu().numpy()), _bits(before[1].cpu().numpy()))
    wi, wv = SO.order(score(batches[0], slates[0], None).cpu().numpy(), slates[0], k)
    np.testing.assert_array_equal(after[0].cpu().numpy(), wi)
    # refusals, before any feed
    for kw in (dict(diversify=1.5), dict(diversify=-0.1), dict(diversify=float('nan')), dict(diversify=True),
               dict(diversify=[0.5] * (B - 1)), dict(max_per_group=0), dict(diversify=0.5, max_per_group=1.5)):
        with pytest.raises(ValueError):
            score(batch, cand, k, **kw)
    with pytest.raises(ValueError):
        score(batch, cand, None, diversify=0.5)                      # k is required
    with pytest.raises(ValueError, match="arx_slate_mmr_supported"):
        score(batch, np.zeros((B, 513), dtype=np.int64), 5, diversify=0.5)
    return C, k


def test_hmf_score_items_diversify(dev):
    from arx.slate import MAX_PLANS
    from test_recommend_exclude_gpu import _hmf
    syn, model = _hmf(3)
    B, V, d, top_n = model.batch_size, model.logit_size, 32, 30
    rng = np.random.default_rng(5)
    batches = [rng.choice(syn.n_users, B, replace=False).astype(np.int32) for _ in range(3)]
    C, k = _model_rounds(model, lambda u: model.step(None, list(u), None, recommend=True),
                         lambda u, c, kk, **kw: model.score_items(list(u), c, k=kk, **kw), batches, V, d, top_n,
                         syn.n_items)
    # the diversified plans count toward the eight: a ninth (C, k) evicts the oldest
    keys = [q for q in model._plans if isinstance(q, tuple)]
    assert len(keys) <= MAX_PLANS
    n = 1
    while len([q for q in model._plans if isinstance(q, tuple)]) < MAX_PLANS:
        model.score_items(list(batches[0]), np.zeros((B, n), dtype=np.int64), k=1, diversify=0.5)
        n += 1
    keys = [q for q in model._plans if isinstance(q, tuple)]
    assert len(keys) == MAX_PLANS
    n_nodes = len(model.rt.nodes)
    model.score_items(list(batches[0]), np.zeros((B, 100), dtype=np.int64), k=2, diversify=0.5)
    now = [q for q in model._plans if isinstance(q, tuple)]
    assert len(now) == MAX_PLANS and keys[0] not in now and now[-1] == ('score_items', 100, 2, 'mmr', False)
    assert now[:-1] == keys[1:] and len(model.rt.nodes) <= n_nodes + 4


def test_linear_seq_score_items_diversify(dev):
    from test_recommend_exclude_gpu import _skipgram
    syn, model = _skipgram()
    B, V, d, top_n = model.batch_size, model.logit_size, 32, 8
    rng = np.random.default_rng(9)
    batches = [(rng.choice(syn.n_users, B, replace=False).astype(np.int32), syn.sample_batch(B, rng)[1][None, :])
               for _ in range(3)]
    _model_rounds(model, lambda b: model.step(None, list(b[0]), b[1].tolist(), recommend=True),
                  lambda b, c, kk, **kw: model.score_items(list(b[0]), b[1].tolist(), c, k=kk, **kw), batches, V, d,
                  top_n, syn.n_items)
