"""score_items(sample_temperature=) on the device (include/arx_slate_sample.h): arx_slate_sample against the float64
oracle of tests/slate_sample_oracle.py -- ids / pos / values exactly, logp within
2^-20 (1 + (smax - smin) / tau) + 2^-22 |logp| + C 2^-24 --, the same draw as the sampled recommend's dense path, the
grid-stride trips, the law tied to the reported propensities, and the two models.  The noise is the device's own:
arx_topk_gumbel_add with tau = 1 over a zero [rows, V] matrix, indexed by candidate id."""
import numpy as np
import pytest

import slate_oracle as SO
import slate_sample_oracle as SS

pytestmark = pytest.mark.gpu

TAUS = np.array([0.0, 0.05, 1.0, 50.0], dtype=np.float32)
V_NOISE = 2048
KEY_NONE = 0x7FFFFFFF
_NOISE = {}
WORST = {"ratio": 0.0, "where": ""}      # the largest |logp error| / tolerance seen (printed by the last kernel test)


def _t(dev, a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _words(seed):
    return np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint32).view(np.int32)


def _noise(dev, rows, V, seed):
    """g [rows, V] float32: the device's noise of noise row r and column c."""
    import torch
    from arx import ops
    key = (rows, V, seed)
    if key not in _NOISE:
        x = torch.zeros((rows, V), dtype=torch.float32, device=dev)
        ops.topk_gumbel_add(x, 0, (torch.ones(rows, dtype=torch.float32, device=dev), rows, _t(dev, _words(seed))))
        _NOISE[key] = x.cpu().numpy()
    return _NOISE[key]


def _run(dev, cand, sc, tau, seed, k, tau_rows=None, want_logp=True, pad=(3, 5, 2, 1, 4, 6)):
    """(ids, values, pos, logp or None) of ops.slate_sample as numpy.  Every 2-D argument is a view of a wider buffer
    (leading dimensions larger than C and k); the outputs start as (7777, NaN, 7777, NaN): every entry is written."""
    import torch
    from arx import ops
    B, C = cand.shape
    wide = lambda a, p, fill: torch.full((B, a + p), fill, device=dev,
                                         dtype=torch.float32 if isinstance(fill, float) else torch.int32)[:, :a]
    cd, sd = wide(C, pad[0], -5), wide(C, pad[1], float('nan'))
    cd.copy_(_t(dev, cand.astype(np.int32)))
    sd.copy_(_t(dev, sc.astype(np.float32)))
    ids, vals, pos = wide(k, pad[2], 7777), wide(k, pad[3], float('nan')), wide(k, pad[4], 7777)
    lp = wide(k, pad[5], float('nan')) if want_logp else None
    tau = np.ascontiguousarray(tau, dtype=np.float32)
    ops.slate_sample(cd, sd, (_t(dev, tau), len(tau) if tau_rows is None else tau_rows, _t(dev, _words(seed))), k, ids,
                     vals, pos, lp)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), vals.cpu().numpy(), pos.cpu().numpy(), None if lp is None else lp.cpu().numpy()


def _slot_noise(G, cand):
    """g [B, C]: the noise of every slot's item, noise row r % len(G) (0 where the id has no column)."""
    B = cand.shape[0]
    ok = (cand >= 0) & (cand < G.shape[1])
    return np.where(ok, G[np.arange(B)[:, None] % G.shape[0], np.where(ok, cand, 0)], np.float32(0))


def _check(cand, sc, tau_row, g, k, out, what):
    """Everything the header promises for one launch, every row: ids / pos / values exactly the oracle's, values the
    bits of scores[pos]; logp against the float64 oracle on the device's own order, finite, not above 0 by more than
    the tolerance, 0 on tau == 0 rows and in the padding."""
    ids, vals, pos, lp = out
    C = cand.shape[1]
    wi, wv, wp = SS.select(cand, sc, g, tau_row, k)
    np.testing.assert_array_equal(pos, wp, err_msg=what)
    np.testing.assert_array_equal(ids, wi, err_msg=what)
    np.testing.assert_array_equal(_bits(vals), _bits(wv), err_msg=what)
    real = pos >= 0
    took = np.take_along_axis(sc.astype(np.float32), np.where(real, pos, 0), 1)
    assert (_bits(vals)[real] == _bits(took)[real]).all(), what
    if lp is None:
        return
    want = SS.logprob(cand, sc, tau_row, pos)
    tol = SS.tolerance(cand, sc, tau_row, want, C)
    assert np.isfinite(lp).all(), what
    assert (lp[~real] == 0).all() and (lp[np.asarray(tau_row) == 0] == 0).all(), what
    err = np.abs(lp.astype(np.float64) - want)
    hot = real & (np.asarray(tau_row)[:, None] > 0)
    if hot.any():
        ratio = np.where(hot, err / np.where(tol > 0, tol, 1.0), 0.0)
        r, t = np.unravel_index(ratio.argmax(), ratio.shape)
        if ratio[r, t] > WORST["ratio"]:
            WORST.update(ratio=float(ratio[r, t]), where="%s row %d pick %d tau %g" % (what, r, t, tau_row[r]))
        assert (err[hot] <= tol[hot]).all(), "%s: logp off by %.3g of its tolerance at row %d pick %d" % (
            what, ratio[r, t], r, t)
        assert (lp[hot] <= tol[hot]).all(), what


# ---------------------------------------------------------------- 1. parity
def _rows(seed, B, C, V=V_NOISE):
    """cand / scores [B, C] and tau [B].  The score is a function of (row, id): copies of an id carry the same bits.
    Row 0: empty slots, NaN / -inf / +inf scores, an id without a pool row, one id three times; row 1: all empty; row 2:
    at most three live slots; row 3: all scores equal at tau = 0, with repeated ids; row 4: the same at tau = 1."""
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((B, V)).astype(np.float32)
    cand = rng.integers(0, V, size=(B, C)).astype(np.int32)
    tau = TAUS[(np.arange(B) + 1) % 4].copy()
    table[0, cand[0, :3]] = [np.nan, -np.inf, np.inf][:min(3, C)]
    cand[0, rng.random(C) < 0.1] = -1
    if C >= 8:
        cand[0, [4, C // 2, C - 1]] = cand[0, 5] if cand[0, 5] >= 0 else 9
        cand[0, 6] = KEY_NONE
    if B > 1:
        cand[1] = -1
    if B > 2:
        cand[2, max(1, min(C // 2, 3)):] = -1
    for r, t in ((3, 0.0), (4, 1.0)):
        if B > r:
            table[r] = np.float32(0.75)
            cand[r, ::3] = cand[r, 0]
            tau[r] = t
    ok = (cand >= 0) & (cand < V)
    sc = np.where(ok, np.take_along_axis(table, np.where(ok, cand, 0), 1), np.float32(-np.inf)).astype(np.float32)
    return cand, sc, tau


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 257, 1000, 1024])
def test_kernel_equals_the_oracle(dev, C):
    from arx import ops
    assert ops.slate_sample_supported(C) and (C < 1024 or not ops.slate_sample_supported(C + 1))   # the largest
    for B in (1, 3, 130):
        cand, sc, tau = _rows(100 + C, B, C)
        g = _slot_noise(_noise(dev, B, V_NOISE, 11 + B), cand)
        for k in sorted({1, min(C, 30), C}):
            out = _run(dev, cand, sc, tau, 11 + B, k)
            _check(cand, sc, tau, g, k, out, "C=%d B=%d k=%d" % (C, B, k))
            if B == 130 and C >= 8:
                ids, _, pos, _ = out
                assert (ids[1] == -1).all() and (pos[2, min(k, 3):] == -1).all()
                n3 = len(np.unique(cand[3]))                         # the all-equal rows: slate order, every id once
                assert (pos[3, :min(k, n3)] == np.sort(np.nonzero(SS.competitors(cand[3], sc[3]))[0])[:k]).all()
            if k == min(C, 30):                                      # logp = NULL: the other three are what they were
                bare = _run(dev, cand, sc, tau, 11 + B, k, want_logp=False)
                for a, b in zip(bare[:3], out[:3]):
                    np.testing.assert_array_equal(_bits(a), _bits(b))


def test_noise_rows_repeat_with_tau_rows(dev):
    """tau_rows < B: row r draws at tau[r % tau_rows] with the noise row r % tau_rows."""
    B, C, k, rows = 10, 50, 20, 5
    cand, sc, _ = _rows(7, B, C)
    cand[5:], sc[5:] = cand[:5], sc[:5]
    tau = TAUS[[1, 2, 3, 1, 2]]
    out = _run(dev, cand, sc, tau, 77, k, tau_rows=rows)
    _check(cand, sc, np.tile(tau, 2), _slot_noise(_noise(dev, rows, V_NOISE, 77), cand), k, out, "tau_rows")
    for a in out:
        np.testing.assert_array_equal(_bits(a[:5]), _bits(a[5:]))


# ---------------------------------------------------------------- 2. the sampled recommend's draw
def test_same_draw_as_the_dense_sampled_recommend(dev):
    import torch
    from arx import ops
    B, V, k, seed = 6, 700, 50, 2 ** 33 + 5
    rng = np.random.default_rng(3)
    logits = rng.standard_normal((B, V)).astype(np.float32)
    tau = np.array([0.0, 0.05, 1.0, 50.0, 0.3, 2.0], dtype=np.float32)
    cand = np.tile(np.arange(V, dtype=np.int32), (B, 1))
    ids, vals, pos, lp = _run(dev, cand, logits, tau, seed, k)
    x = _t(dev, logits)
    sample = (_t(dev, tau), B, _t(dev, _words(seed)))
    ops.topk_gumbel_add(x, 0, sample)
    kv = torch.empty((B, k), dtype=torch.float32, device=dev)
    ki = torch.empty((B, k), dtype=torch.int32, device=dev)
    ops.topk(x, k, kv, ki)
    np.testing.assert_array_equal(ids, ki.cpu().numpy())
    np.testing.assert_array_equal(pos, ids)
    np.testing.assert_array_equal(_bits(vals), _bits(np.take_along_axis(logits, ids.astype(np.int64), 1)))
    # the order of the slate plays no part: the same ids, pos through the permutation
    perm = np.stack([rng.permutation(V) for _ in range(B)]).astype(np.int32)
    inv = np.argsort(perm, axis=1)
    pids, pvals, ppos, plp = _run(dev, perm, np.take_along_axis(logits, perm.astype(np.int64), 1), tau, seed, k)
    np.testing.assert_array_equal(pids, ids)
    np.testing.assert_array_equal(ppos, np.take_along_axis(inv, pos.astype(np.int64), 1))
    np.testing.assert_array_equal(_bits(pvals), _bits(vals))
    tol = SS.tolerance(cand, logits, tau, lp, V)
    assert (np.abs(plp.astype(np.float64) - lp) <= 2 * tol).all()


# ---------------------------------------------------------------- 3. logp
def test_logp_first_and_last_pick_and_the_extremes(dev):
    B, C = 8, 300
    rng = np.random.default_rng(17)
    cand = np.stack([rng.permutation(V_NOISE)[:C] for _ in range(B)]).astype(np.int32)
    sc = rng.standard_normal((B, C)).astype(np.float32)
    sc[2:4] = rng.uniform(-15, 15, (2, C)).astype(np.float32)
    sc[6] += 1000.0                                  # a large common offset: only differences may matter
    tau = np.array([0.05, 1.0, 1e-3, 1e-3, 1e6, 1e6, 0.05, 50.0], dtype=np.float32)
    cand[3, 100:] = -1
    cand[5, 40:] = -1
    G = _noise(dev, B, V_NOISE, 5)
    g = _slot_noise(G, cand)
    out = _run(dev, cand, sc, tau, 5, C)
    _check(cand, sc, tau, g, C, out, "logp k=C")
    ids, vals, pos, lp = out
    n = (pos >= 0).sum(axis=1)
    assert n.tolist() == [C, C, C, 100, C, 40, C, C]
    want = SS.logprob(cand, sc, tau, pos)
    tol = SS.tolerance(cand, sc, tau, want, C)
    for r in range(B):
        # the last real pick at k = C is certain; the first is the log-softmax of its score
        assert abs(lp[r, n[r] - 1]) <= tol[r, n[r] - 1]
        a = sc[r, :n[r]].astype(np.float64) / float(tau[r])
        first = a[pos[r, 0]] - (a.max() + np.log(np.exp(a - a.max()).sum()))
        assert abs(lp[r, 0] - first) <= tol[r, 0]
    assert np.isfinite(lp[2:4]).all() and (lp[2:4] <= tol[2:4]).all()                 # tau = 1e-3 over +-15
    for r in (4, 5):                                                                  # tau = 1e6: uniform
        np.testing.assert_allclose(lp[r, :n[r]], -np.log(n[r] - np.arange(n[r])), atol=1e-4)
    out = _run(dev, cand, sc, tau, 5, 30)
    _check(cand, sc, tau, g, 30, out, "logp k=30")
    print("largest logp error / tolerance: %.3f (%s)" % (WORST["ratio"], WORST["where"]))


# ---------------------------------------------------------------- 4. grid-stride trips
def _grid_cap():
    """slate_sample.hip, arx_slate_sample: one workgroup per row, `cap = cu_count() * 8` workgroups at most."""
    from arx import ops
    return ops.device_info()["cu_count"] * 8


def test_rows_past_the_grid_cap_take_further_trips(dev):
    cap = _grid_cap()
    C, k, V = 8, 3, 64
    B = cap * 2 + 5
    rng = np.random.default_rng(23)
    cand = rng.integers(-1, V, size=(B, C)).astype(np.int32)
    table = rng.standard_normal((B, V)).astype(np.float32)
    sc = np.where(cand >= 0, np.take_along_axis(table, np.maximum(cand, 0), 1), np.float32(-np.inf)).astype(np.float32)
    tau = rng.uniform(0.05, 3.0, B).astype(np.float32)
    tau[::7] = 0
    cand[5] = -1
    sc[5] = -np.inf
    out = _run(dev, cand, sc, tau, 9, k)
    _check(cand, sc, tau, _slot_noise(_noise(dev, B, V, 9), cand), k, out, "grid-stride")
    assert (out[0][5] == -1).all() and (out[0][cap:2 * cap] >= 0).any() and (out[0][2 * cap:] >= 0).any()


# ---------------------------------------------------------------- 5. the law
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_law_of_the_draws_against_the_reported_propensities(dev, seed):
    from test_slate_sample_cpu import LAW_BOUND, LAW_IDS, LAW_ROWS, LAW_SCORES, LAW_TAU
    cand = np.tile(np.array(LAW_IDS, dtype=np.int32), (LAW_ROWS, 1))
    sc = np.tile(np.array(LAW_SCORES, dtype=np.float32), (LAW_ROWS, 1))
    tau = np.full(LAW_ROWS, LAW_TAU, dtype=np.float32)
    ids, vals, pos, lp = _run(dev, cand, sc, tau, seed, 2)
    assert (pos >= 0).all() and np.isfinite(lp).all()
    exact = SS.exact_pairs(LAW_IDS, LAW_SCORES, float(np.float32(LAW_TAU)))
    chi2, cells, small = SS.pair_chi2(ids, lp.astype(np.float64), LAW_IDS, exact)
    print("seed %d: chi2 = %.2f over %d cells, smallest expected %.2f" % (seed, chi2, cells, small))
    assert cells == 30 and chi2 < LAW_BOUND
    # the rows that drew the same pair report the same propensity
    want = SS.logprob(cand, sc, tau, pos)
    tol = SS.tolerance(cand, sc, tau, want, len(LAW_IDS))
    assert (np.abs(lp - want) <= tol).all()
    for a in set(map(tuple, ids.tolist())):
        hit = (ids[:, 0] == a[0]) & (ids[:, 1] == a[1])
        assert (np.abs(lp[hit] - lp[hit][0]) <= tol[hit]).all()


# ---------------------------------------------------------------- 6. the models
def _hmf(B=16, top_n=40, d=32):
    from arx.hmf.hmf_model import LatentProductModel
    from arx.utils.synthetic import SyntheticHMF
    syn = SyntheticHMF(seed=4, n_users=200, n_items=400, logit_size=300)
    params = syn.glorot_params(d, seed=5, scale=0.5)
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind
    model = LatentProductModel(syn.n_users, syn.n_items, d, 1, B, 0.5, 1.0, syn.u_attr, syn.i_attr, i2l, l2i,
                               loss_function='ce', params=params, top_N_items=top_n)
    return syn, model


def _skipgram(B=16, top_n=40, d=32):
    from arx.utils.synthetic import SyntheticHMF
    from arx.word2vec import skipgram_model
    syn = SyntheticHMF(seed=21, n_users=200, n_items=400, logit_size=300)
    syn.u_attr.set_model_size(d)
    syn.i_attr.set_model_size(d)
    params = syn.glorot_params(d, seed=22, item_output=True, scale=0.5)
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind
    model = skipgram_model.Model(syn.n_users, syn.n_items, d, B, 0.5, 1.0, syn.u_attr, syn.i_attr, i2l, l2i,
                                 n_input_items=1, loss_function='ce', use_sep_item=True, top_N_items=top_n,
                                 params=params)
    return syn, model


def _model_rounds(dev, model, recommend, score, batches, V):
    import torch
    rng = np.random.default_rng(41)
    B, C, k = model.batch_size, 40, 7
    slates = []
    for _ in batches:
        c = np.stack([rng.permutation(V)[:C] for _ in range(B)]).astype(np.int64)
        c[:, 30:34] = c[:, :4]                                       # repeated ids
        c[:, 36:] = -1
        c[1, 3:] = -1                                                # fewer than k
        slates.append(c)
    plain0 = score(batches[0], slates[0], k)
    div0 = score(batches[0], slates[0], k, diversify=0.6)
    n_plans = n_nodes = None
    calls = [(0.5, 3), (np.linspace(0.0, 2.0, B).astype(np.float32), 2 ** 40 + 1), (0.0, 3), (0.5, 3)]
    outs = []
    for n, (t, seed) in enumerate(calls):
        batch, cand = batches[n % len(batches)], slates[n % len(batches)]
        sc = score(batch, cand, None).cpu().numpy()
        ids, vals, lp = score(batch, cand, k, sample_temperature=t, sample_seed=seed, return_logprob=True)
        assert all(isinstance(x, torch.Tensor) and x.is_cuda and tuple(x.shape) == (B, k) for x in (ids, vals, lp))
        assert ids.dtype == torch.int32 and vals.dtype == torch.float32 and lp.dtype == torch.float32
        node = model._plans[('score_items', C, k, 'sample')].fetch[0]
        tau = np.broadcast_to(np.asarray(t, dtype=np.float32), (B,))
        out = (ids.cpu().numpy(), vals.cpu().numpy(), node.pos.cpu().numpy(), lp.cpu().numpy())
        _check(cand.astype(np.int32), sc, tau, _slot_noise(_noise(dev, B, V, seed), cand.astype(np.int32)), k, out,
               "model call %d" % n)
        outs.append(out)
        if n == 0:
            n_plans, n_nodes = len(model._plans), len(model.rt.nodes)
    # one plan served every temperature and seed; the same seed gives the same result; tau = 0 is the plain order
    assert len(model._plans) == n_plans and len(model.rt.nodes) == n_nodes
    for a, b in zip(outs[0], outs[3]):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    two = score(batches[0], slates[0], k, sample_temperature=0.5, sample_seed=3)
    assert len(two) == 2
    np.testing.assert_array_equal(two[0].cpu().numpy(), outs[0][0])
    sc2 = score(batches[2], slates[2], None).cpu().numpy()
    dedup = slates[2].copy()
    dedup[:, 30:34] = -1                                             # (the later copies do not compete)
    sc2[:, 30:34] = -np.inf
    wi, wv = SO.order(sc2, dedup, k)
    np.testing.assert_array_equal(outs[2][0], wi)
    assert (outs[2][3] == 0).all()
    # sample_seed=None counts up: the draws of seeds n and n + 1
    att = model.att_emb
    n0 = att.sample_draws
    a = score(batches[0], slates[0], k, sample_temperature=0.8)
    b = score(batches[0], slates[0], k, sample_temperature=0.8, return_logprob=True)
    assert att.sample_draws == n0 + 2 and not np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy())
    for seed, got in ((n0, a), (n0 + 1, b)):
        want = score(batches[0], slates[0], k, sample_temperature=0.8, sample_seed=seed)
        np.testing.assert_array_equal(got[0].cpu().numpy(), want[0].cpu().numpy())
    with pytest.raises(ValueError):
        score(batches[0], slates[0], k, sample_temperature=-1.0)
    with pytest.raises(ValueError):
        score(batches[0], slates[0], k, sample_temperature=0.5, diversify=0.5)
    assert att.sample_draws == n0 + 2 and len(model._plans) == n_plans
    # the plain and the diversified call are what they were
    for before, kw in ((plain0, {}), (div0, dict(diversify=0.6))):
        after = score(batches[0], slates[0], k, **kw)
        for x, y in zip(before, after):
            np.testing.assert_array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))
    # the composition: recommend's best C as the slate (its -1 tails are empty slots already)
    rec = np.asarray(recommend(batches[1]))
    assert rec.shape == (B, C)
    ids, vals, lp = score(batches[1], rec, k, sample_temperature=0.5, sample_seed=8, return_logprob=True)
    ids, lp = ids.cpu().numpy(), lp.cpu().numpy()
    for r in range(B):
        real = ids[r] >= 0
        assert np.isin(ids[r][real], rec[r]).all() and len(set(ids[r][real].tolist())) == real.sum()
        assert real[:real.sum()].all()                               # no -1 before a real id
        assert (lp[r][real] <= 1e-5).all() and (lp[r][~real] == 0).all()


def test_hmf_score_items_sample(dev):
    syn, model = _hmf()
    B = model.batch_size
    rng = np.random.default_rng(5)
    batches = [rng.choice(syn.n_users, B, replace=False).astype(np.int32) for _ in range(3)]
    _model_rounds(dev, model, lambda u: model.step(None, list(u), None, recommend=True),
                  lambda u, c, kk, **kw: model.score_items(list(u), c, k=kk, **kw), batches, model.logit_size)


def test_linear_seq_score_items_sample(dev):
    syn, model = _skipgram()
    B = model.batch_size
    rng = np.random.default_rng(9)
    batches = [(rng.choice(syn.n_users, B, replace=False).astype(np.int32), syn.sample_batch(B, rng)[1][None, :])
               for _ in range(3)]
    _model_rounds(dev, model, lambda b: model.step(None, list(b[0]), b[1].tolist(), recommend=True),
                  lambda b, c, kk, **kw: model.score_items(list(b[0]), b[1].tolist(), c, k=kk, **kw), batches,
                  model.logit_size)


def test_largest_logp_error_seen_stays_under_its_tolerance():
    """(runs last: reports the figure DESIGN.md quotes)"""
    print("largest logp error / tolerance over this file: %.3f (%s)" % (WORST["ratio"], WORST["where"]))
    assert WORST["ratio"] <= 1.0
