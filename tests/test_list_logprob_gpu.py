"""list_logprob on the GPU (include/arx_list_logp.h): the log-probability of a GIVEN ordered list under the sampling
policy, with the reason code of every entry the policy could not draw.

The float64 oracle (tests/list_logprob_oracle.py) is evaluated on L -- the project's own scorer GEMM of the same
operands, materialised (the rig of tests/test_recommend_exclude_gpu.py).  The tolerance is that of the draw's
propensities, unchanged (recommend_logprob_oracle.tolerance), on the drawable entries; the codes, the zeros and the
-inf entries are exact.  Every test prints its largest |error| / tolerance.
"""
import itertools

import numpy as np
import pytest

import list_logprob_oracle as LL
import recommend_logprob_oracle as RL
import tags_oracle as T
from test_recommend_exclude_gpu import _Rig, _const, _hmf, _row_cols, _skipgram
from test_recommend_logprob_gpu import _bias_rig, _filters, _nodes
from test_recommend_sample_gpu import _dev_sample, _dev_tags, _taus

pytestmark = pytest.mark.gpu


def _pos_taus(rng, B):
    tau = _taus(rng, B)
    tau[tau == 0] = 0.5                       # (a deterministic row has no propensities: refused on the host)
    return tau


def _i32(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).to(dev)


def _outs(dev, B, k):
    import torch
    return (torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev),
            torch.empty((B, k), dtype=torch.int32, device=dev))


def _check(name, L, lists, tau, filt, glp, gv, gwhy):
    """codes exact; logp within RL.tolerance of the oracle at the drawable entries, -inf at the codes 2-6, 0 at -1;
    values the bits of L at the drawable entries, -inf elsewhere.  -> (oracle logp, tolerance)"""
    exp, codes, tol = LL.logp(L, lists, tau, **filt)
    np.testing.assert_array_equal(gwhy, codes, err_msg=name)
    ok = codes == LL.OK
    assert not np.isnan(glp).any(), name
    assert np.isneginf(glp[codes >= LL.RANGE]).all() and (glp[codes == LL.EMPTY] == 0).all(), name
    assert np.isfinite(glp[ok]).all() and (tol[ok] > 0).all(), name
    w = float((np.abs(glp[ok].astype(np.float64) - exp[ok]) / tol[ok]).max()) if ok.any() else 0.0
    print("%s: largest |error| / tolerance %.3f (%d drawable of %d)" % (name, w, ok.sum(), ok.size))
    assert w <= 1, (name, w)
    sc = np.take_along_axis(L, np.clip(lists, 0, L.shape[1] - 1), 1)
    np.testing.assert_array_equal(gv[ok].view(np.int32), sc[ok].view(np.int32), err_msg=name)
    assert np.isneginf(gv[~ok]).all(), name
    return exp, tol


# ---------------------------------------------------------------- 1. prepare alone
@pytest.mark.parametrize("k", [1, 65, 1024])
def test_prepare_codes_clean_and_sorted_picks(dev, k):
    import torch
    from arx import ops
    B, V = 130, 593
    rng = np.random.default_rng(k)
    rig = _Rig(B, V, 32, seed=k)
    tags = T.random_tags(rng, V)
    want_any = np.where(np.arange(B) % 4 % 2 == 0, np.uint32(1), np.uint32(0)).astype(np.uint32)      # bit 0: p = 1/2
    want_all = np.where(np.arange(B) % 4 >= 1, np.uint32(2), np.uint32(0)).astype(np.uint32)          # bit 1: p = 1/4
    want_any[np.arange(B) % 4 == 3] = 0
    want_all[np.arange(B) % 4 == 3] = 0       # rows % 4: any alone, all alone, both, none
    tag_ok = T.eligible(tags, want_any, want_all)
    ex_lists = [np.unique(rng.integers(0, V, 40)) for _ in range(B)]
    ex_lists[5] = np.zeros(0, dtype=np.int64)                         # an empty exclusion list
    keys = np.arange(B, dtype=np.int32)
    keys[7] = -1                                                      # a negative key: nothing excluded
    ex_rows = rig.exclusions(keys, ex_lists)
    lists = np.full((B, k), -1, dtype=np.int64)
    for r in range(B):
        free = np.setdiff1d(np.nonzero(tag_ok[r])[0], ex_rows[r])     # the row's eligible columns
        bad_tag = np.setdiff1d(np.nonzero(~tag_ok[r])[0], ex_rows[r])
        sp = [-1, -7, V, 2 ** 31 - 1, int(free[0]), int(free[-1])]
        if len(ex_rows[r]):
            e0, e1 = int(ex_rows[r][0]), int(ex_rows[r][-1])
            sp += [e0, e1, e1, e1]                                    # the last listed column three times: all EXCLUDED
        if len(bad_tag):
            sp += [int(bad_tag[0]), int(bad_tag[-1])]
        sp += [int(free[1])] * 3                                      # three times and eligible: OK, REPEAT, REPEAT
        if k == 1:
            lists[r, 0] = sp[r % len(sp)]
            continue
        body = sp + rng.integers(0, V, max(0, k - 3 - len(sp))).tolist()
        body = [body[i] for i in rng.permutation(len(body))][:k - 3]
        row = [-1] + body[:len(body) // 2] + [-1] + body[len(body) // 2:] + [-1]      # -1 at the ends and in the middle
        lists[r, :len(row)] = row
    if k > 1:
        lists[9] = int(np.setdiff1d(np.nonzero(tag_ok[9])[0], ex_rows[9])[2])         # k copies of one column
    filt = dict(tags=tags, want_any=want_any, want_all=want_all, ex_lists=ex_rows)
    codes = LL.why(rig.logits, lists, **filt)
    assert set(np.unique(codes)) == set(range(6 if k > 1 else 5))     # every code the kernel can give
    if k > 1:
        assert codes[9].tolist() == [LL.OK] + [LL.REPEAT] * (k - 1)
    d_lists = _i32(dev, lists)
    clean, why, pc, ps, pc2, ps2 = (torch.full((B, k), -77, dtype=torch.int32, device=dev) for _ in range(6))
    ops.list_logp_prepare(d_lists, V, rig.ex, _dev_tags(dev, tags, want_any, want_all), clean, why, pc, ps)
    np.testing.assert_array_equal(why.cpu().numpy(), codes)
    np.testing.assert_array_equal(clean.cpu().numpy(), LL.clean(lists, codes))
    ops.sample_logp_sort(clean, pc2, ps2)
    np.testing.assert_array_equal(pc.cpu().numpy(), pc2.cpu().numpy())
    np.testing.assert_array_equal(ps.cpu().numpy(), ps2.cpu().numpy())
    # no filters at all: only EMPTY, RANGE and REPEAT are left
    ops.list_logp_prepare(d_lists, V, None, None, clean, why, pc, ps)
    np.testing.assert_array_equal(why.cpu().numpy(), LL.why(rig.logits, lists))


# ---------------------------------------------------------------- 2. bit identity with the draw
def _dense_node(rig, dev, k, mode, targs, sargs):
    import torch
    from arx.hmf import hmf_model as hm
    logits = _const(rig.rt, torch.from_numpy(rig.logits).to(dev))
    return hm.TopK(rig.rt, logits, k, exclude=(lambda: rig.ex) if 'ex' in mode else None,
                   tags=(lambda: targs) if targs is not None else None, sample=lambda: sargs, logp=True)


def _stream_list_logp(node, rig, lists_dev, mode, targs, sargs, outs):
    logp, values, why = outs
    node.list_logp(rig.latent.value, rig.pool.value, rig.pool.bias_value, rig.rt.ws, lists_dev,
                   rig.ex if 'ex' in mode else None, targs, sargs, logp, values, why)
    return logp.cpu().numpy(), values.cpu().numpy(), why.cpu().numpy()


def _same_bits(name, gi, draw_lp, draw_v, glp, gv, gwhy):
    np.testing.assert_array_equal(glp.view(np.int32), draw_lp.view(np.int32), err_msg=name)
    np.testing.assert_array_equal(gv.view(np.int32), draw_v.view(np.int32), err_msg=name)
    np.testing.assert_array_equal(gwhy, np.where(gi >= 0, LL.OK, LL.EMPTY), err_msg=name)


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("k", [1, 30])
@pytest.mark.parametrize("mode", ["plain", "ex", "tags", "ex_tags"])
def test_own_draws_come_back_bit_identical(dev, d, k, mode):
    """What makes the importance weight of a policy against itself exactly 1: the drawn ids fed back through list_logp
    on the same path give the draw's logp and values bit for bit."""
    B, V = 130, 256 + 5 * 64 + 17
    rig = _Rig(B, V, d, seed=5 * d + k)
    rng = np.random.default_rng(d + k)
    tau = _pos_taus(rng, B)
    filt, targs = _filters(rig, rng, B, V, mode, dev)
    sargs = _dev_sample(dev, tau, 100 * d + k)
    _, node = _nodes(rig, k, mode, targs, sargs)
    assert node.fused
    outs = _outs(dev, B, k)
    for fused in (True, False):
        node.fused = fused
        assert node.mass_streams(rig.latent.value, rig.pool.value) == fused
        node.forward(False)
        gi = node.indices.cpu().numpy()
        got = _stream_list_logp(node, rig, node.indices, mode, targs, sargs, outs)
        _same_bits('d=%d k=%d %s fused=%s' % (d, k, mode, fused), gi, node.logp.cpu().numpy(), node.value.cpu().numpy(),
                   *got)
    if d == 64:
        dense = _dense_node(rig, dev, k, mode, targs, sargs)
        dense.forward(False)
        logp, values, why = outs
        dense.list_logp(dense.indices, sargs, logp, values, why)
        _same_bits('dense k=%d %s' % (k, mode), dense.indices.cpu().numpy(), dense.logp.cpu().numpy(),
                   dense.value.cpu().numpy(), logp.cpu().numpy(), values.cpu().numpy(), why.cpu().numpy())


# ---------------------------------------------------------------- 3. foreign lists against the oracle
def _foreign_lists(rng, logits, k):
    """per row a random permutation of: columns of the row's top 50, 10 % random columns, 5 % repeats of entries of
    the list, two -1 holes"""
    B, V = logits.shape
    top = np.argsort(-logits, axis=1)[:, :50]
    n_rand, n_rep, n_hole = max(1, k // 10), max(1, k // 20), 2
    out = np.empty((B, k), dtype=np.int64)
    for r in range(B):
        own = rng.permutation(top[r])[:k - n_rand - n_rep - n_hole]
        row = np.concatenate([own, rng.integers(0, V, n_rand)])
        row = np.concatenate([row, rng.choice(row, n_rep), np.full(n_hole, -1)])
        out[r] = rng.permutation(row)
        out[r, [0, k - 1]] = np.where(out[r, [0, k - 1]] < 0, top[r, 0], out[r, [0, k - 1]])   # the holes: in the middle
    return out


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("mode", ["plain", "ex", "tags", "ex_tags"])
def test_foreign_lists_against_the_oracle(dev, d, mode):
    B, V, k = 130, 256 + 5 * 64 + 17, 40
    rig = _Rig(B, V, d, seed=7 * d)
    rng = np.random.default_rng(d)
    tau = _pos_taus(rng, B)
    filt, targs = _filters(rig, rng, B, V, mode, dev)                 # ('ex': each row's own top 50 are excluded)
    if 'ex' in mode:                                                  # ... half of them, so that some entries stay
        filt['ex_lists'] = rig.exclusions(np.arange(B, dtype=np.int32), [l[::2] for l in filt['ex_lists']])
    sargs = _dev_sample(dev, tau, 1)
    lists = _foreign_lists(rng, rig.logits, k)
    codes = LL.why(rig.logits, lists, **filt)
    assert (codes == LL.REPEAT).any() and (codes == LL.EMPTY).sum() >= B and (codes == LL.OK).sum() > B
    assert ('ex' not in mode or (codes == LL.EXCLUDED).any()) and ('tags' not in mode or (codes == LL.TAGS).any())
    _, node = _nodes(rig, 8, mode, targs, sargs)                      # (the node's own k plays no part)
    d_lists = _i32(dev, lists)
    outs = _outs(dev, B, k)
    whys = []
    for fused in (True, False):
        node.fused = fused
        glp, gv, gwhy = _stream_list_logp(node, rig, d_lists, mode, targs, sargs, outs)
        _check('d=%d %s fused=%s' % (d, mode, fused), rig.logits, lists, tau, filt, glp, gv, gwhy)
        whys.append(gwhy)
    dense = _dense_node(rig, dev, 8, mode, targs, sargs)
    logp, values, why = outs
    dense.list_logp(d_lists, sargs, logp, values, why)
    _check('d=%d %s dense' % (d, mode), rig.logits, lists, tau, filt, logp.cpu().numpy(), values.cpu().numpy(),
           why.cpu().numpy())
    np.testing.assert_array_equal(whys[0], whys[1])                   # the two mass forms agree on what is impossible
    np.testing.assert_array_equal(whys[0], why.cpu().numpy())


# ---------------------------------------------------------------- 4. the probabilities of all lists sum to one
@pytest.mark.parametrize("tau0", [0.3, 1.0, 4.0])
def test_probabilities_of_all_lists_sum_to_one(dev, tau0):
    import torch
    from arx import ops
    from arx.hmf import hmf_model as hm
    B, d, k = 60, 64, 3
    V = 64 * 40 + 17
    rig = _Rig(B, V, d, seed=11)
    lat = rig.latent.value[:1].repeat(B, 1).contiguous()              # one user, 60 times
    rig.latent = _const(rig.rt, lat)
    buf = torch.empty((B, V), dtype=torch.float32, device=dev)
    ops.gemm(lat, rig.pool.value, buf, rig.rt.ws, transB=True, col_bias=rig.pool.bias_value)
    L = buf.cpu().numpy()
    assert (L == L[0]).all()
    keep = [0, 63, 64, 1300, V - 1]
    ex_rows = rig.exclusions(np.zeros(B, dtype=np.int32), [np.setdiff1d(np.arange(V), keep)])
    lists = np.array(list(itertools.permutations(keep, k)), dtype=np.int64)
    assert lists.shape == (B, k)
    tau = np.full(B, tau0, dtype=np.float32)
    sargs = _dev_sample(dev, tau, 0)
    node = hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, chunk=256, exclude=lambda: rig.ex, sample=lambda: sargs)
    assert node.fused and node.mass_streams(lat, rig.pool.value)
    d_lists = _i32(dev, lists)
    outs = _outs(dev, B, k)
    filt = dict(ex_lists=ex_rows)
    for fused in (True, False):
        node.fused = fused
        glp, gv, gwhy = _stream_list_logp(node, rig, d_lists, 'ex', None, sargs, outs)
        exp, tol = _check('tau=%g fused=%s' % (tau0, fused), L, lists, tau, filt, glp, gv, gwhy)
        assert (gwhy == LL.OK).all()
        total = float(np.exp(glp.astype(np.float64).sum(1)).sum())
        bound = float((np.exp(exp.sum(1)) * tol.sum(1)).sum())
        print("tau=%g fused=%s: |sum - 1| = %.3g, bound %.3g" % (tau0, fused, abs(total - 1), bound))
        assert abs(total - 1) <= bound


# ---------------------------------------------------------------- 5. cursor edges on hand-made lists
def _scan_list_logp(scan, rig, dev, lists, tau, ex, streaming):
    B, k = lists.shape
    sargs = _dev_sample(dev, tau, 0)
    logp, values, why = _outs(dev, B, k)
    assert scan.fused and scan.mass_streams(rig.lat, rig.pl)

    def run():
        scan.list_logp(rig.lat, rig.pl, rig.bias, rig.rt.ws, _i32(dev, lists), ex, None, sargs, logp, values, why)
    if streaming:
        run()
    else:
        with scan.chunked():
            run()
    return logp.cpu().numpy(), values.cpu().numpy(), why.cpu().numpy()


def test_cursor_edges_with_foreign_entries(dev):
    from arx import ops
    from arx.topk import TopKScan
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
    spots = sorted(set(spots))                                        # (two edges may name one column)
    assert len(spots) >= 11
    lists = np.full((B, k), -1, dtype=np.int64)
    ex_lists = []
    for r in range(B):
        mine = rng.permutation(spots)
        gone = mine[5:11]                                             # six excluded spots, one of them in the list
        row = np.concatenate([mine[:5], gone[:1], mine[:1], [V + int(rng.integers(0, 3)) * 1000]])
        lists[r] = rng.permutation(row)                               # five drawable, excluded, repeat, past V
        ex_lists.append(np.setdiff1d(np.concatenate([gone, rng.integers(0, V, 20)]), mine[:5]))
    # row 1: REST is empty (everything but its drawable entries is excluded); row 2: nothing drawable at all
    drawable1 = [c for c in lists[1] if c < V and c not in set(ex_lists[1].tolist())]
    ex_lists[1] = np.setdiff1d(np.arange(V), drawable1)
    lists[2] = [int(ex_lists[2][0]), V, -7, int(ex_lists[2][-1]), 2 ** 31 - 1, int(ex_lists[2][0]), V + 5, -2]
    rig = _bias_rig(B, V, d, bias)
    ex_rows = rig.exclusions(np.arange(B, dtype=np.int32), ex_lists)
    tau = _pos_taus(rng, B)
    L = np.broadcast_to(bias, (B, V)).copy()
    scan = TopKScan(B, V, d, k, dev, chunk=tpb * 64 + 64)
    for streaming in (True, False):
        glp, gv, gwhy = _scan_list_logp(scan, rig, dev, lists, tau, rig.ex, streaming)
        _check('edges streaming=%s' % streaming, L, lists, tau, dict(ex_lists=ex_rows), glp, gv, gwhy)
        for c in (LL.OK, LL.RANGE, LL.EXCLUDED, LL.REPEAT):
            assert (gwhy[3:] == c).sum() >= B - 3, c
        last = np.nonzero(gwhy[1] == LL.OK)[0][-1]
        assert glp[1, last] == 0 and (gwhy[1] == LL.OK).sum() == 5
        assert (gwhy[2] >= LL.RANGE).all() and np.isneginf(glp[2]).all() and np.isneginf(gv[2]).all()
    # -inf biases only: every in-range entry is NOSCORE (a second copy of one REPEAT), -1 stays EMPTY
    rig3 = _bias_rig(B, V, d, np.full(V, -np.inf, dtype=np.float32))
    lists3 = np.stack([rng.permutation(spots)[:k] for _ in range(B)])
    lists3[:, 3] = -1
    lists3[:, 5] = V
    lists3[::2, 6] = lists3[::2, 0]
    L3 = np.full((B, V), -np.inf, dtype=np.float32)
    for streaming in (True, False):
        glp, gv, gwhy = _scan_list_logp(scan, rig3, dev, lists3, tau, None, streaming)
        _check('no scores streaming=%s' % streaming, L3, lists3, tau, {}, glp, gv, gwhy)
        assert (gwhy[:, [0, 1, 2, 4, 7]] == LL.NOSCORE).all() and (gwhy[::2, 6] == LL.REPEAT).all()
        assert (gwhy[:, 3] == LL.EMPTY).all() and (gwhy[:, 5] == LL.RANGE).all()


# ---------------------------------------------------------------- 6. numerics: a target far from the logging policy
@pytest.mark.parametrize("tau0", [0.05, 20.0])
def test_numerics_of_unlikely_lists(dev, tau0):
    B, V, d, k = 130, 256 + 5 * 64 + 17, 64, 30
    rig = _Rig(B, V, d, seed=13)
    lists = np.argsort(rig.logits, axis=1)[:, :k].astype(np.int64)    # each row's BOTTOM 30: logp around -spread / tau
    tau = np.full(B, tau0, dtype=np.float32)
    sargs = _dev_sample(dev, tau, 0)
    _, node = _nodes(rig, 8, 'plain', None, sargs)
    outs = _outs(dev, B, k)
    for fused in (True, False):
        node.fused = fused
        glp, gv, gwhy = _stream_list_logp(node, rig, _i32(dev, lists), 'plain', None, sargs, outs)
        exp, tol = _check('tau=%g fused=%s' % (tau0, fused), rig.logits, lists, tau, {}, glp, gv, gwhy)
        assert np.isfinite(glp).all() and (gwhy == LL.OK).all()
        rows = np.abs(glp.astype(np.float64).sum(1) - exp.sum(1))
        print("tau=%g fused=%s: row sums around %.1f, largest |error| / summed tolerance %.3f"
              % (tau0, fused, exp.sum(1).mean(), (rows / tol.sum(1)).max()))
        assert (rows <= tol.sum(1)).all()


# ---------------------------------------------------------------- 7. through the models
def _model_rounds(name, model, L, syn, users, rec, llp, k):
    """rec(**kw): model.step(recommend=True, ...); llp(lists, tau, **kw): model.list_logprob(...)"""
    from arx.utils.ope import list_weights
    B = model.batch_size
    rng = np.random.default_rng(6)
    item_tags = T.random_tags(rng, syn.n_items)
    col_tags = item_tags[np.asarray(syn.logit_ind2item_ind, dtype=np.int64)]
    sets = {int(u): rng.integers(0, syn.n_items, 60).tolist() for u in users}
    want_any = np.full(B, 1, dtype=np.uint32)
    want_any[::5] = 0
    some = np.zeros((B, k), dtype=np.int64)
    with pytest.raises(ValueError, match="prepare_recommend_exclusions"):
        llp(some, 1.0, exclude_seen=True)
    with pytest.raises(ValueError, match="prepare_item_tags"):
        llp(some, 1.0, tags_any=1)
    model.prepare_recommend_exclusions(sets)
    model.prepare_item_tags(item_tags)
    rows = _row_cols(syn, sets, users)
    filt = dict(tags=col_tags, want_any=want_any, want_all=np.zeros(B, dtype=np.uint32), ex_lists=rows)
    kw = dict(exclude_seen=True, tags_any=want_any)
    # the policy against itself: the same bits, weights exactly 1
    ids, logged = rec(sample_temperature=0.7, sample_seed=3, return_logprob=True, **kw)
    assert ids.shape == (B, k)
    lp, vals, why = llp(ids, 0.7, return_values=True, return_why=True, **kw)
    assert lp.dtype == np.float32 and lp.shape == (B, k) and why.dtype == np.int32 and vals.dtype == np.float32
    np.testing.assert_array_equal(lp.view(np.int32), logged.view(np.int32), err_msg=name)
    np.testing.assert_array_equal(why, np.where(ids >= 0, LL.OK, LL.EMPTY), err_msg=name)
    assert (list_weights(lp, logged) == 1.0).all()
    only = llp(ids, 0.7, **kw)
    assert isinstance(only, np.ndarray)
    np.testing.assert_array_equal(only.view(np.int32), lp.view(np.int32))
    pair = llp(ids, 0.7, return_why=True, **kw)
    assert isinstance(pair, tuple) and len(pair) == 2 and pair[1].dtype == np.int32
    # another temperature and a permuted list, then new lists and a new temperature on the captured plan
    key = ('list_logp_ex_tags', k)
    assert key in model._plans
    n_plans = len(model._plans)
    perm = np.stack([rng.permutation(r) for r in ids]).astype(np.int64)
    tau2 = np.full(B, 1.9, dtype=np.float32)
    got = llp(perm, 1.9, return_values=True, return_why=True, **kw)
    _check(name + ' permuted', L, perm, tau2, filt, *got)
    other = rng.integers(-1, L.shape[1] + 3, (B, k)).astype(np.int64)
    tau3 = _pos_taus(rng, B)
    got = llp(_i32(model.rt.device, other), tau3, return_values=True, return_why=True, **kw)   # a device tensor
    _check(name + ' new lists', L, other, tau3, filt, *got)
    assert len(model._plans) == n_plans and model._plans[key].graph is not None
    # another k is another plan; a list of python ints works
    got = llp(other[:, :3].tolist(), tau3, return_values=True, return_why=True, **kw)
    _check(name + ' k=3', L, other[:, :3], tau3, filt, *got)
    assert ('list_logp_ex_tags', 3) in model._plans
    # new exclusion lists drop the plans that read the old ones: the first entry of row 0 is now excluded
    l2i = syn.logit_ind2item_ind
    first = int(ids[0, 0])
    assert first >= 0
    sets[int(users[0])] = sets[int(users[0])] + [int(l2i[first])]
    model.prepare_recommend_exclusions(sets)
    assert key not in model._plans and ('list_logp_ex_tags', 3) not in model._plans
    lp2, why2 = llp(ids, 0.7, return_why=True, **kw)
    assert why2[0, 0] == LL.EXCLUDED and np.isneginf(lp2[0, 0]) and (why2[1:] == why[1:]).all()
    np.testing.assert_array_equal(lp2[1:].view(np.int32), logged[1:].view(np.int32))
    assert list_weights(lp2, logged)[0] == 0
    # the refusals
    for bad in (np.zeros((B, 0), dtype=np.int64), np.zeros((B, 1025), dtype=np.int64), np.zeros((B + 1, k), np.int64)):
        with pytest.raises(ValueError):
            llp(bad, 1.0)
    for bad in (0, -1.0, float('nan'), float('inf'), [1.0] * (B - 1), None):
        with pytest.raises(ValueError):
            llp(some, bad)
    zero = np.ones(B)
    zero[4] = 0
    with pytest.raises(ValueError, match="row 4 "):
        llp(some, zero)


def test_hmf_list_logprob_dense_and_streamed(dev, monkeypatch):
    from arx.hmf import hmf_model as hm
    syn, mat = _hmf(4)
    monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '0')
    _, st = _hmf(4)
    assert isinstance(st.topk, hm.StreamTopK) and isinstance(mat.topk, hm.TopK)
    st.topk.chunk = 1536
    st.topk._buf = st.topk._buf[:, :1536].contiguous()
    B, k = mat.batch_size, mat.topk.k
    users = np.random.default_rng(6).choice(syn.n_users, B, replace=False).astype(np.int32)
    mat.step(None, list(users), None, recommend=True)
    L = mat.topk.inputs[0].value.cpu().numpy()
    for m in (mat, st):
        _model_rounds('hmf %s' % type(m.topk).__name__, m, L, syn, users,
                      lambda m=m, **kw: m.step(None, list(users), None, recommend=True, **kw),
                      lambda lists, tau, m=m, **kw: m.list_logprob(list(users), lists, tau, **kw), k)
    assert st.topk.fused and st.topk.mass_streams(st.topk.inputs[0].value, st.topk.inputs[1].value)


def test_linear_seq_list_logprob_and_output_feat_refusal(dev):
    syn, model = _skipgram()
    B, d = model.batch_size, 32
    rng = np.random.default_rng(9)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    ctx = syn.sample_batch(B, rng)[1][None, :]
    model.step(None, list(users), ctx.tolist(), recommend=True)
    L = model.topk.inputs[0].value.cpu().numpy()
    _model_rounds('linear_seq', model, L, syn, users,
                  lambda **kw: model.step(None, list(users), ctx.tolist(), recommend=True, **kw),
                  lambda lists, tau, **kw: model.list_logprob(list(users), ctx.tolist(), lists, tau, **kw), model.topk.k)
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
        pooled.list_logprob(list(range(16)), [[0] * 16], np.zeros((16, 3), dtype=np.int64), 1.0)


# ---------------------------------------------------------------- 8. the whole chain at the cap, k = 1024
def test_whole_chain_at_k_1024(dev):
    """prepare, both mass forms and the dense one, finish and stamp on lists of 1024 entries: about 900 distinct
    columns per row, the rest repeats, -1 holes and ids past V; some of the columns excluded."""
    B, d, k = 130, 64, 1024
    V = 64 * 40 + 17
    rig = _Rig(B, V, d, seed=17)
    rng = np.random.default_rng(17)
    tau = _pos_taus(rng, B)
    filt, targs = _filters(rig, rng, B, V, 'ex', dev)
    sargs = _dev_sample(dev, tau, 1)
    lists = np.empty((B, k), dtype=np.int64)
    for r in range(B):
        own = rng.permutation(V)[:900]
        row = np.concatenate([own, rng.choice(own, 80), np.full(24, -1), V + rng.integers(0, 5, 20)])
        lists[r] = rng.permutation(row)
    codes = LL.why(rig.logits, lists, **filt)
    assert set(np.unique(codes)) == {LL.OK, LL.EMPTY, LL.RANGE, LL.EXCLUDED, LL.REPEAT}
    _, node = _nodes(rig, 8, 'ex', targs, sargs, chunk=1024)
    d_lists = _i32(dev, lists)
    outs = _outs(dev, B, k)
    for fused in (True, False):
        node.fused = fused
        assert node.mass_streams(rig.latent.value, rig.pool.value) == fused
        glp, gv, gwhy = _stream_list_logp(node, rig, d_lists, 'ex', targs, sargs, outs)
        _check('k=1024 fused=%s' % fused, rig.logits, lists, tau, filt, glp, gv, gwhy)
    dense = _dense_node(rig, dev, 8, 'ex', targs, sargs)
    logp, values, why = outs
    dense.list_logp(d_lists, sargs, logp, values, why)
    _check('k=1024 dense', rig.logits, lists, tau, filt, logp.cpu().numpy(), values.cpu().numpy(), why.cpu().numpy())


# ---------------------------------------------------------------- 9. a fresh model, and the cap on the kept plans
def test_fresh_model_and_the_oldest_plan_goes_first(dev):
    """list_logprob as the FIRST call of a model (no sampled step before it: the temperature placeholder is made and
    fed here, the seed words are never read), then nine values of k: eight plans stay, the oldest is dropped with
    its nodes, and asking for it again rebuilds it."""
    from arx.topk import MAX_LIST_PLANS
    syn, model = _hmf(4)
    _, twin = _hmf(4)
    B = model.batch_size
    rng = np.random.default_rng(2)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    twin.step(None, list(users), None, recommend=True)
    L = twin.topk.inputs[0].value.cpu().numpy()
    V = L.shape[1]
    assert getattr(model.att_emb, '_sample_tau', None) is None and not model._plans
    tau = _pos_taus(rng, B)

    def call(k):
        lists = rng.integers(-1, V + 2, (B, k)).astype(np.int64)
        got = model.list_logprob(list(users), lists, tau, return_values=True, return_why=True)
        _check('fresh model k=%d' % k, L, lists, tau, {}, *got)
    call(12)
    assert list(model._plans) == [('list_logp', 12)]
    n_nodes = None
    for k in range(1, MAX_LIST_PLANS + 1):
        call(k)
        if k == MAX_LIST_PLANS - 1:
            n_nodes = len(model.rt.nodes)                              # eight plans: the most a model keeps
    keys = [q for q in model._plans if isinstance(q, tuple) and q[0].startswith('list_logp')]
    assert keys == [('list_logp', k) for k in range(1, MAX_LIST_PLANS + 1)]           # k = 12, the oldest, is gone
    assert len(model.rt.nodes) == n_nodes                             # ... with its placeholder and its node
    call(12)
    keys = [q for q in model._plans if isinstance(q, tuple) and q[0].startswith('list_logp')]
    assert len(keys) == MAX_LIST_PLANS and ('list_logp', 1) not in keys and keys[-1] == ('list_logp', 12)
    np.testing.assert_array_equal(model.step(None, list(users), None, recommend=True),
                                  twin.step(None, list(users), None, recommend=True))
