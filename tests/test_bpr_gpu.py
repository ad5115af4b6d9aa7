"""The pairwise losses 'bpr' / 'bpr-hinge' on the device: the fused pair kernel against fp64 numpy, whole steps of
LatentProductModel against a reference composed from the oracle's own pieces (two target scores per row), the
rank-select negative draw against its numpy statement, and the model drawing its negatives inside the captured step."""
import numpy as np
import pytest

from oracle import ref_graph as rg
from test_bpr_cpu import rank_select
from test_hmf_gpu import ATOL, CFG_HET, CFG_ID, CFG_MIX, RTOL, _compare_state

pytestmark = pytest.mark.gpu

KINDS = ('bpr', 'bpr-hinge')


# ------------------------------------------------------------------ 1. kernel parity
def _pair_case(B, d, seed):
    """Operands of one kernel case; entries ~ N(0, 1) / (2 d^(1/4)): the scores stay O(1) at every d."""
    rng = np.random.default_rng(seed)
    s = 0.5 / d ** 0.25
    U, P, N = (rng.standard_normal((B, d)).astype(np.float32) * np.float32(s) for _ in range(3))
    pb, nb = (rng.standard_normal(B).astype(np.float32) * np.float32(0.1) for _ in range(2))
    rw = rng.uniform(0.5, 1.5, B).astype(np.float32)
    dU0 = rng.standard_normal((B, d)).astype(np.float32)
    return U, P, pb, N, nb, rw, dU0


def _pair_ref(kind, U, P, pb, N, nb, void, rw, gscale, dU0):
    U, P, pb, N, nb, rw, dU0 = (np.asarray(a, dtype=np.float64) for a in (U, P, pb, N, nb, rw, dU0))
    ps = (U * P).sum(1) + pb
    ns = (U * N).sum(1) + nb
    x = ns - ps
    if kind == 'bpr':
        loss, g = np.logaddexp(0.0, x), 1.0 / (1.0 + np.exp(-x))
    else:
        loss, g = np.maximum(1.0 + x, 0.0), (1.0 + x > 0).astype(np.float64)
    live = ~void
    c = gscale * rw * g * live
    return dict(ps=ps, ns=ns, x=x, loss=loss * live, dU=dU0 + c[:, None] * (N - P), dP=-c[:, None] * U,
                dN=c[:, None] * U, dpb=-c, dnb=c)


PAIR_SEED = 5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,d", [(1, 32), (3, 20), (64, 64), (200, 128), (37, 256)])
@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("with_w", [False, True])
def test_pair_kernel_matches_fp64(dev, kind, B, d, pad, acc, with_w):
    """arx_pair_loss_fwdbwd against fp64 numpy at the project's tolerance: leading dims d and d + 4, acc_dU, row
    weights, one void row (where the batch has a second row), forward-only with null gradients, two runs bit for
    bit."""
    import torch
    from arx import ops
    U, P, pb, N, nb, rw, dU0 = _pair_case(B, d, PAIR_SEED)
    void = np.zeros(B, dtype=bool)
    if B > 1:
        void[B // 2] = True
    gscale = 1.0 / B
    ref = _pair_ref(kind, U, P, pb, N, nb, void, rw if with_w else np.ones(B), gscale, dU0 if acc else 0 * dU0)
    if kind == 'bpr-hinge':
        assert np.abs(1.0 + ref['x']).min() > 1e-4        # no row near the kink: fp32 takes the same branch

    def mat(a):
        t = torch.zeros((B, d + pad), dtype=torch.float32, device=dev)
        t[:, :d] = torch.from_numpy(a)
        return t[:, :d]
    up = lambda a, dt=None: torch.from_numpy(a).to(dev) if dt is None else torch.from_numpy(a.astype(dt)).to(dev)
    Ud, Pd, Nd = mat(U), mat(P), mat(N)
    pbd, nbd, rwd = up(pb), up(nb), (up(rw) if with_w else None)
    ids = up(np.where(void, -1, 7), np.int32)
    runs = []
    for _ in range(2):
        out = {k: torch.full((B,), 9.0, dtype=torch.float32, device=dev) for k in ('ps', 'ns', 'loss', 'dpb', 'dnb')}
        dU, dP, dN = mat(dU0), mat(0 * dU0 + 9), mat(0 * dU0 + 9)
        ops.pair_loss(Ud, Pd, pbd, Nd, nbd, kind, gscale, out['ps'], out['ns'], out['loss'], neg_ids=ids,
                      row_w=rwd, dU=dU, acc_dU=bool(acc), dP=dP, dpbias=out['dpb'], dN=dN, dnbias=out['dnb'])
        out.update(dU=dU, dP=dP, dN=dN)
        runs.append({k: v.cpu().numpy().copy() for k, v in out.items()})
    for k, v in runs[0].items():
        np.testing.assert_allclose(v, ref[k], rtol=RTOL, atol=ATOL, err_msg=k)
        np.testing.assert_array_equal(v.view(np.uint32), runs[1][k].view(np.uint32), err_msg=k + ': second run')
    if void.any():
        r = int(np.nonzero(void)[0][0])
        for k in ('loss', 'dP', 'dN', 'dpb', 'dnb'):
            assert not np.any(runs[0][k][r]), k                               # exact zeros
        np.testing.assert_array_equal(runs[0]['dU'][r], dU0[r] if acc else 0 * dU0[r])
    # forward only: null gradients, the same scores and loss
    f = {k: torch.full((B,), 9.0, dtype=torch.float32, device=dev) for k in ('ps', 'ns', 'loss')}
    ops.pair_loss(Ud, Pd, pbd, Nd, nbd, kind, gscale, f['ps'], f['ns'], f['loss'], neg_ids=ids, row_w=rwd)
    for k, v in f.items():
        np.testing.assert_array_equal(v.cpu().numpy(), runs[0][k], err_msg=k + ': forward only')
    # auc over the rows that are not void
    auc = ops.pair_auc(f['ps'], f['ns'], ids, torch.zeros(1, dtype=torch.float32, device=dev))
    x32 = runs[0]['ns'] - runs[0]['ps']
    want = 0.5 - 0.5 * np.sign(x32[~void]).mean() if (~void).any() else 0.5
    assert abs(float(auc.item()) - want) < 1e-6


def test_pair_auc_of_void_rows_only_is_one_half(dev):
    import torch
    from arx import ops
    z = torch.zeros(5, dtype=torch.float32, device=dev)
    ids = torch.full((5,), -1, dtype=torch.int32, device=dev)
    out = torch.zeros(1, dtype=torch.float32, device=dev)
    assert float(ops.pair_auc(z, z + 1, ids, out).item()) == 0.5
    assert float(ops.pair_auc(z, z + 1, None, out).item()) == 0.0             # every negative above its positive


# ------------------------------------------------------------------ 2. whole step
def _build_pair(cfg, kind, d, B, seed, nonlinear='linear', use_graph=True):
    from arx.hmf.hmf_model import LatentProductModel
    from arx.utils.synthetic import SyntheticHMF
    syn = SyntheticHMF(seed=seed, **cfg)
    params = syn.glorot_params(d, seed=seed + 1, scale=0.5)
    if nonlinear in ('relu', 'tanh'):
        rng = np.random.default_rng(seed + 2)
        params['w1'] = (rng.standard_normal((d, 48)) * 0.3).astype(np.float32)
        params['b1'] = (rng.standard_normal((48,)) * 0.1).astype(np.float32)
        params['w2'] = (rng.standard_normal((48, d)) * 0.3).astype(np.float32)
        params['b2'] = (rng.standard_normal((d,)) * 0.1).astype(np.float32)
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind
    model = LatentProductModel(syn.n_users, syn.n_items, d, 1, B, 0.5, 1.0, syn.u_attr, syn.i_attr, i2l, l2i,
                               loss_function=kind, params=params, nonlinear=nonlinear, hidden_size=48,
                               top_N_items=10, use_graph=use_graph)
    # the oracle has no pair loss: a 'ce' model whose pieces _ref_pair_step composes
    ref = rg.RefLatentProductModel(d, B, 0.5, syn.u_attr, syn.i_attr, i2l, l2i, loss_function='ce', params=params,
                                   dtype=np.float64, top_N_items=10, nonlinear=nonlinear, hidden_size=48)
    return syn, model, ref


def _ref_pair_step(ref, users, pos, neg, kind, update=True):
    """hmf_model.py:96-107,132-133,140-151 from the oracle's pieces: user lookup, two target scores, the transform
    of embed_attribute.py:541-544, and the backward of the mean through both scores."""
    m = ref.att_emb
    u, c_user = m.get_batch_user(list(users), concat=False)
    c_mlp = None
    if ref.nonlinear in ('relu', 'tanh'):
        u, c_mlp = ref._mlp_fwd(u, None)
    ps, c_p = m.get_target_score(u, list(pos))
    ns, c_n = m.get_target_score(u, list(neg))
    x = ns - ps
    if kind == 'bpr':
        bl, g = np.logaddexp(0.0, x), 1.0 / (1.0 + np.exp(-x))
    else:
        bl, g = np.maximum(1.0 + x, 0.0), (1.0 + x > 0).astype(np.float64)
    B = len(users)
    if update:
        grads = rg.Grads()
        d_u = m.get_target_score_bwd(c_n, g / B, grads) + m.get_target_score_bwd(c_p, -g / B, grads)
        if c_mlp is not None:
            d_u = ref._mlp_bwd(c_mlp, d_u, grads)
        m.get_batch_user_bwd(c_user, d_u, grads)
        m.apply_gradients(grads, ref.learning_rate)
    return dict(loss=float(bl.mean()), ps=ps, ns=ns, x=x, bl=bl)


def _pair_batch(syn, B, rng, kind):
    """A batch with a duplicated user, an item that is positive in one row and negative in another, a duplicated
    negative and -- 'bpr' -- row 8 with neg == pos on an item no other row touches.  Returns (users, pos, neg, z)."""
    l2i = np.asarray(syn.logit_ind2item_ind)
    users, pos = syn.sample_batch(B, rng)
    neg = rng.choice(l2i, size=B).astype(np.int32)
    users[1] = users[0]
    neg[4] = pos[5]
    neg[6] = neg[7]
    z = None
    if kind == 'bpr':
        pos[8] = neg[8] = -1
        z = int(np.setdiff1d(l2i, np.concatenate([pos, neg]))[0])
        pos[8] = neg[8] = z
    return users, pos, neg, z


def _item_id_row(syn, item):
    """(table name, row) of the item's own row, or None where the items have no id feature (CFG_MIX)."""
    ia = syn.i_attr
    if ia.num_features_cat == 0:
        return None
    return 'itemembed_cat_0', int(np.asarray(ia.features_cat[0])[item])


WHOLE_STEP = [(cfg, d, B, kind, use_graph, 'linear')
              for cfg, d, B in ((CFG_ID, 64, 64), (CFG_HET, 64, 64), (CFG_MIX, 32, 48))
              for kind in KINDS for use_graph in (True, False)] + [(CFG_HET, 64, 64, 'bpr', True, 'tanh')]


@pytest.mark.parametrize("cfg,d,B,kind,use_graph,nonlinear", WHOLE_STEP)
def test_pair_steps_match_oracle(dev, cfg, d, B, kind, use_graph, nonlinear):
    syn, model, ref = _build_pair(cfg, kind, d, B, seed=3, nonlinear=nonlinear, use_graph=use_graph)
    rng = np.random.default_rng(11)
    tol = dict(rtol=1e-4, atol=1e-5) if nonlinear == 'tanh' else {}           # (test_mlp_variant's)
    for step in range(4):
        users, pos, neg, z = _pair_batch(syn, B, rng, kind)
        spot = _item_id_row(syn, z) if z is not None else None
        if spot is not None:
            before = (model.att_emb.get_params()[spot[0]][spot[1]].copy(),
                      model.att_emb.get_slots()[spot[0]][spot[1]].copy())
        r = _ref_pair_step(ref, users, pos, neg, kind)
        if kind == 'bpr-hinge':
            assert np.abs(1.0 + r['x']).min() > 1e-4, step
        got = model.step(None, list(users), list(pos), list(neg))
        np.testing.assert_allclose(got, r['loss'], rtol=RTOL, err_msg='step %d' % step)
        np.testing.assert_allclose(model.pos_score.read().cpu().numpy(), r['ps'], rtol=RTOL, atol=1e-5)
        np.testing.assert_allclose(model.neg_score.read().cpu().numpy(), r['ns'], rtol=RTOL, atol=1e-5)
        _compare_state(model, ref, **tol)
        # auc: exact unless a pair's scores are closer than fp32 can tell apart
        other = np.asarray(pos) != np.asarray(neg)
        close = int((np.abs(r['x'][other]) <= 1e-5).sum())
        assert close <= 1
        auc_ref = 0.5 - 0.5 * np.sign(r['x']).mean()
        auc = float(model.auc.read().item())
        print('step %d loss %.6f (oracle %.6f) auc %.6f (oracle %.6f) min|x| %.3g' %
              (step, got, r['loss'], auc, auc_ref, np.abs(r['x'][other]).min()))
        assert abs(auc - auc_ref) <= (close / B if close else 0) + 1e-6
        if z is not None:
            x_got = (model.neg_score.read() - model.pos_score.read()).cpu().numpy()
            assert x_got[8] == 0.0
            assert abs(float(model.batch_loss.value[8].item()) - np.log(2.0)) < 1e-6
            if spot is not None:      # +c U and -c U cancel exactly: the only contributor leaves the row alone
                np.testing.assert_array_equal(model.att_emb.get_params()[spot[0]][spot[1]], before[0])
                np.testing.assert_array_equal(model.att_emb.get_slots()[spot[0]][spot[1]], before[1])
    # forward_only: the same loss, no update
    users, pos, neg, _ = _pair_batch(syn, B, rng, kind)
    p0, s0 = model.att_emb.get_params(), model.att_emb.get_slots()
    e_ref = _ref_pair_step(ref, users, pos, neg, kind, update=False)
    e_got = model.step(None, list(users), list(pos), list(neg), forward_only=True)
    np.testing.assert_allclose(e_got, e_ref['loss'], rtol=RTOL)
    p1, s1 = model.att_emb.get_params(), model.att_emb.get_slots()
    for k in p0:
        np.testing.assert_array_equal(p0[k], p1[k], err_msg=k)
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=k + '/Adagrad')


# ------------------------------------------------------------------ 3. / 4. the draw
V_DRAW = 50


def _draw_lists(rng):
    V = V_DRAW
    return [np.zeros(0, dtype=np.int64),                                     # 0: no positives
            np.asarray([c for c in range(V) if c != 17]),                    # 1: all but one column
            np.arange(V),                                                    # 2: every column -> void
            np.sort(rng.choice(V, 13, replace=False)),                       # 3: 37 eligible columns
            np.arange(20),                                                   # 4: a leading run
            np.arange(V - 20, V)]                                            # 5: a trailing run


def _csr(lists, dev):
    import torch
    ptr = np.zeros(len(lists) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    cols = np.concatenate(lists).astype(np.int32)
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(cols).to(dev)


def _draw(users_d, ptr, cols, col2item, seed, step, counter, dev, with_lookup=False):
    import torch
    from arx import ops
    B = users_d.shape[0]
    out, rank = (torch.full((B,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    look = torch.full((B,), -7, dtype=torch.int32, device=dev) if with_lookup else None
    step_dev = None if step is None else torch.tensor([step], dtype=torch.int64, device=dev)
    ops.neg_draw_uniform(users_d, ptr, cols, V_DRAW, col2item, seed, step_dev, counter, out, lookup_items=look,
                         out_rank=rank)
    res = (out.cpu().numpy(), rank.cpu().numpy())
    return res + (look.cpu().numpy(),) if with_lookup else res


def test_neg_draw_is_the_rank_select_of_its_rank(dev):
    import torch
    rng = np.random.default_rng(0)
    lists = _draw_lists(rng)
    ptr, cols = _csr(lists, dev)
    col2item_np = (rng.permutation(V_DRAW) * 2 + 1).astype(np.int32)          # not the identity
    col2item = torch.from_numpy(col2item_np).to(dev)
    B = 4096
    users = rng.choice(np.asarray([0, 1, 2, 3, 4, 5, -1, 99], dtype=np.int32), size=B)   # -1 / 99: out of range
    users_d = torch.from_numpy(users).to(dev)
    items, rank, look = _draw(users_d, ptr, cols, col2item, 5, 3, 0, dev, with_lookup=True)
    for r in range(B):
        lst = lists[users[r]] if 0 <= users[r] < len(lists) else lists[0]
        n_elig = V_DRAW - len(lst)
        if n_elig == 0:
            assert items[r] == -1 and rank[r] == -1 and look[r] == col2item_np[0]
            continue
        assert 0 <= rank[r] < n_elig
        col = rank_select(lst, rank[r])
        assert col not in set(lst.tolist())
        assert items[r] == col2item_np[col] == look[r], r
    assert (rank[users == 1] == 0).all() and (items[users == 1] == col2item_np[17]).all()
    # every eligible rank of the 37-column user turns up in ~500 rows
    assert set(rank[users == 3].tolist()) == set(range(37))
    # the same (seed, counter) -> the same draw; the device counter and the host offset add up
    again = _draw(users_d, ptr, cols, col2item, 5, 3, 0, dev)
    np.testing.assert_array_equal(again[0], items)
    np.testing.assert_array_equal(_draw(users_d, ptr, cols, col2item, 5, None, 3, dev)[0], items)
    np.testing.assert_array_equal(_draw(users_d, ptr, cols, col2item, 5, 1, 2, dev)[0], items)
    # another counter, another seed: more than half the rows change
    assert (_draw(users_d, ptr, cols, col2item, 5, 4, 0, dev)[0] != items).mean() > 0.5
    assert (_draw(users_d, ptr, cols, col2item, 6, 3, 0, dev)[0] != items).mean() > 0.5
    # without col2item the columns themselves come back
    plain, prank = _draw(users_d, ptr, cols, None, 5, 3, 0, dev)
    np.testing.assert_array_equal(prank, rank)
    live = items >= 0
    np.testing.assert_array_equal(col2item_np[plain[live]], items[live])
    assert (plain[~live] == -1).all()


def test_neg_draw_is_uniform_over_the_eligible_columns(dev):
    """Pearson's statistic of 4 x 8192 draws over 37 eligible columns stays below the mean plus six standard
    deviations of chi-square with 36 degrees of freedom."""
    import torch
    rng = np.random.default_rng(1)
    lists = _draw_lists(rng)
    ptr, cols = _csr(lists, dev)
    users_d = torch.full((8192,), 3, dtype=torch.int32, device=dev)
    counts = np.zeros(37)
    for counter in range(4):
        items, rank = _draw(users_d, ptr, cols, None, 9, counter, 0, dev)
        assert not np.isin(items, lists[3]).any()
        counts += np.bincount(rank, minlength=37)
    n = counts.sum()
    assert n == 4 * 8192
    chi2 = float(((counts - n / 37) ** 2 / (n / 37)).sum())
    print('chi2 = %.2f' % chi2)
    assert chi2 < 36 + 6 * np.sqrt(72)


# ------------------------------------------------------------------ 5. the model draws its negatives
def test_model_draws_negatives_inside_the_captured_step(dev):
    B, d = 64, 32
    syn, model, _ = _build_pair(CFG_ID, 'bpr', d, B, seed=4, use_graph=True)
    l2i = np.asarray(syn.logit_ind2item_ind)
    rng = np.random.default_rng(2)
    users, pos = syn.sample_batch(B, rng)
    with pytest.raises(ValueError):
        model.step(None, list(users), list(pos), None)                        # nothing prepared: before any launch
    with pytest.raises(ValueError):
        model.step(None, list(users), list(pos), [])
    hist = syn.positives_dict()
    u_full = 7
    hist[u_full] = l2i.tolist()                                               # this user has seen everything
    model.prepare_pair_negatives(hist, seed=3)
    m = model.att_emb
    urow = int(np.asarray(syn.u_attr.features_cat[0])[u_full])
    prev, graph = None, None
    for step in range(6):
        users, pos = syn.sample_batch(B, rng)
        users[users == u_full] = u_full + 1
        users[0] = u_full
        urow_before = m.get_params()['userembed_cat_0'][urow].copy()
        model.prepare_next(users, pos)                                        # announced, but the plan cannot ring:
        loss = model.step(None, list(users), list(pos), None)                 # its 'neg' ids are not known a step early
        plan = model._plan('train_draw')
        assert not plan._ring_ready
        assert np.isfinite(loss)
        ids = m.neg_draw.value.cpu().numpy()
        fed = m.i_indices['neg'].value.cpu().numpy()
        assert ids[0] == -1 and (ids[1:] >= 0).all()
        np.testing.assert_array_equal(fed[1:], ids[1:])
        assert fed[0] == l2i[0]
        for r in range(1, B):
            assert ids[r] in set(l2i.tolist()) and ids[r] not in set(hist[int(users[r])]), (step, r)
        # the void row: no loss, and its user's row is untouched
        assert float(model.batch_loss.value[0].item()) == 0.0
        np.testing.assert_array_equal(m.get_params()['userembed_cat_0'][urow], urow_before)
        if prev is not None:
            assert (ids != prev).mean() > 0.5                                 # a replay draws anew
        prev = ids
        if step == 1:
            graph = plan.graph
            assert graph is not None
        if step > 1:
            assert plan.graph is graph                                        # one capture
    # forward_only draws through the same path and updates nothing
    p0 = m.get_params()
    e = model.step(None, list(users), list(pos), None, forward_only=True)
    assert np.isfinite(e)
    for k, v in m.get_params().items():
        np.testing.assert_array_equal(v, p0[k], err_msg=k)
    # fed negatives still work on the same model, and new lists replace the old
    model.step(None, list(users), list(pos), list(rng.choice(l2i, size=B)))
    model.prepare_pair_negatives(syn.positives_dict(), seed=4)
    assert 'train_draw' not in model._plans
    model.step(None, list(users), list(pos), None)
    assert (m.neg_draw.value.cpu().numpy() >= 0).all()


# ------------------------------------------------------------------ 6. unchanged paths
def test_recommend_of_a_pair_model_and_the_mw_path(dev):
    B, d = 64, 64
    syn, model, ref = _build_pair(CFG_ID, 'bpr', d, B, seed=6)
    rng = np.random.default_rng(3)
    users, pos, neg, _ = _pair_batch(syn, B, rng, 'bpr')
    r = _ref_pair_step(ref, users, pos, neg, 'bpr')
    np.testing.assert_allclose(model.step(None, list(users), list(pos), list(neg)), r['loss'], rtol=RTOL)
    r_ref = ref.step(list(users), None, recommend=True)
    np.testing.assert_array_equal(model.step(None, list(users), None, recommend=True), r_ref)
    # exclude_seen: the oracle's logits without each user's history
    sets = syn.positives_dict()
    model.prepare_recommend_exclusions(sets)
    u, _ = ref.att_emb.get_batch_user(list(users), concat=False)
    logits, _ = ref.att_emb.get_prediction(u, 'full')
    logits = np.array(logits, dtype=np.float64)
    for row, usr in enumerate(users):
        logits[row, syn.item2logit[np.asarray(sets[int(usr)])]] = -np.inf
    want = np.argsort(-logits, axis=1, kind='stable')[:, :10].astype(np.int32)
    np.testing.assert_array_equal(model.step(None, list(users), None, recommend=True, exclude_seen=True), want)
    # 'mw' on the same configuration still runs the fused scorer
    from conftest import assert_mw_scorer_path
    from test_hmf_gpu import _build
    S = 256
    syn2, mw, _ = _build(CFG_ID, 'mw', 128, B, S, seed=3)
    pool = syn2.sample_pool(S, rng)
    users, items = syn2.sample_batch(B, rng)
    mw.step(None, list(users), list(items), None, pool, {int(v): i for i, v in enumerate(pool)}, loss='mw')
    assert assert_mw_scorer_path(mw._plan('train'), B, S, 128)
