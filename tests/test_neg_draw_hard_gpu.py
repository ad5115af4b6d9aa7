"""The hardest of C drawn negatives on the device (arx_neg_draw_hardest, include/arx_neg_hard.h): the kernel against the
composition of its parts -- the plain draws at C consecutive counters, arx_slate_scores on the gathered rows, a first
arg-max in numpy --, its tie and non-finite rules, rows past the grid cap, LatentProductModel training against the pick
inside its captured step, and the refusals of prepare_pair_negatives(hardest_of=)."""
import numpy as np
import pytest

from test_bpr_gpu import _build_pair
from test_hmf_gpu import CFG_HET, CFG_ID

pytestmark = pytest.mark.gpu

V_DRAW = 50
N_UROWS, N_PROWS = 40, 70
NINF_BITS = np.float32(-np.inf).view(np.int32)


# ------------------------------------------------------------------ shared pieces
def _draw_lists(rng):
    """The lists of test_bpr_gpu._draw_lists, restated."""
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
    cols = np.concatenate(lists + [np.zeros(1, dtype=np.int64)]).astype(np.int32)     # (never an empty tensor: a pointer)
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(cols).to(dev)


def _weight_tables(q, lists, dev):
    """cum and ex_cum of integer column weights q, stated directly."""
    import torch
    cum = np.concatenate([[0], np.cumsum(q)]).astype(np.int64)
    ex = [np.concatenate([[0], np.cumsum(q[np.asarray(l, dtype=np.int64)])])[:len(l)] for l in lists]
    ex_cum = np.concatenate(ex + [np.zeros(1)]).astype(np.int64)                      # (aligned with _csr's cols)
    return torch.from_numpy(ex_cum).to(dev), torch.from_numpy(cum).to(dev)


def _up(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Case(object):
    """The operands of one launch, on the host (numpy, None where the kernel gets NULL) and on the device."""

    def __init__(self, dev, users, ptr, cols, V, U, P, pbias=None, umap=None, col2row=None, col2item=None,
                 ex_cum=None, cum=None, pad=0):
        import torch
        self.dev, self.V = dev, V
        self.users_np, self.U_np, self.P_np, self.pbias_np = users, U, P, pbias
        self.umap_np, self.col2row_np, self.col2item_np = umap, col2row, col2item
        self.users, self.ptr, self.cols, self.ex_cum, self.cum = _up(users, dev), ptr, cols, ex_cum, cum

        def mat(a):                              # (pad: a strided view, leading dimension d + pad)
            t = torch.zeros((a.shape[0], a.shape[1] + pad), dtype=torch.float32, device=dev)
            t[:, :a.shape[1]] = torch.from_numpy(a)
            return t[:, :a.shape[1]]
        self.U, self.P = mat(U), mat(P)
        self.pbias, self.umap, self.col2row, self.col2item = (_up(a, dev) for a in (pbias, umap, col2row, col2item))


def _hard(case, C, seed, step, counter, extra=3):
    """One launch into sentinel-filled buffers -> dict of numpy arrays (score: the int32 bit patterns)."""
    import torch
    from arx import ops
    B, dev = case.users.shape[0], case.dev
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=dev)
    out = dict(items=i32(B), look=i32(B), pick=i32(B), cand=i32(B, C + extra),
               score=torch.full((B, C + extra), 7.0, dtype=torch.float32, device=dev))
    step_dev = None if step is None else torch.tensor([step], dtype=torch.int64, device=dev)
    ops.neg_draw_hard(case.users, case.ptr, case.cols, case.ex_cum, case.cum, case.V, case.col2item, seed, step_dev,
                      counter, C, case.U, case.umap, case.P, case.pbias, case.col2row, out['items'],
                      lookup_items=out['look'], out_pick=out['pick'], out_cand=out['cand'], out_score=out['score'])
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res['score'] = res['score'].view(np.int32)
    return res


def _plain_columns(case, C, seed, counter):
    """[B, C] int32: column j is the EXISTING draw kernel at counter + j (no col2item: the columns themselves)."""
    import torch
    from arx import ops
    B = case.users.shape[0]
    out = torch.full((C, B), -7, dtype=torch.int32, device=case.dev)
    for j in range(C):
        if case.cum is None:
            ops.neg_draw_uniform(case.users, case.ptr, case.cols, case.V, None, seed, None, counter + j, out[j])
        else:
            ops.neg_draw_weighted(case.users, case.ptr, case.cols, case.ex_cum, case.cum, case.V, None, seed, None,
                                  counter + j, out[j])
    return out.t().contiguous()


def _compose(case, C, seed, counter):
    """What the kernel must return, from parts that share no code with it: the plain draws, arx_slate_scores on the
    gathered user rows and the candidates' table rows, and the first arg-max of the NaN-cleaned scores in numpy."""
    import torch
    from arx import ops
    users, B = case.users_np.astype(np.int64), len(case.users_np)
    if case.umap_np is not None:
        inmap = (users >= 0) & (users < len(case.umap_np))
        urow = np.where(inmap, case.umap_np[np.where(inmap, users, 0)], -1).astype(np.int64)
    else:
        urow = users
    has_u = (urow >= 0) & (urow < case.U_np.shape[0])
    cand_d = _plain_columns(case, C, seed, counter)
    cand = cand_d.cpu().numpy()
    draws = cand[:, 0] >= 0
    assert ((cand >= 0) == draws[:, None]).all()                      # a void draw is void at every counter
    void = ~(draws & has_u)
    cand[void] = -1
    prow = cand if case.col2row_np is None else np.where(cand >= 0, case.col2row_np[np.maximum(cand, 0)], -1)
    Ug = case.U[torch.from_numpy(np.where(has_u, urow, 0)).to(case.dev)].contiguous()
    sc_d = torch.full((B, C), 7.0, dtype=torch.float32, device=case.dev)
    ops.slate_scores(Ug, case.P, case.pbias, _up(prow.astype(np.int32), case.dev), sc_d)
    score = sc_d.cpu().numpy()
    clean = np.where(np.isnan(score), -np.inf, score)
    pick = np.where(void, -1, np.argmax(clean, axis=1)).astype(np.int32)          # (argmax: the FIRST maximum)
    c_pick = np.where(void, -1, cand[np.arange(B), np.maximum(pick, 0)])
    c2i = case.col2item_np
    item = c_pick if c2i is None else np.where(c_pick >= 0, c2i[np.maximum(c_pick, 0)], -1)
    look = np.where(item >= 0, item, 0 if c2i is None else c2i[0])
    return dict(items=item.astype(np.int32), look=look.astype(np.int32), pick=pick, cand=cand,
                score=score.view(np.int32), void=void, clean=clean)


def _assert_composition(got, want, C):
    np.testing.assert_array_equal(got['cand'][:, :C], want['cand'], err_msg='candidates')
    np.testing.assert_array_equal(got['score'][:, :C], want['score'], err_msg='score bits')
    np.testing.assert_array_equal(got['pick'], want['pick'], err_msg='pick')
    np.testing.assert_array_equal(got['items'], want['items'], err_msg='items')
    np.testing.assert_array_equal(got['look'], want['look'], err_msg='lookup items')
    assert (got['cand'][:, C:] == -7).all() and (got['score'][:, C:] == np.float32(7.0).view(np.int32)).all()
    v = want['void']
    assert (got['items'][v] == -1).all() and (got['pick'][v] == -1).all()
    assert (got['cand'][v, :C] == -1).all() and (got['score'][v, :C] == NINF_BITS).all()


def _tables(d, seed):
    rng = np.random.default_rng(seed)
    s = np.float32(0.5 / d ** 0.25)
    U = rng.standard_normal((N_UROWS, d)).astype(np.float32) * s
    P = rng.standard_normal((N_PROWS, d)).astype(np.float32) * s
    pbias = (rng.standard_normal(N_PROWS) * 0.1).astype(np.float32)
    return U, P, pbias


# ------------------------------------------------------------------ 1. the composition of its parts
@pytest.mark.parametrize("rule", ['uniform', 'weighted'])
@pytest.mark.parametrize("d", [4, 32, 64, 128, 200, 256])
@pytest.mark.parametrize("C", [2, 5, 16, 64])
def test_kernel_is_the_composition_of_draw_score_and_pick(dev, rule, d, C):
    """Users 0..5 own the lists, 6 and 7 have none (everything is eligible), -1 and 99 are out of range.  Once with
    non-identity umap (user 7 -> a row outside U, 99 and -1 outside the map), col2row (one column -> a row outside P,
    one -> -1), col2item, a bias and padded tables; once with all three maps and the bias NULL (users 99 and -1 then
    name no row of U)."""
    rng = np.random.default_rng(0)
    V, B = V_DRAW, 1024
    lists = _draw_lists(rng)
    ptr, cols = _csr(lists, dev)
    ex_cum = cum = None
    if rule == 'weighted':
        q = rng.integers(1, (1 << 32) + 1, size=V).astype(np.int64)
        q[rng.random(V) < 0.3] = 0
        q[17] = 1 << 32                                           # (user 1's only column has weight)
        ex_cum, cum = _weight_tables(q, lists, dev)
    users = rng.choice(np.asarray([0, 1, 2, 3, 4, 5, 6, 7, -1, 99], dtype=np.int32), size=B)
    U, P, pbias = _tables(d, 1)
    umap = rng.permutation(N_UROWS)[:8].astype(np.int32)
    umap[7] = N_UROWS + 3
    col2row = rng.permutation(N_PROWS)[:V].astype(np.int32)
    col2row[5], col2row[6] = N_PROWS + 2, -1
    col2item = (rng.permutation(V) * 2 + 1).astype(np.int32)
    seed, step, counter = 5, 3, 2
    for mapped in (True, False):
        kw = dict(pbias=pbias, umap=umap, col2row=col2row, col2item=col2item, pad=4) if mapped else {}
        case = Case(dev, users, ptr, cols, V, U, P, ex_cum=ex_cum, cum=cum, **kw)
        got = _hard(case, C, seed, step, counter)
        want = _compose(case, C, seed, step + counter)
        _assert_composition(got, want, C)
        void_users = ([2, 7, -1, 99] if mapped else [2, -1, 99])
        np.testing.assert_array_equal(want['void'], np.isin(users, void_users))
        assert (got['cand'][users == 1, :C] == 17).all()          # the all-but-one user: column 17, whatever C
        assert (got['items'][users == 1] == (col2item[17] if mapped else 17)).all()
        if mapped:                                                # the -inf candidates never win against a score
            live = ~want['void']
            assert (np.isin(got['cand'][live, :C], [5, 6]) == (got['score'][live, :C] == NINF_BITS)).all()
        # the device counter and the host offset add up; the same arguments give the same bits
        again = _hard(case, C, seed, None, step + counter)
        for k in got:
            np.testing.assert_array_equal(again[k], got[k], err_msg=k)
    assert len(set(got['pick'][users == 3].tolist())) >= 2        # the pick moves with the scores


# ------------------------------------------------------------------ 2. ties and non-finite scores
def _rule_case(dev, P, pbias, users=None, umap=None, B=256):
    V, d = V_DRAW, 32
    ptr, cols = _csr([np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)], dev)
    U, _, _ = _tables(d, 2)
    users = np.zeros(B, dtype=np.int32) if users is None else users
    col2row = (np.arange(V) // 2).astype(np.int32)                # two columns share every table row
    return Case(dev, users, ptr, cols, V, U, P, pbias=pbias, umap=umap, col2row=col2row)


def test_ties_go_to_the_earlier_candidate_and_nan_never_wins(dev):
    C, d = 16, 32
    _, P, pbias = _tables(d, 2)
    # ties: columns 2k and 2k + 1 read the same row and score the same bits
    case = _rule_case(dev, P, pbias)
    got, want = _hard(case, C, 9, None, 0), _compose(case, C, 9, 0)
    _assert_composition(got, want, C)
    r = np.arange(len(got['pick']))
    best = want['clean'].max(axis=1)
    tied = (want['clean'] == best[:, None]).sum(axis=1) >= 2
    first = np.argmax(want['clean'] == best[:, None], axis=1)
    other = np.asarray([(got['cand'][i, :C][want['clean'][i] == best[i]] != got['cand'][i, first[i]]).any()
                        for i in r])
    assert (tied & other).sum() > 10                              # ties between DIFFERENT columns do occur
    np.testing.assert_array_equal(got['pick'], first)
    # NaN rows never win against a finite score; +inf (a bias) wins
    Pn, bn = P.copy(), pbias.copy()
    Pn[:12] = np.nan                                              # columns 0 .. 23
    bn[20] = np.inf                                               # columns 40, 41
    case = _rule_case(dev, Pn, bn)
    got, want = _hard(case, C, 9, None, 0), _compose(case, C, 9, 0)
    _assert_composition(got, want, C)
    sc = got['score'][:, :C].view(np.float32)
    picked = sc[r, got['pick']]
    assert np.isnan(sc).any(axis=1).all()                         # (every row holds a NaN candidate)
    anyfin = (~np.isnan(sc)).any(axis=1)
    assert anyfin.sum() > 200 and not np.isnan(picked[anyfin]).any()
    has_inf = (sc == np.inf).any(axis=1)
    assert has_inf.sum() > 20 and (picked[has_inf] == np.inf).all()
    np.testing.assert_array_equal(got['pick'][has_inf], np.argmax(sc[has_inf] == np.inf, axis=1))
    # every score NaN: candidate 0
    case = _rule_case(dev, np.full_like(P, np.nan), pbias)
    got = _hard(case, C, 9, None, 0)
    assert np.isnan(got['score'][:, :C].view(np.float32)).all() and (got['pick'] == 0).all()
    np.testing.assert_array_equal(got['items'], got['cand'][:, 0])


def test_a_user_without_a_table_row_is_void_and_its_neighbours_are_intact(dev):
    """Odd rows belong to a user whose umap entry is out of range.  The even rows equal those of a run where every
    row is valid (the draw is keyed by the row), and the buffers around the live range keep their sentinels."""
    import torch
    from arx import ops
    C, d, B, pad = 5, 32, 64, 16
    _, P, pbias = _tables(d, 2)
    umap = np.asarray([3, N_UROWS + 1], dtype=np.int32)
    users = (np.arange(B) % 2).astype(np.int32)
    case = _rule_case(dev, P, pbias, users=users, umap=umap, B=B)
    full = _hard(_rule_case(dev, P, pbias, users=np.zeros(B, dtype=np.int32), umap=umap, B=B), C, 4, None, 0, extra=0)
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    items, look, pick, cand = i32(B + 2 * pad), i32(B + 2 * pad), i32(B + 2 * pad), i32(B + 2 * pad, C)
    score = torch.full((B + 2 * pad, C), 7.0, dtype=torch.float32, device=dev)
    live = slice(pad, pad + B)
    ops.neg_draw_hard(case.users, case.ptr, case.cols, None, None, case.V, None, 4, None, 0, C, case.U, case.umap,
                      case.P, case.pbias, case.col2row, items[live], lookup_items=look[live], out_pick=pick[live],
                      out_cand=cand[live], out_score=score[live])
    got = dict(items=items, look=look, pick=pick, cand=cand, score=score)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    got['score'] = got['score'].view(np.int32)
    for k, v in got.items():
        sentinel = np.float32(7.0).view(np.int32) if k == 'score' else -7
        assert (v[:pad] == sentinel).all() and (v[pad + B:] == sentinel).all(), k
        np.testing.assert_array_equal(v[live][0::2], full[k][0::2], err_msg=k)
    odd = {k: v[live][1::2] for k, v in got.items()}
    assert (odd['items'] == -1).all() and (odd['pick'] == -1).all() and (odd['look'] == 0).all()
    assert (odd['cand'] == -1).all() and (odd['score'] == NINF_BITS).all()
    assert (full['items'] >= 0).all()


# ------------------------------------------------------------------ 3. past the grid cap
def test_rows_past_the_grid_cap_take_further_trips(dev):
    """The launch rule, restated: one wave per row, 4 waves per workgroup, at most 8 * cu workgroups; the waves stride
    the rows.  B exceeds two full trips, so rows are served by a third."""
    from arx import ops
    cu = ops.device_info()['cu_count']
    C, d = 2, 4
    B = 2 * (8 * cu * 4) + 37
    waves = min(-(-B // 4), 8 * cu) * 4
    assert B > 2 * waves
    rng = np.random.default_rng(7)
    lists = _draw_lists(rng)
    ptr, cols = _csr(lists, dev)
    users = rng.choice(np.asarray([0, 1, 2, 3, 4, 5, 6, -1], dtype=np.int32), size=B)
    U, P, pbias = _tables(d, 3)
    col2row = rng.permutation(N_PROWS)[:V_DRAW].astype(np.int32)
    case = Case(dev, users, ptr, cols, V_DRAW, U, P, pbias=pbias, col2row=col2row)
    got, want = _hard(case, C, 11, 1, 0), _compose(case, C, 11, 1)
    _assert_composition(got, want, C)
    tail = slice(2 * waves, B)
    assert (~want['void'][tail]).sum() > 10 and want['void'][tail].any()


# ------------------------------------------------------------------ 4. the model
def _model_replay(m, syn, params, users, C, seed, counter, dev):
    """The kernel itself on a get_params() snapshot, the model's lists and the given seed and counter."""
    import torch
    from arx import ops
    l2i = np.asarray(syn.logit_ind2item_ind)
    ptr, cols, c2i, ex_cum, cum = m._pair_lists
    U, P = _up(params['userembed_cat_0'], dev), _up(params['itemembed_cat_0'], dev)
    pbias = _up(params['item_bias_cat_0'].reshape(-1), dev)
    umap = _up(np.asarray(syn.u_attr.features_cat[0], dtype=np.int32), dev)
    col2row = _up(np.asarray(syn.i_attr.features_cat[0], dtype=np.int32)[l2i], dev)
    out = torch.full((len(users),), -7, dtype=torch.int32, device=dev)
    ops.neg_draw_hard(_up(np.asarray(users, dtype=np.int32), dev), ptr, cols, ex_cum, cum, m.logit_size, c2i, seed,
                      None, counter, C, U, umap, P, pbias, col2row, out)
    return out.cpu().numpy()


def _plain_items(m, users, seed, counter, dev):
    import torch
    from arx import ops
    ptr, cols, c2i = m._pair_lists[:3]
    out = torch.full((len(users),), -7, dtype=torch.int32, device=dev)
    ops.neg_draw_uniform(_up(np.asarray(users, dtype=np.int32), dev), ptr, cols, m.logit_size, c2i, seed, None,
                         counter, out)
    return out.cpu().numpy()


def test_model_trains_against_the_hardest_of_eight_inside_the_captured_step(dev):
    B, d, C = 64, 32, 8
    syn, model, _ = _build_pair(CFG_ID, 'bpr', d, B, seed=4, use_graph=True)
    l2i = np.asarray(syn.logit_ind2item_ind)
    rng = np.random.default_rng(2)
    hist = syn.positives_dict()
    u_full = 7
    hist[u_full] = l2i.tolist()                                               # this user has seen everything
    model.prepare_pair_negatives(hist, seed=3, hardest_of=C)
    m = model.att_emb
    urow = int(np.asarray(syn.u_attr.features_cat[0])[u_full])
    graph = None
    for step in range(6):
        users, pos = syn.sample_batch(B, rng)
        users[users == u_full] = u_full + 1
        users[0] = u_full
        before = m.get_params()
        assert int(m.neg_draw.counter.item()) == C * step
        loss = model.step(None, list(users), list(pos), None)
        plan = model._plan('train_draw')
        assert np.isfinite(loss)
        ids = m.neg_draw.value.cpu().numpy()
        fed = m.i_indices['neg'].value.cpu().numpy()
        # the kernel itself, on the tables as they stood before the step
        np.testing.assert_array_equal(ids, _model_replay(m, syn, before, users, C, 3, C * step, dev), err_msg=str(step))
        assert ids[0] == -1 and (ids[1:] >= 0).all()
        np.testing.assert_array_equal(fed[1:], ids[1:])
        assert fed[0] == l2i[0]
        plain = np.stack([_plain_items(m, users, 3, C * step + j, dev) for j in range(C)], axis=1)
        for r in range(1, B):
            assert ids[r] in set(plain[r].tolist()) and ids[r] not in set(hist[int(users[r])]), (step, r)
        # the void row: no loss, and its user's row is untouched
        assert float(model.batch_loss.value[0].item()) == 0.0
        np.testing.assert_array_equal(m.get_params()['userembed_cat_0'][urow], before['userembed_cat_0'][urow])
        if step == 1:
            graph = plan.graph
            assert graph is not None
        if step > 1:
            assert plan.graph is graph                                        # one capture
    # forward_only: the plain draw at the current counter, one bump, nothing updated
    c0 = int(m.neg_draw.counter.item())
    assert c0 == 6 * C
    p0 = m.get_params()
    e = model.step(None, list(users), list(pos), None, forward_only=True)
    assert np.isfinite(e) and int(m.neg_draw.counter.item()) == c0 + 1
    plain_ids = m.neg_draw.value.cpu().numpy()
    np.testing.assert_array_equal(plain_ids, _plain_items(m, users, 3, c0, dev))
    plain_ns = model.neg_score.read().cpu().numpy().copy()
    for k, v in m.get_params().items():
        np.testing.assert_array_equal(v, p0[k], err_msg=k)
    # the same batch, the same tables, the counter set back: candidate 0 of the hard step is that plain draw, so the
    # hard negatives score at least as high row by row (up to the last bits of two orders of adds) and higher on average
    m.neg_draw.counter.fill_(c0)
    model.step(None, list(users), list(pos), None)
    assert int(m.neg_draw.counter.item()) == c0 + C
    hard_ids = m.neg_draw.value.cpu().numpy()
    np.testing.assert_array_equal(hard_ids, _model_replay(m, syn, p0, users, C, 3, c0, dev))
    hard_ns = model.neg_score.read().cpu().numpy()
    live = plain_ids >= 0
    assert live.sum() == B - 1 and (hard_ids != plain_ids).sum() > B // 2
    print('mean neg_score: plain %.6f, hardest of %d %.6f' % (plain_ns[live].mean(), C, hard_ns[live].mean()))
    assert hard_ns[live].mean() > plain_ns[live].mean()
    # fed negatives still work on the same model
    model.step(None, list(users), list(pos), list(rng.choice(l2i, size=B)))
    # without the argument the model is back on plain draws, and the plan is dropped
    model.prepare_pair_negatives(syn.positives_dict(), seed=4)
    assert 'train_draw' not in model._plans and m.neg_draw.hard is None
    c1 = int(m.neg_draw.counter.item())
    model.step(None, list(users), list(pos), None)
    assert int(m.neg_draw.counter.item()) == c1 + 1
    np.testing.assert_array_equal(m.neg_draw.value.cpu().numpy(), _plain_items(m, users, 4, c1, dev))


# ------------------------------------------------------------------ 5. refusals
def _steps_plainly(model, syn, rng, B):
    users, pos = syn.sample_batch(B, rng)
    assert np.isfinite(model.step(None, list(users), list(pos), None))
    assert model.att_emb.neg_draw.hard is None and 'train_draw' in model._plans


@pytest.mark.parametrize("cfg,nonlinear,what", [(CFG_HET, 'linear', 'item'), (CFG_ID, 'relu', 'relu')])
def test_prepare_refuses_what_it_cannot_score(dev, cfg, nonlinear, what):
    B = 64
    syn, model, _ = _build_pair(cfg, 'bpr', 32, B, seed=4, nonlinear=nonlinear)
    rng = np.random.default_rng(5)
    model.prepare_pair_negatives(syn.positives_dict(), seed=3)
    _steps_plainly(model, syn, rng, B)
    lists = model.att_emb._pair_lists
    with pytest.raises(NotImplementedError, match=what):
        model.prepare_pair_negatives(syn.positives_dict(), seed=9, hardest_of=8)
    assert model.att_emb._pair_lists is lists and model.att_emb.neg_draw.seed == 3
    _steps_plainly(model, syn, rng, B)                            # the earlier prepare is in force, plan and all


def test_prepare_refuses_a_bad_hardest_of(dev):
    B = 64
    syn, model, _ = _build_pair(CFG_ID, 'bpr', 32, B, seed=4)
    rng = np.random.default_rng(5)
    model.prepare_pair_negatives(syn.positives_dict(), seed=3)
    _steps_plainly(model, syn, rng, B)
    for bad in (1, 65, 2.5):
        with pytest.raises(ValueError, match='hardest_of'):
            model.prepare_pair_negatives(syn.positives_dict(), seed=9, hardest_of=bad)
        assert model.att_emb.neg_draw.seed == 3
        _steps_plainly(model, syn, rng, B)
