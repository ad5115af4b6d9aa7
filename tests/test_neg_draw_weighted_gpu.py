"""The weighted pair draw on the device (arx_neg_draw_weighted): every row against the masked cumulative sum and the
RNG in Python integers, deep binary searches, the drawn distribution, and the two models drawing by popularity --
LatentProductModel inside its captured step, ShardedHMF in prepare_route."""
import os

import numpy as np
import pytest

from numpy_backend_pair import PairRef
from test_bpr_gpu import CFG_ID, V_DRAW, _build_pair, _csr, _draw_lists
from test_hmf_gpu import ATOL, RTOL
from test_neg_draw_weighted_cpu import brute, draw_key, eligible_mass

pytestmark = pytest.mark.gpu


def _tables_of(q, lists):
    """cum and ex_cum of integer weights q, stated directly."""
    cum = np.concatenate([[0], np.cumsum(q)]).astype(np.int64)
    ex = [np.concatenate([[0], np.cumsum(q[np.asarray(l, dtype=np.int64)])])[:len(l)] for l in lists]
    ex_cum = np.concatenate(ex + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return cum, (ex_cum if len(ex_cum) else np.zeros(1, dtype=np.int64))


def _draw_w(users_d, ptr, cols, ex_cum, cum, V, col2item, seed, step, counter, dev):
    """-> (items, mass, lookup) of one launch; step None: no device counter."""
    import torch
    from arx import ops
    B = users_d.shape[0]
    out, look = (torch.full((B,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    mass = torch.full((B,), -7, dtype=torch.int64, device=dev)
    step_dev = None if step is None else torch.tensor([step], dtype=torch.int64, device=dev)
    ops.neg_draw_weighted(users_d, ptr, cols, ex_cum, cum, V, col2item, seed, step_dev, counter, out,
                          lookup_items=look, out_mass=mass)
    return out.cpu().numpy(), mass.cpu().numpy(), look.cpu().numpy()


# ------------------------------------------------------------------ 1. exact select
def test_weighted_draw_is_the_column_of_its_mass_point(dev):
    import torch
    V = V_DRAW
    rng = np.random.default_rng(0)
    lists = _draw_lists(rng)
    q = rng.integers(1, (1 << 32) + 1, size=V).astype(np.int64)
    q[rng.random(V) < 0.3] = 0
    outside3 = np.setdiff1d(np.arange(V), lists[3])
    beside = [c for c in outside3 if c - 1 in lists[3] or c + 1 in lists[3]]
    q[beside[0]], q[beside[2]], q[beside[-1]] = 0, 0, 0          # zero weights directly beside list entries
    q[17], q[V - 1], q[0] = 1 << 32, 12345, 0                    # (user 1's only column has weight)
    lists.append(np.nonzero(q > 0)[0])                           # 6: every column that has weight, not every column
    assert 0 < len(lists[6]) < V and 0.15 < (q == 0).mean() < 0.5
    cum_np, ex_np = _tables_of(q, lists)
    assert cum_np[-1] > 1 << 32
    ptr, cols = _csr(lists, dev)
    cum, ex_cum = torch.from_numpy(cum_np).to(dev), torch.from_numpy(ex_np).to(dev)
    col2item_np = (rng.permutation(V) * 2 + 1).astype(np.int32)               # not the identity
    col2item = torch.from_numpy(col2item_np).to(dev)
    B = 4096
    users = rng.choice(np.asarray([0, 1, 2, 3, 4, 5, 6, -1, 99], dtype=np.int32), size=B)   # -1 / 99: out of range
    users_d = torch.from_numpy(users).to(dev)
    seed, step = 5, 3
    args = (users_d, ptr, cols, ex_cum, cum, V)
    items, mass, look = _draw_w(*args, col2item, seed, step, 0, dev)
    M = [eligible_mass(cum_np, l) for l in lists]
    assert M[2] == 0 and M[6] == 0 and M[1] == 1 << 32 and min(M[k] for k in (0, 3, 4, 5)) > 0
    for r in range(B):
        k = users[r] if 0 <= users[r] < len(lists) else 0
        if M[k] == 0:
            assert items[r] == -1 and mass[r] == -1 and look[r] == col2item_np[0]
            continue
        t = int(mass[r])
        assert 0 <= t < M[k]
        col = brute(cum_np, lists[k], t)
        assert col not in set(lists[k].tolist()) and q[col] > 0
        assert items[r] == col2item_np[col] == look[r], r
        assert t == (draw_key(seed, step, r) * M[k]) >> 64, r                # the RNG, in Python integers
    assert (items[users == 1] == col2item_np[17]).all()
    assert len(set(items[users == 3].tolist())) > 10
    # the same (seed, step, counter) -> the same draw; the device counter and the host offset add up
    np.testing.assert_array_equal(_draw_w(*args, col2item, seed, step, 0, dev)[0], items)
    np.testing.assert_array_equal(_draw_w(*args, col2item, seed, None, 3, dev)[0], items)
    np.testing.assert_array_equal(_draw_w(*args, col2item, seed, 1, 2, dev)[0], items)
    # another counter, another seed: more than half the rows change
    assert (_draw_w(*args, col2item, seed, 4, 0, dev)[0] != items).mean() > 0.5
    assert (_draw_w(*args, col2item, seed + 1, step, 0, dev)[0] != items).mean() > 0.5
    # without col2item the columns themselves come back
    plain, pmass, plook = _draw_w(*args, None, seed, step, 0, dev)
    np.testing.assert_array_equal(pmass, mass)
    live = items >= 0
    np.testing.assert_array_equal(col2item_np[plain[live]], items[live])
    assert (plain[~live] == -1).all() and (plook[~live] == 0).all()


# ------------------------------------------------------------------ 2. deep searches
def test_weighted_draw_with_long_lists_and_a_large_vocabulary(dev):
    import torch
    V, B = 100003, 2048
    rng = np.random.default_rng(3)
    q = rng.integers(0, 1 << 32, size=V).astype(np.int64)
    q[rng.choice(V, 500, replace=False)] = 0
    lists = [np.zeros(0, dtype=np.int64), np.sort(rng.choice(V, 1000, replace=False)),
             np.sort(rng.choice(V, 99990, replace=False))]
    cum_np, ex_np = _tables_of(q, lists)
    ptr, cols = _csr(lists, dev)
    users = rng.integers(0, 3, size=B).astype(np.int32)
    items, mass, _ = _draw_w(torch.from_numpy(users).to(dev), ptr, cols, torch.from_numpy(ex_np).to(dev),
                             torch.from_numpy(cum_np).to(dev), V, None, 11, 2, 0, dev)
    for k, lst in enumerate(lists):
        rows = np.nonzero(users == k)[0]
        assert len(rows) > 500
        masked = q.copy()
        masked[lst] = 0
        running = np.cumsum(masked)
        M = int(running[-1])
        assert M == eligible_mass(cum_np, lst) and M > 0
        t = mass[rows]
        assert (t >= 0).all() and (t < M).all()
        want = np.searchsorted(running, t, side='right')                      # the masked cumulative sum, vectorised
        np.testing.assert_array_equal(items[rows], want)
        assert not np.isin(items[rows], lst).any() and (q[items[rows]] > 0).all()
        for r in rows[:16]:
            assert int(mass[r]) == (draw_key(11, 2, int(r)) * M) >> 64
        if k == 2:                                                            # 13 columns are left
            assert len(np.setdiff1d(np.arange(V), lst)) == 13
            assert len(set(items[rows].tolist())) > 6


# ------------------------------------------------------------------ 3. distribution
@pytest.mark.parametrize("power,smooth", [(0.75, 1.0), (1.0, 0.0), (0.0, 1.0)])
def test_weighted_draw_follows_the_weights(dev, power, smooth):
    """Pearson's statistic of 4 x 8192 draws over the live columns (eligible and with weight) stays below the mean
    plus six standard deviations of chi-square with (live - 1) degrees of freedom; the expected cell counts come from
    the integer weights of pair_draw_tables."""
    import torch
    from arx.utils.prepare_train import pair_draw_tables
    V = V_DRAW
    rng = np.random.default_rng(1)
    counts = rng.integers(0, 200, V)
    excluded = np.sort(rng.choice(V, 13, replace=False))
    counts[np.setdiff1d(np.arange(V), excluded)[[3, 20]]] = 0                 # two eligible counts zeroed
    ptr_np, cols_np = np.asarray([0, 13]), excluded
    cum_np, ex_np = pair_draw_tables(counts, power, smooth, ptr_np, cols_np)
    q = np.diff(cum_np)
    live = np.setdiff1d(np.nonzero(q > 0)[0], excluded)
    n_live = 37 if smooth > 0 else int((counts[np.setdiff1d(np.arange(V), excluded)] > 0).sum())
    assert len(live) == n_live and n_live >= 34
    ptr, cols = _csr([excluded], dev)
    cum, ex_cum = torch.from_numpy(cum_np).to(dev), torch.from_numpy(ex_np).to(dev)
    users_d = torch.zeros((8192,), dtype=torch.int32, device=dev)
    hits = np.zeros(V)
    for counter in range(4):
        items, _, _ = _draw_w(users_d, ptr, cols, ex_cum, cum, V, None, 9, counter, 0, dev)
        hits += np.bincount(items, minlength=V)
    n = hits.sum()
    assert n == 4 * 8192
    assert hits[excluded].sum() == 0 and hits[q == 0].sum() == 0              # no excluded and no dead column
    expect = n * q[live] / q[live].sum()
    chi2 = float(((hits[live] - expect) ** 2 / expect).sum())
    df = n_live - 1
    print('power %g smooth %g: chi2 = %.2f, bound %.2f, smallest expected cell %.1f'
          % (power, smooth, chi2, df + 6 * np.sqrt(2 * df), expect.min()))
    assert chi2 < df + 6 * np.sqrt(2 * df)


# ------------------------------------------------------------------ 5. the single-GPU model
def test_model_draws_weighted_negatives_inside_the_captured_step(dev):
    import torch
    from arx import ops
    B, d = 64, 32
    syn, model, _ = _build_pair(CFG_ID, 'bpr', d, B, seed=4, use_graph=True)
    l2i = np.asarray(syn.logit_ind2item_ind)
    m = model.att_emb
    rng = np.random.default_rng(2)
    unseen = np.setdiff1d(l2i, syn.pos_items)
    assert len(unseen) > 2
    everywhere, other = int(np.intersect1d(l2i, syn.pos_items)[0]), int(unseen[0])
    counts = np.zeros(syn.n_items + 1, dtype=np.int64)
    counts[everywhere], counts[other] = 5, 2                                  # weight on exactly two items
    hist = {u: its + [everywhere] for u, its in syn.positives_dict().items()}
    u_full = 7
    hist[u_full] = l2i.tolist()                                               # this user has seen everything
    model.prepare_pair_negatives(hist, seed=3, power=1.0, smooth=0.0, counts=counts)
    urow = int(np.asarray(syn.u_attr.features_cat[0])[u_full])
    graph = None
    for step in range(6):
        users, pos = syn.sample_batch(B, rng)
        users[users == u_full] = u_full + 1
        users[0] = u_full
        urow_before = m.get_params()['userembed_cat_0'][urow].copy()
        loss = model.step(None, list(users), list(pos), None)
        plan = model._plan('train_draw')
        assert np.isfinite(loss)
        ids = m.neg_draw.value.cpu().numpy()
        fed = m.i_indices['neg'].value.cpu().numpy()
        assert ids[0] == -1 and (ids[1:] == other).all(), step               # the one item with weight left
        assert fed[0] == l2i[0] and (fed[1:] == other).all()
        assert float(model.batch_loss.value[0].item()) == 0.0                 # the void row: no loss,
        np.testing.assert_array_equal(m.get_params()['userembed_cat_0'][urow], urow_before)   # its user untouched
        if step == 1:
            graph = plan.graph
            assert graph is not None
        if step > 1:
            assert plan.graph is graph                                        # one capture
    # the unigram rule over the default counts: smooth 0 never draws an item nobody has seen
    hist = syn.positives_dict()
    model.prepare_pair_negatives(hist, seed=5, power=0.75, smooth=0.0)
    assert 'train_draw' not in model._plans
    seen_items = set(syn.pos_items.tolist())
    prev = None
    for step in range(3):
        users, pos = syn.sample_batch(B, rng)
        c0 = int(m.neg_draw.counter.item())
        model.step(None, list(users), list(pos), None)
        ids = m.neg_draw.value.cpu().numpy()
        assert (ids >= 0).all()
        for r in range(B):
            assert ids[r] in seen_items and ids[r] not in set(hist[int(users[r])]), (step, r)
        # ... and is the export itself, on the model's tables, seed and counter
        ptr, cols, c2i, ex_cum, cum = m._pair_lists
        direct = torch.zeros(B, dtype=torch.int32, device=dev)
        ops.neg_draw_weighted(m.u_indices['input'].value, ptr, cols, ex_cum, cum, m.logit_size, c2i, 5, None, c0,
                              direct)
        np.testing.assert_array_equal(direct.cpu().numpy(), ids)
        if prev is not None:
            assert (ids != prev).mean() > 0.5                                 # a replay draws anew
        prev = ids
    # forward_only draws through the same path and updates nothing
    p0 = m.get_params()
    c0 = int(m.neg_draw.counter.item())
    e = model.step(None, list(users), list(pos), None, forward_only=True)
    assert np.isfinite(e) and int(m.neg_draw.counter.item()) == c0 + 1
    for k, v in m.get_params().items():
        np.testing.assert_array_equal(v, p0[k], err_msg=k)
    # without power the model is back on the uniform draw
    model.prepare_pair_negatives(hist, seed=6)
    assert 'train_draw' not in model._plans and m._pair_lists[3] is None and m._pair_lists[4] is None
    c0 = int(m.neg_draw.counter.item())
    model.step(None, list(users), list(pos), None)
    ptr, cols, c2i = m._pair_lists[:3]
    direct = torch.zeros(B, dtype=torch.int32, device=dev)
    ops.neg_draw_uniform(m.u_indices['input'].value, ptr, cols, m.logit_size, c2i, 6, None, c0, direct)
    np.testing.assert_array_equal(direct.cpu().numpy(), m.neg_draw.value.cpu().numpy())


# ------------------------------------------------------------------ 6. the sharded model, world 1
def _group(dev, port):
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    return dist


def test_sharded_model_draws_weighted_negatives(dev):
    import torch
    from arx import ops
    from arx.dist import ShardedHMF
    from arx.utils.synthetic import SyntheticHMF
    dist = _group(dev, 29761)
    try:
        n_users, n_items, d, B = 100, 64, 32, 32
        syn = SyntheticHMF(n_users=n_users, n_items=n_items, seed=1, permute_logits=False, n_pos=8)
        params = syn.glorot_params(d, seed=2, scale=0.5)
        tables = {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
                  'item_bias': params['item_bias_cat_0'][2:]}
        lists = [set(syn.pos_items[syn.pos_ptr[u]:syn.pos_ptr[u + 1]].tolist()) for u in range(n_users)]

        def build(seed):
            mdl = ShardedHMF(n_users, n_items, d, B, 0, 0.5, 0, 1, dev, tables=tables, loss='bpr', seed=seed)
            ptr = np.concatenate([syn.pos_ptr[:n_users + 1], [syn.pos_ptr[n_users]]]).astype(np.int32)
            mdl.set_positives(ptr, syn.pos_items)
            mdl.prepare_pair_negatives(power=0.75)
            return mdl
        model = build(3)
        rng = np.random.default_rng(2)
        users = rng.integers(0, n_users, size=B).astype(np.int32)
        pos = rng.integers(0, n_items, size=B).astype(np.int32)
        ex_cum, cum = model._neg_tables
        assert cum.dtype == torch.int64 and cum.shape[0] == n_items + 1 and int(cum[0].item()) == 0
        seq = []
        for step in range(3):
            n0 = model.n_draws
            route = model.prepare_route(users, pos)
            ng = route['neg_items'].cpu().numpy()
            assert (ng >= 0).all() and ng.max() < n_items and model.n_draws == n0 + 1
            assert all(int(ng[r]) not in lists[int(users[r])] for r in range(B))
            direct = torch.zeros(B, dtype=torch.int32, device=dev)
            ops.neg_draw_weighted(route['urows'], model._neg_csr[0], model._neg_csr[1], ex_cum, cum, n_items, None,
                                  model.seed * 1000003 + model.rank, None, n0, direct)
            np.testing.assert_array_equal(direct.cpu().numpy(), ng)
            seq.append((route, ng))
        assert (seq[0][1] != seq[1][1]).any()
        twin = build(3)
        for step in range(3):
            np.testing.assert_array_equal(twin.prepare_route(users, pos)['neg_items'].cpu().numpy(), seq[step][1])
        assert (build(4).prepare_route(users, pos)['neg_items'].cpu().numpy() != seq[0][1]).mean() > 0.5
        # the route behind the draw is intact: one step with the drawn ids against BPR in fp64
        ref = PairRef(tables, 0.5)
        route, ng = seq[2]
        r = ref.step(users, pos, ng, 'bpr')
        model.step(route)
        np.testing.assert_allclose(float(model.read_loss().item()), r['loss'], rtol=RTOL)
        np.testing.assert_allclose(model.pos_score.cpu().numpy(), r['ps'], rtol=RTOL, atol=1e-5)
        np.testing.assert_allclose(model.neg_score.cpu().numpy(), r['ns'], rtol=RTOL, atol=1e-5)
        ref.compare(model.gather_global_tables(slots=True), rtol=RTOL, atol=ATOL)
    finally:
        dist.destroy_process_group()
