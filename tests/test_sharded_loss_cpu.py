"""The `loss` argument of the row-sharded models (arx.dist.ShardedHMF, ShardedHMFBags, ShardedHMFRepTokens) without a
GPU: gloo ranks over the numpy compute double (tests/numpy_backend_pair.py).

  'bpr' / 'bpr-hinge'  pair steps at worlds 2, 3 and 4 against BPR on the global batch in fp64 (PairRef): the slot
                       route, R = 0 ranks, a growing receive capacity, an item that is a positive on one rank and a
                       negative on another, one void row; the negatives drawn by the model; checkpoints
  'mce'                world 2 on all three classes (both exchanges of the id-only one) against the oracle's 'mce'
  constructor checks, and the argument validation of arx_pair_loss_slots (no device is touched)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

N_USERS, N_ITEMS, D, B_LOC, LR = 60, 90, 16, 8, 0.5
KINDS = ('bpr', 'bpr-hinge')
PAIR_SEED = {'bpr': 5, 'bpr-hinge': 5}          # (hinge: no row of any step within 1e-4 of the kink, asserted below)


def _init(rank, world, port):
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _tables():
    from arx.utils.synthetic import SyntheticHMF
    syn = SyntheticHMF(n_users=N_USERS, n_items=N_ITEMS, seed=1, permute_logits=False, n_pos=6)
    params = syn.glorot_params(D, seed=2, scale=0.5)
    return syn, params, {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
                         'item_bias': params['item_bias_cat_0'][2:]}


def pair_batches(world, seed, n_steps=5):
    """The global batches of the pair test, per step ([users], [positives], [negatives]) of every rank, and the
    (step, rank, row) of the void row.  Every step: a duplicate user, an item that is a positive twice, an item that
    is the positive of a row on rank 0 and the negative of a row on rank 1.  Step 1: one void row whose user no other
    row names.  Step 3: every requested item lives on rank 0 (R = 0 elsewhere, and rank 0's receive capacity grows).
    Step 4: three quarters of the positives on the last owner."""
    rng = np.random.default_rng(seed)
    out = []
    void = (1, world - 1, 6)
    for step in range(n_steps):
        gu, gi, gn = [], [], []
        for g in range(world):
            gu.append(rng.integers(0, len(np.arange(g, N_USERS, world)), size=B_LOC) * world + g)
            gi.append(rng.integers(0, N_ITEMS, size=B_LOC))
            gn.append(rng.integers(0, N_ITEMS, size=B_LOC))
        if step == 3:
            for g in range(world):
                gi[g] = rng.integers(0, N_ITEMS // world, size=B_LOC) * world
                gn[g] = rng.integers(0, N_ITEMS // world, size=B_LOC) * world
        if step == 4:
            k = (3 * B_LOC) // 4
            for g in range(world):
                gi[g][:k] = rng.integers(0, N_ITEMS // world - 1, size=k) * world + (world - 1)
        gu[0][1] = gu[0][0]
        gi[1][2] = gi[1][3]
        gn[1][4] = gi[0][5]
        for g in range(world):                       # (no row with its positive as its negative)
            same = gn[g] == gi[g]
            gn[g][same] = (gi[g][same] + world) % N_ITEMS
        if step == void[0]:
            _, g, r = void
            gn[g][r] = -1
            free = np.setdiff1d(np.arange(g, N_USERS, world), np.concatenate(gu))
            gu[g][r] = free[0]
        out.append((gu, gi, gn))
    return out, void


def _check_batches(world, batches, void):
    gu, gi, gn = batches[0]
    assert gu[0][1] == gu[0][0] and gi[1][2] == gi[1][3] and gn[1][4] == gi[0][5]
    s, g, r = void
    assert batches[s][2][g][r] == -1 and (np.concatenate(batches[s][0]) == batches[s][0][g][r]).sum() == 1
    assert all((np.concatenate(batches[3][k]) % world == 0).all() for k in (1, 2))


@pytest.mark.parametrize("world", [2, 3, 4])
def test_hinge_reference_stays_clear_of_the_kink(world):
    """fp32 and fp64 may branch differently near 1 + x = 0: on the fp64 reference no row of any step of the pair test
    lies within 1e-4 of it (the seed is chosen so; no row is left out)."""
    from numpy_backend_pair import PairRef
    _, _, tables = _tables()
    batches, void = pair_batches(world, PAIR_SEED['bpr-hinge'])
    _check_batches(world, batches, void)
    ref = PairRef(tables, LR)
    for gu, gi, gn in batches:
        r = ref.step(np.concatenate(gu), np.concatenate(gi), np.concatenate(gn), 'bpr-hinge')
        assert np.abs(1.0 + r['x'][r['live']]).min() > 1e-4


def _pair_worker(rank, world, port, out_dir, kind):
    dist = _init(rank, world, port)
    from arx.dist import ShardedHMF
    from numpy_backend_pair import NumpyPairBackend, PairRef
    _, _, tables = _tables()
    model = ShardedHMF(N_USERS, N_ITEMS, D, B_LOC, 0, LR, rank, world, 'cpu', backend=NumpyPairBackend(),
                       tables=tables, loss=kind)
    ref = PairRef(tables, LR)
    batches, void = pair_batches(world, PAIR_SEED[kind])
    padded = grew = after_growth = False
    for step, (gu, gi, gn) in enumerate(batches):
        users, pos, neg = np.concatenate(gu), np.concatenate(gi), np.concatenate(gn)
        r = ref.step(users, pos, neg, kind)
        if kind == 'bpr-hinge':
            assert np.abs(1.0 + r['x'][r['live']]).min() > 1e-4, step
        is_void = step == void[0] and rank == void[1]
        if is_void:
            urow = int(gu[rank][void[2]]) // world
            before = (model.E_user[urow].clone(), model.A_user[urow].clone())
        cap_r0 = model.cap_r
        model.step(gu[rank].astype(np.int32), gi[rank].astype(np.int32), gn[rank].astype(np.int32))   # no set_pool
        l_got = float(model.read_loss().item())
        assert abs(l_got - r['loss']) <= 1e-5 * abs(r['loss']), (step, l_got, r['loss'])
        assert abs(model.read_auc() - r['auc']) <= 1e-6, (step, model.read_auc(), r['auc'])
        mine = slice(rank * B_LOC, (rank + 1) * B_LOC)                      # this rank's rows, in the caller's order
        np.testing.assert_allclose(model.pos_score.numpy(), r['ps'][mine], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(model.neg_score.numpy(), r['ns'][mine], rtol=1e-4, atol=1e-6)
        if is_void:
            import torch
            assert float(model.bl[void[2]]) == 0.0
            assert torch.equal(model.E_user[urow], before[0]) and torch.equal(model.A_user[urow], before[1])
        req = np.concatenate([pos, neg[neg >= 0]])
        padded |= int((req % world == rank).sum()) < model.cap_r
        after_growth |= grew
        grew |= model.cap_r > cap_r0
        if step == 3 and rank != 0:
            assert int((req % world == rank).sum()) == 0
    seen = [None] * world
    dist.all_gather_object(seen, (bool(padded), bool(after_growth)))
    assert any(p for p, _ in seen), "no rank saw a batch with R < cap_r"
    assert any(g for _, g in seen), "no step followed a growth of cap_r"
    ref.compare(model.gather_global_tables(slots=True), rtol=1e-4, atol=1e-6)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("world", [2, 3, 4])
def test_sharded_pair_steps_match_fp64_gloo(tmp_path, world, kind):
    import torch.multiprocessing as mp
    port = 28100 + (os.getpid() % 400) + 10 * world + KINDS.index(kind)
    mp.spawn(_pair_worker, args=(world, port, str(tmp_path), kind), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(world))


# ------------------------------------------------------------------------------------------------ drawn negatives
def _draw_model(rank, world, seed, full_user):
    """A 'bpr' model whose lists are the synthetic positives -- unsorted, one entry doubled -- and, for `full_user`,
    every item."""
    from arx.dist import ShardedHMF
    from numpy_backend_pair import NumpyPairBackend
    syn, _, tables = _tables()
    model = ShardedHMF(N_USERS, N_ITEMS, D, B_LOC, 0, LR, rank, world, 'cpu', backend=NumpyPairBackend(),
                       tables=tables, loss='bpr', seed=seed)
    own = np.arange(rank, N_USERS, world)
    ptr, items, lists = np.zeros(len(own) + 2, dtype=np.int32), [], {}
    for k, u in enumerate(own):
        its = syn.pos_items[syn.pos_ptr[u]:syn.pos_ptr[u + 1]].tolist()
        its = list(range(N_ITEMS)) if u == full_user else its[::-1] + its[:1]
        lists[int(u)] = set(its)
        items.extend(its)
        ptr[k + 1] = len(items)
    ptr[-1] = ptr[-2]
    model.set_positives(ptr, np.asarray(items, dtype=np.int32))
    return syn, model, lists


def _draw_worker(rank, world, port, out_dir):
    _init(rank, world, port)
    full_user = rank + 2 * world                       # a user of this rank whose list is every item
    syn, model, lists = _draw_model(rank, world, 7, full_user)
    rng = np.random.default_rng(20 + rank)
    own = np.arange(rank, N_USERS, world)

    def batch():
        u = rng.choice(own, size=B_LOC)
        u[u == full_user] = own[0]
        u[3] = full_user
        return u.astype(np.int32), rng.integers(0, N_ITEMS, size=B_LOC).astype(np.int32)
    u, it = batch()
    with pytest.raises(RuntimeError, match="prepare_pair_negatives"):
        model.prepare_route(u, it)
    model.prepare_pair_negatives()
    seq = []
    for step in range(3):
        route = model.prepare_route(u, it)             # the same batch: only the draw counter moves
        ng = route['neg_items'].numpy()
        assert ng[3] == -1 and (np.delete(ng, 3) >= 0).all() and ng.max() < N_ITEMS
        assert all(int(ng[r]) not in lists[int(u[r])] for r in range(B_LOC) if r != 3)
        assert route['slots'].numpy()[B_LOC + 3] == -1 and route['n_req'] == 2 * B_LOC - 1
        model.step(route)
        assert np.isfinite(float(model.read_loss().item())) and float(model.bl[3]) == 0.0
        seq.append(ng.copy())
    assert (seq[0] != seq[1]).any() and (seq[1] != seq[2]).any()          # a fresh draw per route
    # the same seed: the same sequence
    _, twin, _ = _draw_model(rank, world, 7, full_user)
    twin.prepare_pair_negatives()
    for step in range(3):
        np.testing.assert_array_equal(twin.prepare_route(u, it)['neg_items'].numpy(), seq[step])
    _, other, _ = _draw_model(rank, world, 8, full_user)
    other.prepare_pair_negatives()
    assert (other.prepare_route(u, it)['neg_items'].numpy() != seq[0]).any()
    # save / restore: the sequence goes on where it stopped
    path = os.path.join(out_dir, "ck")
    model.saver.save(None, path)
    nxt = model.prepare_route(u, it)['neg_items'].numpy().copy()
    _, fresh, _ = _draw_model(rank, world, 7, full_user)
    fresh.prepare_pair_negatives()
    fresh.saver.restore(None, path)
    assert fresh.n_draws == 3 and fresh.steps == 3
    np.testing.assert_array_equal(fresh.prepare_route(u, it)['neg_items'].numpy(), nxt)
    # a manifest from before the loss choice has neither scalar: it restores as before; and the tables of a 'bpr'
    # run restore into a model that trains another loss
    import torch.distributed as dist
    dist.barrier()
    if rank == 0:
        mf = path + '.manifest.json'
        man = json.load(open(mf))
        assert man['scalars']['loss'] == 'bpr' and man['scalars']['n_draws'] == 3
        del man['scalars']['loss'], man['scalars']['n_draws']
        json.dump(man, open(mf, 'w'))
    dist.barrier()
    from arx.dist import ShardedHMF
    from numpy_backend_pair import NumpyPairBackend
    old = ShardedHMF(N_USERS, N_ITEMS, D, B_LOC, 16, LR, rank, world, 'cpu', backend=NumpyPairBackend(), loss='mce')
    old.saver.restore(None, path)
    assert old.steps == 3 and old.n_draws == 0
    assert np.array_equal(old.E_item.numpy(), model.E_item.numpy())
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_sharded_pair_model_draws_its_negatives_gloo(tmp_path):
    import torch.multiprocessing as mp
    port = 28600 + (os.getpid() % 400)
    mp.spawn(_draw_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))


def test_prepare_pair_negatives_sorts_and_checks_the_lists(tmp_path):
    import torch.multiprocessing as mp
    port = 28650 + (os.getpid() % 400)
    mp.spawn(_lists_worker, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    assert os.path.exists(tmp_path / "ok0")


def _lists_worker(rank, world, port, out_dir):
    _init(rank, world, port)
    _, model, lists = _draw_model(0, 1, 0, 5)
    model.prepare_pair_negatives()
    ptr, cols = (t.numpy() for t in model._neg_csr)
    for u in range(N_USERS):
        lst = cols[ptr[u]:ptr[u + 1]]
        assert (np.diff(lst) > 0).all() and set(lst.tolist()) == lists[u]
    model.set_positives(np.asarray([0, 1] + [1] * N_USERS, dtype=np.int32), np.asarray([N_ITEMS], dtype=np.int32))
    with pytest.raises(ValueError, match="item ids"):
        model.prepare_pair_negatives()
    with open(os.path.join(out_dir, "ok0"), "w") as f:
        f.write("ok")
    import torch.distributed as dist
    dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------- 'mce'
def _mce_worker(rank, world, port, out_dir, exchange):
    """tests/test_dist_cpu.py's 'mw' worker -- its shapes, pools, batches and steps -- with loss='mce'."""
    dist = _init(rank, world, port)
    from arx.dist import ShardedHMF
    from numpy_backend_pair import NumpyPairBackend
    from oracle import ref_graph as rg
    S = 16
    syn, params, tables = _tables()
    model = ShardedHMF(N_USERS, N_ITEMS, D, B_LOC, S, LR, rank, world, 'cpu', backend=NumpyPairBackend(),
                       tables=tables, exchange=exchange, loss='mce')
    own_users = np.arange(rank, N_USERS, world)
    ptr, items = np.zeros(len(own_users) + 2, dtype=np.int32), []
    for k, u in enumerate(own_users):
        items.extend(syn.pos_items[syn.pos_ptr[u]:syn.pos_ptr[u + 1]].tolist())
        ptr[k + 1] = len(items)
    ptr[-1] = ptr[-2]
    model.set_positives(ptr, np.asarray(items, dtype=np.int32))
    B = B_LOC * world
    ref = rg.RefLatentProductModel(D, B, LR, syn.u_attr, syn.i_attr, syn.item_ind2logit_ind_dict(),
                                   syn.logit_ind2item_ind, loss_function='mce', n_sampled=S, params=params,
                                   dtype=np.float64)
    pos = syn.positives_dict()
    ref.prepare_warp(pos, pos)
    rng = np.random.default_rng(5)
    for step in range(5):
        pool = None
        if step % 2 == 0:
            if step == 0:
                pool = rng.choice(N_ITEMS, size=S, replace=False)
            elif step == 2:
                pool = rng.choice(np.arange(world - 1, N_ITEMS, world), size=S, replace=False)
            else:
                hot = rng.choice(np.arange(0, N_ITEMS, world), size=(3 * S) // 4, replace=False)
                rest = rng.choice(np.setdiff1d(np.arange(N_ITEMS), hot), size=S - len(hot), replace=False)
                pool = rng.permutation(np.concatenate([hot, rest]))
            pool = pool.astype(np.int32)
            id2idx = {int(v): i for i, v in enumerate(pool)}
            model.set_pool(pool)
        gu, gi = [], []
        for g in range(world):
            users = rng.integers(0, len(np.arange(g, N_USERS, world)), size=B_LOC) * world + g
            gu.append(users)
            gi.append(syn.pos_items[syn.pos_ptr[users] + rng.integers(0, syn.n_pos, size=B_LOC)])
        gu[0][1] = gu[0][0]
        gi[1][2] = gi[1][3]
        if step == 0:
            gi[0][0] = pool[np.nonzero(pool % world == 1)[0][0]]
        if step == 3:
            for g in range(world):
                gi[g] = (rng.integers(0, N_ITEMS // world, size=B_LOC) * world).astype(gi[g].dtype)
        l_ref = ref.step(np.concatenate(gu).tolist(), np.concatenate(gi).tolist(), pool, id2idx, loss='mce')
        model.step(gu[rank].astype(np.int32), gi[rank].astype(np.int32))
        l_got = float(model.read_loss().item())
        assert abs(l_got - l_ref) <= 1e-5 * abs(l_ref), (step, l_got, l_ref)
    got = model.gather_global_tables()
    P = ref.att_emb.params
    np.testing.assert_allclose(got['user'], P['userembed_cat_0'][2:], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(got['item'], P['itemembed_cat_0'][2:], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(got['item_bias'], P['item_bias_cat_0'][2:, 0], rtol=1e-4, atol=1e-6)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("exchange", ['rows', 'logits'])
def test_sharded_mce_matches_oracle_gloo(tmp_path, exchange):
    import torch.multiprocessing as mp
    port = 28700 + (os.getpid() % 400) + (exchange == 'logits')
    mp.spawn(_mce_worker, args=(2, port, str(tmp_path), exchange), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))


def _mce_bags_worker(rank, world, port, out_dir, replicated):
    """tests/test_dist_cpu.py's HET worker with loss='mce'."""
    dist = _init(rank, world, port)
    from arx.dist import ShardedHMFBags, ShardedHMFRepTokens
    from arx.utils.synthetic import SyntheticHMF
    from numpy_backend_pair import NumpyPairBackend
    from oracle import ref_graph as rg
    S, V = 16, 37
    syn = SyntheticHMF(n_users=N_USERS, n_items=N_ITEMS, seed=1, permute_logits=False, n_pos=6,
                       item_mulhot=True, mulhot_vocab=V, avg_len=4, max_len=9)
    ia = syn.i_attr
    n_tok = ia._embedding_classes_list_mulhot[0]
    params = syn.glorot_params(D, seed=2, scale=0.5)
    tables = {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
              'item_bias': params['item_bias_cat_0'][2:], 'token': params['itemembed_mulhot_0'],
              'token_bias': params['item_bias_mulhot_0']}
    bags = (np.asarray(ia.features_mulhot[0]), np.asarray(ia.mulhot_starts[0]), np.asarray(ia.mulhot_lengths[0]))
    cls = ShardedHMFRepTokens if replicated else ShardedHMFBags
    model = cls(N_USERS, N_ITEMS, D, B_LOC, S, LR, rank, world, 'cpu', bags, n_tok, backend=NumpyPairBackend(),
                tables=tables, loss='mce')
    own_users = np.arange(rank, N_USERS, world)
    ptr, items = np.zeros(len(own_users) + 2, dtype=np.int32), []
    for k, u in enumerate(own_users):
        items.extend(syn.pos_items[syn.pos_ptr[u]:syn.pos_ptr[u + 1]].tolist())
        ptr[k + 1] = len(items)
    ptr[-1] = ptr[-2]
    model.set_positives(ptr, np.asarray(items, dtype=np.int32))
    B = B_LOC * world
    ref = rg.RefLatentProductModel(D, B, LR, syn.u_attr, syn.i_attr, syn.item_ind2logit_ind_dict(),
                                   syn.logit_ind2item_ind, loss_function='mce', n_sampled=S, params=params,
                                   dtype=np.float64)
    pos = syn.positives_dict()
    ref.prepare_warp(pos, pos)
    rng = np.random.default_rng(5)
    for step in range(4):
        pool = None
        if step % 2 == 0:
            blocks = [rng.choice(np.arange(g, N_ITEMS, world), size=S // world + (1 if g < S % world else 0),
                                 replace=False) for g in range(world)]
            pool = np.concatenate(blocks).astype(np.int32)
            id2idx = {int(v): i for i, v in enumerate(pool)}
            model.set_pool(pool)
        gu, gi = [], []
        for g in range(world):
            users = rng.integers(0, len(np.arange(g, N_USERS, world)), size=B_LOC) * world + g
            gu.append(users)
            gi.append(syn.pos_items[syn.pos_ptr[users] + rng.integers(0, syn.n_pos, size=B_LOC)])
        gu[0][1] = gu[0][0]
        gi[1][2] = gi[1][3]
        if step == 0:
            gi[0][0] = pool[S // world]
        if step == 3:
            for g in range(world):
                gi[g] = (rng.integers(0, N_ITEMS // world, size=B_LOC) * world).astype(gi[g].dtype)
        l_ref = ref.step(np.concatenate(gu).tolist(), np.concatenate(gi).tolist(), pool, id2idx, loss='mce')
        model.step(gu[rank].astype(np.int32), gi[rank].astype(np.int32))
        l_got = float(model.read_loss().item())
        assert abs(l_got - l_ref) <= 1e-5 * abs(l_ref), (step, l_got, l_ref)
    got = model.gather_global_tables()
    P = ref.att_emb.params
    for name, want in (('user', P['userembed_cat_0'][2:]), ('item', P['itemembed_cat_0'][2:]),
                       ('item_bias', P['item_bias_cat_0'][2:, 0]), ('token', P['itemembed_mulhot_0']),
                       ('token_bias', P['item_bias_mulhot_0'][:, 0])):
        np.testing.assert_allclose(got[name], want, rtol=1e-4, atol=1e-6, err_msg=name)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("replicated", [False, True])
def test_sharded_het_mce_matches_oracle_gloo(tmp_path, replicated):
    import torch.multiprocessing as mp
    port = 28750 + (os.getpid() % 400) + int(replicated)
    mp.spawn(_mce_bags_worker, args=(2, port, str(tmp_path), replicated), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))


# ------------------------------------------------------------------------------------------ constructor, the export
def test_constructors_check_the_loss():
    """Refused before any buffer, backend or process group is touched."""
    from arx.dist import ShardedHMF, ShardedHMFBags, ShardedHMFRepTokens
    base = (N_USERS, N_ITEMS, D, B_LOC, 16, LR, 0, 1, 'cpu')
    bags = ((np.zeros(1, np.int32), np.zeros(N_ITEMS, np.int32), np.ones(N_ITEMS, np.int32)), 4)
    with pytest.raises(ValueError, match="loss"):
        ShardedHMF(*base, backend=object(), loss='warp')
    for cls in (ShardedHMFBags, ShardedHMFRepTokens):
        with pytest.raises(ValueError, match="loss"):
            cls(*base, *bags, backend=object(), loss='ce')
        for kind in KINDS:
            with pytest.raises(NotImplementedError, match="ShardedHMF"):
                cls(*base, *bags, backend=object(), loss=kind)
    for kind in KINDS:
        with pytest.raises(ValueError, match="logits"):
            ShardedHMF(*base, backend=object(), loss=kind, exchange='logits')


def test_pair_loss_slots_validates_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib
    EINVAL = -1

    def err():
        m = lib.arx_last_error()
        return m.decode() if m else ""
    P = 4096          # (pointers are only compared with NULL and checked for alignment before the first HIP call)

    def slots(U=P, R=P, pos=P, neg=P, B=8, d=64, kind=0, ldu=64, ldr=68, n_slots=16, dU=None, dR=None, lddr=68,
              out=P):
        return lib.arx_pair_loss_slots(U, ldu, R, ldr, n_slots, pos, neg, None, B, d, kind, 1.0, out, P, P, dU, ldu, 0,
                                       dR, lddr, None, None)
    for bad in (dict(U=None), dict(R=None), dict(pos=None), dict(neg=None), dict(out=None), dict(B=-1),
                dict(n_slots=-1), dict(B=1 << 31), dict(kind=2), dict(d=62), dict(d=260, ldu=260, ldr=264),
                dict(ldu=66), dict(ldr=64),                   # a packed row holds d + 4 floats
                dict(ldr=70), dict(U=P + 4), dict(R=P + 8), dict(dU=P), dict(dR=P),      # one gradient, not both
                dict(dU=P, dR=P, lddr=64), dict(dU=P + 4, dR=P)):
        assert slots(**bad) == EINVAL and "arx_pair_loss_slots" in err(), bad
    assert slots(d=62) == EINVAL and "d=62" in err()
    assert slots(B=0) == 0
    assert slots(B=0, dU=P, dR=P) == 0
