"""list_logprob on the row-sharded models, on the GPU (include/arx_list_logp_shard.h).

Kernel level: arx_list_logp_prepare_shard against the numpy statement of the header (tests/numpy_backend_list.py) for
W in {1, 2, 3} and every shard, against arx_list_logp_prepare at (1, 0) and against arx_picks_to_shard +
arx_sample_logp_sort over the merged clean list; arx_list_logp_merge_shards over a strided view of a packed buffer.
Model level: world 1 (an nccl group of one), two rank processes on the one GPU over gloo, ShardedW2V and
ShardedHetView -- a list recommend_sampled(return_logprob=True) drew itself comes back bit for bit, foreign lists with
every reason code against tests/list_logprob_oracle.py on the device's own logits within that oracle's tolerance."""
import os
import time

import numpy as np
import pytest

import list_logprob_oracle as LL
import tags_oracle as T
from numpy_backend_list import merge_shards, prepare_shard
from test_list_logprob_gpu import _check, _i32
from test_sharded_recommend_gpu import _histories, _init_world1, _shard_logits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V_G = 1000


# ---------------------------------------------------------------- 1. the two kernels
def _shard_filters(rng, B, V, W, s, on, n_ex=40):
    """-> (ex, tags) of shard s as numpy tuples in the kernels' conventions, or (None, None)"""
    if not on:
        return None, None
    keys = rng.permutation(B).astype(np.int32)
    keys[B // 2] = -1                                            # a row without a list
    rows = [sorted(set(rng.integers(0, V, n_ex).tolist())) for _ in range(B)]        # by key, global ids
    loc = [[c // W for c in row if c % W == s] for row in rows]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in loc])]).astype(np.int32)
    cols = np.array([c for x in loc for c in x] + [0], dtype=np.int32)
    tags = rng.integers(0, 16, V).astype(np.uint32)
    wa, wl = rng.integers(0, 16, B).astype(np.uint32), rng.integers(0, 4, B).astype(np.uint32)
    wa[::3] = 0
    return (keys, B, ptr, cols), (tags[s::W].copy().view(np.int32), wa.view(np.int32), wl.view(np.int32), B)


def _run_prepare_shard(dev, lists, V, W, s, ex, tags):
    import torch
    from arx import ops
    B, k = lists.shape
    out = [torch.full((B, k), -77, dtype=torch.int32, device=dev) for _ in range(4)]
    dex = (_i32(dev, ex[0]), ex[1], _i32(dev, ex[2]), _i32(dev, ex[3])) if ex is not None else None
    dtg = (_i32(dev, tags[0]), _i32(dev, tags[1]), _i32(dev, tags[2]), tags[3]) if tags is not None else None
    ops.list_logp_prepare_shard(_i32(dev, lists), V, W, s, dex, dtg, *out)
    return [t.cpu().numpy() for t in out], dex, dtg


@pytest.mark.parametrize("filt", [False, True], ids=["plain", "ex+tags"])
@pytest.mark.parametrize("k", [1, 64, 70, 1024])
def test_prepare_shard_against_the_header(dev, k, filt):
    """k = 70 puts a second slot on a lane, 1024 is the LDS bound; 37 rows: ten blocks of four waves."""
    import torch
    from arx import ops
    rng = np.random.default_rng(1000 + k)
    B = 37
    lists = rng.integers(-3, V_G + 3, size=(B, k))
    lists[rng.random((B, k)) < 0.1] = -1
    if k > 1:
        lists[:, k // 2] = lists[:, 0]                           # a repeat of whoever owns entry 0
    for W in (1, 2, 3):
        slabs = []
        sorted_of = {}
        for s in range(W):
            frng = np.random.default_rng(5)                      # (the same global filters for every shard)
            ex, tags = _shard_filters(frng, B, V_G, W, s, filt)
            got, dex, dtg = _run_prepare_shard(dev, lists, V_G, W, s, ex, tags)
            want = prepare_shard(lists, V_G, W, s, ex, tags)
            for g, w, name in zip(got, want, ("clean", "codes", "pk_cols", "pk_slot")):
                np.testing.assert_array_equal(g, w, err_msg="%s W %d s %d" % (name, W, s))
            slabs.append(got[1])
            sorted_of[s] = (got[2], got[3])
            if W == 1:                                           # (1, 0): arx_list_logp_prepare, bit for bit
                single = [torch.full((B, k), -77, dtype=torch.int32, device=dev) for _ in range(4)]
                ops.list_logp_prepare(_i32(dev, lists), V_G, dex, dtg, *single)
                for g, t in zip(got, single):
                    np.testing.assert_array_equal(g, t.cpu().numpy())
        # the owner's merge, then arx_picks_to_shard + arx_sample_logp_sort over the merged clean list
        codes = _i32(dev, np.stack(slabs))
        clean, why = (torch.empty((B, k), dtype=torch.int32, device=dev) for _ in range(2))
        ops.list_logp_merge_shards(_i32(dev, lists), V_G, codes, clean, why)
        wc, ww = merge_shards(lists, V_G, np.stack(slabs))
        np.testing.assert_array_equal(clean.cpu().numpy(), wc)
        np.testing.assert_array_equal(why.cpu().numpy(), ww)
        if not filt:                                             # the single-device rule's codes (NOSCORE: the stamp's)
            np.testing.assert_array_equal(ww, LL.why(np.zeros((B, V_G), dtype=np.float32), lists))
        for s in range(W):
            cols, pc, ps = (torch.empty((B, k), dtype=torch.int32, device=dev) for _ in range(3))
            ops.picks_to_shard(clean, W, s, cols)
            ops.sample_logp_sort(cols, pc, ps)
            np.testing.assert_array_equal(sorted_of[s][0], pc.cpu().numpy())
            np.testing.assert_array_equal(sorted_of[s][1], ps.cpu().numpy())


def test_prepare_shard_second_trip_of_the_row_loop(dev):
    """B = 4 * 8 * CU count + 5 rows at k = 3: the capped grid walks its rows twice."""
    import torch
    rng = np.random.default_rng(9)
    B, k, W, s = 4 * 8 * torch.cuda.get_device_properties(dev).multi_processor_count + 5, 3, 2, 1
    lists = rng.integers(-2, 40, size=(B, k))
    ex, tags = _shard_filters(np.random.default_rng(6), B, 40, W, s, True, n_ex=6)
    got, _, _ = _run_prepare_shard(dev, lists, 40, W, s, ex, tags)
    want = prepare_shard(lists, 40, W, s, ex, tags)
    assert set(want[1].ravel().tolist()) == set(range(6))
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_merge_shards_all_codes_from_a_packed_view(dev):
    """W = 3, the codes as int32 bits behind float columns of one packed buffer (the exchange's layout)."""
    import torch
    from arx import ops
    rng = np.random.default_rng(2)
    W, B, k, P, V = 3, 9, 11, 2, 50
    lists = rng.integers(0, V, size=(B, k))
    lists[:, 0], lists[:, 1], lists[:, 2] = -1, V, -9
    slabs = rng.integers(0, 7, size=(W, B, k)).astype(np.int32)          # whatever an owner says is passed on
    packed = torch.full((W, B, 2 * P + 2 * k), float('nan'), dtype=torch.float32, device=dev)
    view = packed.view(torch.int32)[:, :, 2 * P + k:]
    view.copy_(_i32(dev, slabs))
    clean, why = (torch.full((B, k), -77, dtype=torch.int32, device=dev) for _ in range(2))
    ops.list_logp_merge_shards(_i32(dev, lists), V, view, clean, why)
    wc, ww = merge_shards(lists, V, slabs)
    assert set(ww.ravel().tolist()) == set(range(7))
    np.testing.assert_array_equal(why.cpu().numpy(), ww)
    np.testing.assert_array_equal(clean.cpu().numpy(), wc)
    assert torch.isnan(packed[:, :, :2 * P + k]).all()                   # nothing else was touched


def test_shard_entries_return_einval_with_a_message(dev):
    import test_sharded_list_logprob_cpu as C
    C.test_shard_entries_validate_arguments_without_gpu()


# ---------------------------------------------------------------- 2. the models
def _foreign(rng, n, k, n_items, world, dead, ex_rows=None, bad_tag=None):
    """lists [n, k >= 14] with every reason code: slots 1 / 3 / 4 EMPTY and RANGE, 6 a REPEAT of slot 0, 7 a NOSCORE
    item and 8 its REPEAT, 9-10 excluded and 11-12 tag-failing items of the owners r and r + 1 (mod world); row 1 all
    -1; the rest random ids."""
    ls = np.stack([rng.permutation(n_items)[:k] for _ in range(n)])
    for r in range(n):
        ls[r, 1], ls[r, 3], ls[r, 4], ls[r, 6] = -1, n_items + r, -7, ls[r, 0]
        ls[r, 7] = ls[r, 8] = dead[r % len(dead)]
        for src, at in ((ex_rows, 9), (bad_tag, 11)):
            for j in range(2):
                mine = [c for c in src[r][:200] if c % world == (r + j) % world] if src is not None else []
                if mine:
                    ls[r, at + j] = mine[0]
    ls[1] = -1
    return ls


def _tables(n_users, n_items, d, dead, seed=3):
    import torch
    g = torch.Generator(device='cpu').manual_seed(seed)
    U = torch.randn(n_users, d, generator=g) * 0.3
    I = torch.randn(n_items, d, generator=g) * 0.3
    b = torch.randn(n_items, generator=g) * 0.1
    b[dead] = float('-inf')                                      # items that never score
    return U, I, b


def _filters(rng, users, n_items, dead, top):
    """tags, request words (user 2: nothing eligible), histories without the dead items, the tag-failing columns"""
    n = len(users)
    tags = T.random_tags(rng, n_items)
    tags[dead] = 0xffffffff
    want_any, want_all = T.random_words(rng, n, zero_every=7)
    want_all[2] = 0xffffffff
    ex = {u: [c for c in its if c not in dead] for u, its in _histories(rng, users, n_items, top=top).items()}
    ex_rows = [sorted(set(ex[int(u)])) for u in users]
    ok = T.eligible(tags, want_any, want_all)
    bad_tag = [[int(c) for c in np.nonzero(~ok[r])[0][:400] if c not in ex_rows[r]] for r in range(n)]
    return tags, want_any, want_all, ex, ex_rows, bad_tag


def _self_drawn(model, users, k, tau, seed, pre=(), **kw):
    """recommend_sampled(return_logprob=True)'s own list through list_logprob: logprob and values bit for bit."""
    from arx.utils.ope import list_weights
    head = (users,) + tuple(pre)                                 # (ShardedW2V: the context comes second)
    ids, v0, lp0 = model.recommend_sampled(*head, k, return_values=True, sample_temperature=tau, sample_seed=seed,
                                           return_logprob=True, **kw)
    lp1, v1, why = model.list_logprob(*head, ids, tau, return_values=True, return_why=True, **kw)
    ids, v0, lp0, lp1, v1, why = (t.cpu().numpy() for t in (ids, v0, lp0, lp1, v1, why))
    np.testing.assert_array_equal(lp1, lp0)
    np.testing.assert_array_equal(v1, v0)
    np.testing.assert_array_equal(why, np.where(ids >= 0, LL.OK, LL.EMPTY))
    assert (list_weights(lp1, lp0) == 1.0).all()
    return ids, v0, lp0


def _foreign_check(name, model, users, lists, tau, lg, filt, pre=(), **kw):
    args = (users,) + tuple(pre) + (lists, tau)
    lp, vals, why = (t.cpu().numpy() for t in model.list_logprob(*args, return_values=True, return_why=True, **kw))
    assert lp.shape == lists.shape and lp.dtype == np.float32 and why.dtype == np.int32
    _check(name, lg, lists, tau, filt, lp, vals, why)
    return lp, why


def test_sharded_list_logprob_world1(dev):
    """World 1, 100003 items (past the first chunk: the streaming mass pass runs), d 64, B_loc 64, k 30."""
    import torch
    import torch.distributed as dist
    from arx.dist import ShardedHMF
    _init_world1(dev, 29811)
    try:
        n_users, n_items, d, B_loc, k = 500, 100003, 64, 64, 30
        dead = [5, 70001, 99999]
        U, I, b = _tables(n_users, n_items, d, dead)
        model = ShardedHMF(n_users, n_items, d, B_loc, 64, 0.1, 0, 1, dev,
                           tables={'user': U.numpy(), 'item': I.numpy(), 'item_bias': b.numpy()})
        assert model.be.shard_mass_parts(B_loc, n_items, d) > 1
        rng = np.random.default_rng(4)
        users = rng.choice(n_users, size=B_loc - 5, replace=False)
        n = len(users)
        U_all = torch.zeros(B_loc, d, device=dev)
        U_all[:n] = U[torch.from_numpy(users)].to(dev)
        lg = _shard_logits(U_all, I.to(dev), b.to(dev), 1, np.arange(n), dev)
        tau = np.array([0.25, 1.0, 3.0], dtype=np.float32)[rng.integers(0, 3, n)]
        ids0, v0, lp0 = _self_drawn(model, users, k, tau, 11)
        assert (ids0 >= 0).all() and (lp0 < 0).all()
        lists = _foreign(rng, n, k, n_items, 1, dead)
        lp, why = _foreign_check('world 1 plain', model, users, lists, tau, lg, {})
        assert set(why.ravel().tolist()) == {LL.OK, LL.EMPTY, LL.RANGE, LL.REPEAT, LL.NOSCORE}
        assert (lp[1] == 0).all()                                # the row of -1: the empty list is certain
        # exclusions + tags; user 2 has nothing eligible
        tags, want_any, want_all, ex, ex_rows, bad_tag = _filters(rng, users, n_items, dead, ids0)
        model.prepare_item_tags(tags)
        model.prepare_recommend_exclusions(ex)
        kw = dict(exclude_seen=True, tags_any=want_any, tags_all=want_all)
        filt = dict(tags=tags, want_any=want_any, want_all=want_all, ex_lists=ex_rows)
        ids1, v1, lp1 = _self_drawn(model, users, k, tau, 21, **kw)
        assert (ids1[2] == -1).all()
        lists = _foreign(rng, n, k, n_items, 1, dead, ex_rows, bad_tag)
        lp, why = _foreign_check('world 1 ex + tags', model, users, lists, tau, lg, filt, **kw)
        assert set(why.ravel().tolist()) == set(range(7))
        assert (why[2] != LL.OK).all() and np.isneginf(lp[2][why[2] >= LL.RANGE]).all()
        # another k right after: nothing stale; a single user
        _foreign_check('world 1 k 7', model, users, lists[:, :7], tau, lg, filt, **kw)
        _foreign_check('world 1 one user', model, users[:1], lists[:1, :17], tau[:1], lg[:1],
                       {q: v[:1] if q != 'tags' else v for q, v in filt.items()}, exclude_seen=True,
                       tags_any=want_any[:1], tags_all=want_all[:1])
        # recommend_sampled afterwards: unchanged bits
        again = model.recommend_sampled(users, k, return_values=True, sample_temperature=tau, sample_seed=21,
                                        return_logprob=True, **kw)
        for g, w in zip(again, (ids1, v1, lp1)):
            np.testing.assert_array_equal(g.cpu().numpy(), w)
    finally:
        dist.destroy_process_group()


def _two_rank_worker(rank, world, port, out_dir):
    import sys
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from arx.dist import ShardedHMF

    # uneven shards, both past the first chunk
    n_users, n_items, d, B_loc, k = 401, 2 * 70003 + 1, 64, 48, 30
    dead = [10, 11, 140001]
    U, I, b = _tables(n_users, n_items, d, dead, seed=9)
    model = ShardedHMF(n_users, n_items, d, B_loc, 64, 0.1, rank, world, dev,
                       tables={'user': U.numpy(), 'item': I.numpy(), 'item_bias': b.numpy()})
    rng = np.random.default_rng(21)                                     # the same stream on both ranks
    asks = [rng.choice(np.arange(s, n_users, world), size=B_loc - 7 * s, replace=False) for s in range(world)]
    U_all = torch.zeros(world * B_loc, d, device=dev)
    for s in range(world):
        U_all[s * B_loc:s * B_loc + len(asks[s])] = U[torch.from_numpy(asks[s])].to(dev)
    mine = asks[rank]
    n = len(mine)
    mrng = np.random.default_rng(70 + rank)
    tau = np.array([0.25, 1.0, 3.0], dtype=np.float32)[mrng.integers(0, 3, n)]
    lg = _shard_logits(U_all, I.to(dev), b.to(dev), world, rank * B_loc + np.arange(n), dev)
    ids0, v0, lp0 = _self_drawn(model, mine, k, tau, 31)
    owners = ids0[ids0 >= 0] % world
    assert (owners == 0).any() and (owners == 1).any()
    lists = _foreign(mrng, n, k, n_items, world, dead)
    _foreign_check('rank %d plain' % rank, model, mine, lists, tau, lg, {})
    # ---- exclusions + tags (the tags are the same on both ranks)
    tags = T.random_tags(rng, n_items)
    tags[dead] = 0xffffffff
    _, want_any, want_all, ex, ex_rows, _ = _filters(mrng, mine, n_items, dead, ids0)
    ok = T.eligible(tags, want_any, want_all)
    bad_tag = [[int(c) for c in np.nonzero(~ok[r])[0][:400] if c not in ex_rows[r]] for r in range(n)]
    model.prepare_item_tags(tags)
    model.prepare_recommend_exclusions(ex)
    kw = dict(exclude_seen=True, tags_any=want_any, tags_all=want_all)
    filt = dict(tags=tags, want_any=want_any, want_all=want_all, ex_lists=ex_rows)
    _self_drawn(model, mine, k, tau, 32, **kw)
    lists = _foreign(mrng, n, k, n_items, world, dead, ex_rows, bad_tag)
    lp, why = _foreign_check('rank %d ex + tags' % rank, model, mine, lists, tau, lg, filt, **kw)
    assert set(why.ravel().tolist()) == set(range(7))
    for c in (LL.OK, LL.EXCLUDED, LL.TAGS):
        assert len(set((lists[why == c] % world).tolist())) == world     # decided by both shards
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_sharded_list_logprob_two_ranks_one_gpu(dev, tmp_path):
    """Two rank processes on the one GPU over gloo: uneven shards and asks, lists with entries owned by both shards,
    with and without exclusions + tags, against the global oracle; the self-drawn list bit-equal.  The two processes
    run under a time limit of their own."""
    import torch.multiprocessing as mp
    port = 30180 + (os.getpid() % 100)
    ctx = mp.spawn(_two_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 240.0
    try:
        while not ctx.join(timeout=5.0):
            assert time.monotonic() < deadline, "the rank processes did not finish in time"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))


def test_sharded_w2v_list_logprob_world1(dev):
    """ShardedW2V, 2003 items, d 32: the lists' propensities under x_test of (users, context)."""
    import torch
    import torch.distributed as dist
    from arx.dist import ShardedW2V
    _init_world1(dev, 29812)
    try:
        n_users, n_items, d, B_loc, n_in, k = 300, 2003, 32, 32, 3, 20
        dead = [7, 1500]
        U, I, b = _tables(n_users, n_items, d, dead, seed=5)
        Cx = torch.randn(n_items, d, generator=torch.Generator(device='cpu').manual_seed(6)) * 0.3
        model = ShardedW2V(n_users, n_items, d, B_loc, 64, n_in, 0.1, 0, 1, dev, graphs=False,
                           tables={'userembed_cat_0': U.numpy(), 'itemembed_cat_0': Cx.numpy(),
                                   'item_outputembed_cat_0': I.numpy(), 'item_output_bias_cat_0': b.numpy()})
        rng = np.random.default_rng(8)
        users = rng.choice(n_users, size=B_loc - 3, replace=False)
        n = len(users)
        ctx = rng.integers(0, n_items, size=(n_in, n))
        X = torch.zeros(B_loc, d, device=dev)
        model._serve_ctx = model._context_array(ctx, n, "test")
        model._serve_latents(users, X[:n])
        model._serve_ctx = None
        lg = _shard_logits(X, model.E_item[:n_items], model.b_item[:n_items], 1, np.arange(n), dev)
        tau = np.array([0.5, 2.0], dtype=np.float32)[rng.integers(0, 2, n)]
        _self_drawn(model, users, k, tau, 3, pre=(ctx,))
        lists = _foreign(rng, n, k, n_items, 1, dead)
        lp, why = _foreign_check('w2v', model, users, lists, tau, lg, {}, pre=(ctx,))
        assert set(why.ravel().tolist()) == {LL.OK, LL.EMPTY, LL.RANGE, LL.REPEAT, LL.NOSCORE}
    finally:
        dist.destroy_process_group()


def test_sharded_het_view_list_logprob_world1(dev):
    """ShardedHetView over a ShardedHMFRepTokens model, 2003 items, d 32; the training class points at the view."""
    import torch
    import torch.distributed as dist
    from arx.dist import ShardedHMFRepTokens
    from test_sharded_het_view_gpu import _random_bags
    _init_world1(dev, 29813)
    try:
        n_users, n_items, n_tok, d, B_loc, k = 300, 2003, 400, 32, 32, 20
        rng = np.random.default_rng(31)
        model = ShardedHMFRepTokens(n_users, n_items, d, B_loc, 64, 0.1, 0, 1, dev, _random_bags(rng, n_items, n_tok),
                                    n_tok, seed=3, graphs=False)
        with torch.no_grad():                             # (scores that tell the items apart)
            for t in (model.E_user, model.E_item[:n_items], model.E_tok[:n_tok]):
                t.mul_(40.0)
        dead = [9, 1200]
        users = rng.choice(n_users, size=B_loc - 3, replace=False)
        n = len(users)
        with pytest.raises(NotImplementedError, match="item_view"):
            model.list_logprob(users, np.zeros((n, k), dtype=np.int64), 1.0)
        view = model.item_view()
        view.refresh()
        view.b_item[dead] = float('-inf')
        X = torch.zeros(B_loc, d, device=dev)
        X[:n] = view.E_user[torch.from_numpy(users).to(dev)]
        lg = _shard_logits(X, view.E_item[:n_items], view.b_item[:n_items], 1, np.arange(n), dev)
        tau = np.array([0.5, 2.0], dtype=np.float32)[rng.integers(0, 2, n)]
        _self_drawn(view, users, k, tau, 3)
        lists = _foreign(rng, n, k, n_items, 1, dead)
        lp, why = _foreign_check('het view', view, users, lists, tau, lg, {})
        assert set(why.ravel().tolist()) == {LL.OK, LL.EMPTY, LL.RANGE, LL.REPEAT, LL.NOSCORE}
        assert view.n_refresh == 1
    finally:
        dist.destroy_process_group()
