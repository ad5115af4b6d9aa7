"""arx_het_rows_range and the serving view of the sharded HET models (ShardedHetView) on the GPU.

The kernel is compared bit for bit with arx_gather_id_plus_bag on the explicit id vector c * W + s; the view's
recommend / evaluate are compared exactly with a reference ShardedHMF whose item table holds latents materialised by
that existing kernel (the same GEMM on the same bits), and -- two ranks on the one GPU, dyadic tables -- with the
global float64 oracles of the CPU tests."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.5


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("d", [32, 36, 64, 128])
def test_het_rows_range_equals_gather_id_plus_bag(dev, d, world):
    """ops.het_rows_range == ops.gather_id_plus_bag on ids = c * W + s, exactly: n_items = 1001 (a ragged stripe and
    columns past it: zero rows), bags of 1 .. 40 tokens (33 and 40: more than one sub-group pass at d = 32), c0 > 0,
    one owner and all owners (there: the rank's masked copy of vals and its token stripe on both sides, as the
    token-striped step passes them), packed and separate bias outputs; the sentinel around the range, between the
    owner blocks and in the columns behind the bias stays."""
    import torch
    from arx import ops
    W, n_items, n_tok = world, 1001, 301
    rng = np.random.default_rng(100 * d + W)
    lens = rng.choice([1, 2, 3, 4, 5, 8, 12, 20, 33, 40], size=n_items).astype(np.int32)
    lens[:4] = [1, 4, 5, 33]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    vals = rng.integers(0, n_tok, size=int(lens.sum())).astype(np.int32)
    T = rng.standard_normal((n_tok, d)).astype(np.float32)
    bT = rng.standard_normal(n_tok).astype(np.float32)
    I = rng.standard_normal((n_items, d)).astype(np.float32)
    b = rng.standard_normal(n_items).astype(np.float32)
    cols = (n_items + W - 1) // W
    c0, c1 = 3, cols + 1                                  # (column `cols`: past every stripe)
    t_starts, t_lens = torch.from_numpy(starts).to(dev), torch.from_numpy(lens).to(dev)
    for rank in sorted({0, W - 1}):
        ni = (n_items - rank + W - 1) // W
        E_id = torch.zeros((ni + 1, d), dtype=torch.float32, device=dev)          # the shard + its zero row
        E_id[:ni] = torch.from_numpy(I[rank::W]).to(dev)
        b_id = torch.zeros(ni + 1, dtype=torch.float32, device=dev)
        b_id[:ni] = torch.from_numpy(b[rank::W]).to(dev)
        g_all = np.arange(n_items, dtype=np.int64)
        cmap = torch.from_numpy(np.where(g_all % W == rank, g_all // W, ni).astype(np.int32)).to(dev)
        for all_owners in (False, True):
            if all_owners:                                # the rank's token stripe, other owners' tokens -> its zero row
                nt = (n_tok - rank + W - 1) // W
                E_tok = torch.zeros((nt + 1, d), dtype=torch.float32, device=dev)
                E_tok[:nt] = torch.from_numpy(T[rank::W]).to(dev)
                b_tok = torch.zeros(nt + 1, dtype=torch.float32, device=dev)
                b_tok[:nt] = torch.from_numpy(bT[rank::W]).to(dev)
                v = vals.astype(np.int64)
                t_vals = torch.from_numpy(np.where(v % W == rank, v // W, nt).astype(np.int32)).to(dev)
            else:
                E_tok, b_tok, t_vals = torch.from_numpy(T).to(dev), torch.from_numpy(bT).to(dev), \
                    torch.from_numpy(vals).to(dev)
            owners = list(range(W)) if all_owners else [rank]
            block_rows = (c1 - c0) + 2 if all_owners else 0
            # the rows of the range, their items, and the reference rows of the items that exist
            rows = np.concatenate([(s * block_rows if all_owners else 0) + np.arange(c1 - c0) for s in owners])
            gids = np.concatenate([np.arange(c0, c1, dtype=np.int64) * W + s for s in owners])
            live = gids < n_items
            assert (~live).any() and live.any()
            ids = torch.from_numpy(gids[live].astype(np.int32)).to(dev)
            ref = torch.empty((int(live.sum()), d), dtype=torch.float32, device=dev)
            ref_b = torch.empty(int(live.sum()), dtype=torch.float32, device=dev)
            ops.gather_id_plus_bag(E_id, b_id, cmap, E_tok, b_tok, t_vals, t_starts, t_lens, ids, ref, scale=0.5,
                                   bias_out=ref_b)
            R = int(rows.max()) + 1 + 3                   # three sentinel rows behind the range
            r_live = torch.from_numpy(rows[live]).to(dev)
            r_dead = torch.from_numpy(rows[~live]).to(dev)
            for packed in (True, False):
                width = d + 4 if packed else d
                want = torch.full((R, width), SENT, dtype=torch.float32, device=dev)
                want_b = want[:, d] if packed else torch.full((R,), SENT, dtype=torch.float32, device=dev)
                want[r_live, :d], want[r_dead, :d] = ref, 0.0
                want_b[r_live], want_b[r_dead] = ref_b, 0.0
                out = torch.full((R, width), SENT, dtype=torch.float32, device=dev)
                out_b = None if packed else torch.full((R,), SENT, dtype=torch.float32, device=dev)
                ops.het_rows_range(E_id, b_id, E_tok, b_tok, t_vals, t_starts, t_lens, n_items, W, rank, c0, c1, out,
                                   bias_out=out_b, all_owners=all_owners, scale=0.5, block_rows=block_rows)
                what = (d, W, rank, all_owners, packed)
                assert torch.equal(out, want), what
                if not packed:
                    assert torch.equal(out_b, want_b), what
    with pytest.raises(ValueError):                       # (the wrapper refuses an output the range does not fit in)
        ops.het_rows_range(E_id, b_id, E_tok, b_tok, t_vals, t_starts, t_lens, n_items, W, rank, 0, cols,
                           torch.empty((cols - 1, d + 4), dtype=torch.float32, device=dev))


# ---------------------------------------------------------------- world 1
def _init_world1(dev, port):
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)


def _random_bags(rng, n_items, n_tok, max_len=12):
    lens = rng.integers(1, max_len + 1, size=n_items).astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    return rng.integers(0, n_tok, size=int(lens.sum())).astype(np.int32), starts, lens


def _reference_hmf(model, B_loc, dev):
    """A ShardedHMF (world 1) over the model's user table and its item latents as the EXISTING kernel materialises
    them (arx_gather_id_plus_bag on ids 0 .. n_items-1)."""
    import torch
    from arx import ops
    from arx.dist import ShardedHMF
    n = model.n_items
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    L = torch.empty((n, model.d), dtype=torch.float32, device=dev)
    Lb = torch.empty(n, dtype=torch.float32, device=dev)
    ops.gather_id_plus_bag(model.E_item, model.b_item, None, model.E_tok, model.b_tok, model.bag_vals,
                           model.bag_starts, model.bag_lens, ids, L, scale=0.5, bias_out=Lb)
    return ShardedHMF(model.n_users, n, model.d, B_loc, 64, 0.1, 0, 1, dev, graphs=False,
                      tables={'user': model.E_user.cpu().numpy(), 'item': L.cpu().numpy(),
                              'item_bias': Lb.cpu().numpy()})


@pytest.mark.parametrize("cls_name", ["ShardedHMFRepTokens", "ShardedHMFBags"])
def test_het_view_world1_equals_reference_hmf(dev, cls_name):
    """n_items = 70001 (past the 65 536 chunk: the fused filter GEMM runs), d = 64, 64 users, k = 100: recommend (with
    and without exclusions, with values) and evaluate (three losses, with rows) through the view == the same calls on
    a reference ShardedHMF over latents from the existing kernel, exactly."""
    import torch
    import torch.distributed as dist
    from arx import dist as adist
    _init_world1(dev, 29781)
    try:
        n_users, n_items, n_tok, d, B_loc, k = 500, 70001, 5000, 64, 64, 100
        rng = np.random.default_rng(31)
        bags = _random_bags(rng, n_items, n_tok)
        model = getattr(adist, cls_name)(n_users, n_items, d, B_loc, 64, 0.1, 0, 1, dev, bags, n_tok, seed=3,
                                         graphs=False)
        with torch.no_grad():                             # (scores that tell the items apart)
            for t in (model.E_user, model.E_item[:n_items], model.E_tok[:n_tok]):
                t.mul_(40.0)
        view = model.item_view()
        ref = _reference_hmf(model, B_loc, dev)
        users = rng.choice(n_users, size=B_loc - 5, replace=False)
        got, gv = view.recommend(users, k, return_values=True)
        want, wv = ref.recommend(users, k, return_values=True)
        assert torch.equal(view.E_item, ref.E_item) and torch.equal(view.b_item, ref.b_item)
        assert torch.equal(got, want) and torch.equal(gv, wv)
        assert len(torch.unique(want[0])) == k
        ex = {int(u): rng.integers(0, n_items, size=40).tolist() + want[j, :20].cpu().tolist()
              for j, u in enumerate(users)}
        view.prepare_recommend_exclusions(ex)
        ref.prepare_recommend_exclusions(ex)
        got, gv = view.recommend(users, k, exclude_seen=True, return_values=True)
        want2, wv = ref.recommend(users, k, exclude_seen=True, return_values=True)
        assert torch.equal(got, want2) and torch.equal(gv, wv) and not torch.equal(want2, want)
        items = rng.integers(0, n_items, size=len(users))
        pos = {int(u): rng.integers(0, n_items, size=30).tolist() for u in users}
        view.prepare_eval_positives(pos)
        ref.prepare_eval_positives(pos)
        for loss in ('ce', 'warp'):
            gm, gr = view.evaluate(users, items, loss=loss, return_rows=True)
            wm, wr = ref.evaluate(users, items, loss=loss, return_rows=True)
            assert gm == wm and torch.equal(gr, wr) and np.isfinite(gm), loss
        (gm, gc), (wm, wc) = view.evaluate(users, items, loss='warp_eval'), ref.evaluate(users, items, loss='warp_eval')
        assert torch.equal(gm, wm) and torch.equal(gc, wc) and int(wc.max()) > 0
        assert view.n_refresh == 1
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("cls_name", ["ShardedHMFRepTokens", "ShardedHMFBags"])
def test_het_view_between_captured_steps(dev, cls_name):
    """graphs=True: three steps, recommend through the view (== the reference over the tables as they stand), one more
    step; the tables are bit-identical to a twin that never had a view, and the view captured nothing."""
    import torch
    import torch.distributed as dist
    from arx import dist as adist
    from arx.utils.synthetic import SyntheticHMF
    _init_world1(dev, 29782)
    try:
        n_users, n_items, V, d, B, S, k = 300, 500, 120, 64, 32, 64, 30
        syn = SyntheticHMF(n_users=n_users, n_items=n_items, seed=1, permute_logits=False, n_pos=8,
                           item_mulhot=True, mulhot_vocab=V, avg_len=5, max_len=12)
        ia = syn.i_attr
        n_tok = ia._embedding_classes_list_mulhot[0]
        params = syn.glorot_params(d, seed=2, scale=0.5)
        tables = {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
                  'item_bias': params['item_bias_cat_0'][2:], 'token': params['itemembed_mulhot_0'],
                  'token_bias': params['item_bias_mulhot_0']}
        bags = (np.asarray(ia.features_mulhot[0]), np.asarray(ia.mulhot_starts[0]), np.asarray(ia.mulhot_lengths[0]))
        ptr = np.concatenate([syn.pos_ptr[:n_users + 1], [syn.pos_ptr[n_users]]]).astype(np.int32)
        models = [getattr(adist, cls_name)(n_users, n_items, d, B, S, 0.5, 0, 1, dev, bags, n_tok, tables=tables,
                                           graphs=True) for _ in range(2)]
        rng = np.random.default_rng(3)
        pool = syn.sample_pool(S, rng)
        for m in models:
            assert m.use_graphs
            m.set_positives(ptr, syn.pos_items)
            m.set_pool(pool)
        view = models[0].item_view()
        batches = [syn.sample_batch(B, rng) for _ in range(4)]
        ask = rng.choice(n_users, size=B, replace=False)
        for step, (users, items) in enumerate(batches):
            for m in models:
                m.step(users, items)
            if step == 2:
                got = view.recommend(ask, k)
                assert view.steps == 3 and view.n_refresh == 1
                want = _reference_hmf(models[0], B, dev).recommend(ask, k)
                assert torch.equal(got, want)
        assert models[0].n_replays > 0 and models[0].n_replays == models[1].n_replays
        assert models[0].n_captures == models[1].n_captures >= 1
        for name in ('E_user', 'A_user', 'E_item', 'A_item', 'b_item', 'Ab_item', 'E_tok', 'A_tok', 'b_tok', 'Ab_tok'):
            assert torch.equal(getattr(models[0], name), getattr(models[1], name)), name
        assert view.steps == 3 and models[0].steps == 4                 # (stale again, by one step)
    finally:
        dist.destroy_process_group()


# ---------------------------------------------------------------- two ranks on one GPU (gloo)
def _two_rank_setup(rank, world, port):
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
    return torch.device('cuda', 0)


def _two_rank_oracle_worker(rank, world, port, out_dir):
    """Both classes over the dyadic tables of the CPU test at d = 32 on the HIP backend: recommend ids and the
    'warp_eval' true ranks exact against the global float64 oracles (the token-striped view: its owner-major partial
    blocks through the reduce-scatter, in chunks of 4 columns)."""
    dev = _two_rank_setup(rank, world, port)
    import torch.distributed as dist
    import test_sharded_eval_cpu as tec
    import test_sharded_het_view_cpu as hv
    from test_sharded_recommend_cpu import oracle_recommend
    from arx import dist as adist
    n_users, n_items, d, B_loc, k = tec.N_USERS, tec.N_ITEMS, 32, tec.B_LOC, 12
    U, I, b, T, bT, bags = hv._tables(d)
    L, Lb = hv._latents(I, b, T, bT, bags)
    tables = {'user': U, 'item': I, 'item_bias': b, 'token': T, 'token_bias': bT}
    own = np.arange(rank, n_users, world)
    users = own[[0, 1, 2, 1]] if rank == 0 else own[:B_loc]
    eu = own[[0, 1, 2, 1]]                                              # a user twice; targets with equal rows elsewhere
    ei = np.random.default_rng(200 + rank).integers(0, n_items, size=len(eu)).astype(np.int64)
    ei[0], ei[2] = tec.TIES[rank][0], tec.TIES[rank + 1][1]
    pos = [tec.positives(g, world, 0) for g in range(world)]
    pos_all = {u: set(v) for p in pos for u, v in p.items()}
    for cls_name in ('ShardedHMFRepTokens', 'ShardedHMFBags'):
        model = getattr(adist, cls_name)(n_users, n_items, d, B_loc, 8, 0.5, rank, world, dev, bags, hv.N_TOK,
                                         tables=tables)
        view = model.item_view(chunk_cols=4)
        got = view.recommend(users, k).cpu().numpy()
        np.testing.assert_array_equal(got, oracle_recommend(U, L, Lb, users, k), err_msg=cls_name)
        ni = model.ni_loc
        np.testing.assert_array_equal(view.E_item[:ni].cpu().numpy(), L[rank::world].astype(np.float32))
        np.testing.assert_array_equal(view.b_item[:ni].cpu().numpy(), Lb[rank::world].astype(np.float32))
        view.prepare_eval_positives(pos[rank])
        mr, tr = view.evaluate(eu, ei, loss='warp_eval')
        wm, wr = tec.oracle_eval(U, L, Lb, eu, ei, 'warp_eval', pos_all)
        np.testing.assert_array_equal(tr.cpu().numpy(), wr, err_msg=cls_name)
        np.testing.assert_allclose(mr.cpu().numpy(), wm, rtol=1e-5, err_msg=cls_name)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_het_view_two_ranks_one_gpu_matches_global_oracle(dev, tmp_path):
    import torch.multiprocessing as mp
    port = 30080 + (os.getpid() % 100)
    mp.spawn(_two_rank_oracle_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))


def _two_rank_chunk_worker(rank, world, port, out_dir):
    dev = _two_rank_setup(rank, world, port)
    import torch
    import torch.distributed as dist
    from arx.dist import ShardedHMFBags
    n_users, n_items, n_tok, d = 40, 70001, 3001, 32                    # rank 0: ni_loc = 35001
    bags = _random_bags(np.random.default_rng(8), n_items, n_tok, max_len=6)
    model = ShardedHMFBags(n_users, n_items, d, 8, 8, 0.1, rank, world, dev, bags, n_tok, seed=4, graphs=False)
    assert model.ni_loc == 35001 - rank
    small, default = model.item_view(chunk_cols=1000), model.item_view()
    assert small.chunk == 1000 and default.chunk == 16384
    small.refresh()
    default.refresh()
    assert torch.equal(small.E_item, default.E_item) and torch.equal(small.b_item, default.b_item)
    ni = model.ni_loc
    assert float(small.E_item[:ni].abs().sum()) > 0 and not bool(small.E_item[ni].any())
    # ... and they are the latents: the last owned item against its tables, gathered from both ranks
    g = model.gather_global_tables()
    it = (ni - 1) * world + rank
    tok = bags[0][bags[1][it]:bags[1][it] + bags[2][it]]
    want = 0.5 * (g['item'][it].astype(np.float64) + g['token'][tok].astype(np.float64).mean(0))
    np.testing.assert_allclose(small.E_item[ni - 1].cpu().numpy(), want, rtol=1e-5, atol=1e-7)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_het_view_chunking_two_ranks_one_gpu(dev, tmp_path):
    """A ShardedHMFBags view with chunk_cols = 1000 at ni_loc = 35001 (36 chunks, the last one short) holds latents
    bit-identical to the default chunk's (3 chunks)."""
    import torch.multiprocessing as mp
    port = 30190 + (os.getpid() % 100)
    mp.spawn(_two_rank_chunk_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))
