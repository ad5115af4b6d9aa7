"""Recommend of the row-sharded HMF model (ShardedHMF.recommend) and its merge kernel on the GPU.

The oracle ranks the device's own logits in numpy: every shard's logits come from ops.gemm over that shard's rows in
the chunks the shard scores them in (the fused filter GEMM's values are bit-identical to them), scattered to global
columns c * W + s; excluded items -> -inf; a stable sort by (-value, global id); -inf -> -1.  Indices compare exactly.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 65536


def _rank(x, k, ex_rows=None):
    """x [R, V] float32 logits (global columns) -> ids [R, k] by (-value, id), excluded -> never, -inf -> -1"""
    x = np.array(x, dtype=np.float32, copy=True)
    R, V = x.shape
    out = np.full((R, k), -1, dtype=np.int64)
    for r in range(R):
        if ex_rows is not None and len(ex_rows[r]):
            x[r, np.asarray(sorted(ex_rows[r]), dtype=np.int64)] = -np.inf
        kk = min(k, V)
        kth = np.partition(x[r], V - kk)[V - kk]
        c = np.nonzero(x[r] >= kth)[0]
        o = c[np.lexsort((c, -x[r, c]))][:kk]
        out[r, :kk] = np.where(np.isneginf(x[r, o]), -1, o)
    return out


def _shard_logits(U_all, E_items, b_items, world, rows, dev):
    """logits [len(rows), n_items] of rows `rows` of U_all, every shard's columns as the shard computes them"""
    import torch
    from arx import ops
    ws = ops.Workspace(dev)
    n_items = E_items.shape[0]
    out = np.empty((len(rows), n_items), dtype=np.float32)
    sel = torch.as_tensor(np.asarray(rows, dtype=np.int64), device=dev)
    for s in range(world):
        E, b = E_items[s::world].contiguous(), b_items[s::world].contiguous()
        ni = E.shape[0]
        buf = torch.empty((U_all.shape[0], min(CHUNK, max(ni, 1))), dtype=torch.float32, device=dev)
        for c0 in range(0, ni, CHUNK):
            c1 = min(ni, c0 + CHUNK)
            lg = buf[:, :c1 - c0]
            ops.gemm(U_all, E[c0:c1], lg, ws, transB=True, col_bias=b[c0:c1])
            out[:, s + world * c0:s + world * c1:world] = lg[sel].cpu().numpy()
    return out


# ---------------------------------------------------------------- the merge kernel
def _merge_inputs(rng, W, B, k):
    v = (rng.integers(0, 12, size=(W, B, k)) / 4.0).astype(np.float32)         # few values: ties across blocks
    c = np.cumsum(rng.integers(1, 4, size=(W, B, k)), axis=-1).astype(np.int64) - 1
    n_ok = rng.integers(0, k + 1, size=(W, B, 1))                               # empty tails (c = -1)
    n_ok[:, 0] = k                                                              # (row 0: full lists)
    n_fin = np.minimum(n_ok, rng.integers(0, k + 1, size=(W, B, 1)) + k // 2)   # ... -inf entries in front of them
    pos = np.arange(k)[None, None, :]
    v[pos >= n_fin] = -np.inf
    empty = pos >= n_ok
    c[empty] = -1
    o = np.lexsort((c, -v.astype(np.float64), empty), axis=-1)
    return np.take_along_axis(v, o, -1), np.take_along_axis(c, o, -1).astype(np.int32)


def _merge_ref(v, c, k):
    W, B, _ = v.shape
    g = c.astype(np.int64) * W + np.arange(W)[:, None, None]
    vv = np.transpose(v, (1, 0, 2)).reshape(B, -1).astype(np.float64)
    gg = np.transpose(g, (1, 0, 2)).reshape(B, -1)
    ok = np.transpose(c, (1, 0, 2)).reshape(B, -1) >= 0
    vv = np.where(ok, vv, -np.inf)
    o = np.lexsort((gg, -vv, ~ok), axis=-1)[:, :k]
    rv, ri = np.take_along_axis(vv, o, -1), np.take_along_axis(gg, o, -1)
    ri = np.where(np.isneginf(rv), -1, ri)
    return rv.astype(np.float32), ri


@pytest.mark.parametrize("W", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("k", [1, 30, 100, 1024])
def test_topk_merge_shards_matches_numpy(dev, W, k):
    """arx_topk_merge_shards == numpy on B in {1, 7, 4096} (4096 where the input stays under 16 M entries): ties
    inside and across blocks, empty entries, -inf values, lists of every length from 0 to k."""
    import torch
    from arx import ops
    rng = np.random.default_rng(W * 1000 + k)
    for B in (1, 7, 4096):
        if W * B * k > 16 * 2 ** 20:
            continue
        v, c = _merge_inputs(rng, W, B, k)
        vo = torch.full((B, k), 7.0, dtype=torch.float32, device=dev)
        io = torch.full((B, k), 7, dtype=torch.int32, device=dev)
        ops.topk_merge_shards(torch.from_numpy(v).to(dev), torch.from_numpy(c).to(dev), vo, io)
        rv, ri = _merge_ref(v, c, k)
        np.testing.assert_array_equal(io.cpu().numpy(), ri, err_msg=str((W, B, k)))
        np.testing.assert_array_equal(vo.cpu().numpy(), rv, err_msg=str((W, B, k)))


# ---------------------------------------------------------------- world 1
def _init_world1(dev, port):
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)


def _histories(rng, users, n_items, n=40, top=None):
    ex = {}
    for j, u in enumerate(users):
        its = rng.integers(0, n_items, size=n)
        if top is not None:
            its = np.concatenate([its, top[j][:20]])
        ex[int(u)] = its.tolist()
    return ex


@pytest.mark.parametrize("rising", [False, True])
def test_sharded_recommend_world1(dev, rising):
    """World 1 (an nccl group of one): the fused path, and with rising=True scores that rise along the vocabulary so
    the fused candidate lists overflow and the request re-runs chunked -- with and without exclusions."""
    import torch
    import torch.distributed as dist
    from arx.dist import ShardedHMF
    _init_world1(dev, 29771)
    try:
        n_users, n_items, d, B_loc, k = 500, 200003, 64, 64, 100
        g = torch.Generator(device='cpu').manual_seed(3)
        U = torch.randn(n_users, d, generator=g) * 0.3
        I = torch.randn(n_items, d, generator=g) * 0.3
        b = torch.randn(n_items, generator=g) * 0.1
        if rising:
            b = b + torch.linspace(0.0, 40.0, n_items)
        I[77], b[77] = I[123456], b[123456]                                    # a tie in the id order
        model = ShardedHMF(n_users, n_items, d, B_loc, 64, 0.1, 0, 1, dev,
                           tables={'user': U.numpy(), 'item': I.numpy(), 'item_bias': b.numpy()})
        rng = np.random.default_rng(4)
        users = rng.choice(n_users, size=B_loc - 5, replace=False)
        U_all = torch.zeros(B_loc, d, device=dev)
        U_all[:len(users)] = U[torch.from_numpy(users)].to(dev)
        lg = _shard_logits(U_all, I.to(dev), b.to(dev), 1, np.arange(len(users)), dev)
        want = _rank(lg, k)
        got = model.recommend(users, k).cpu().numpy()
        np.testing.assert_array_equal(got, want)
        ov = [int(s.overflow.item()) for s in model.be._scans.values()]
        assert any(ov) == rising
        ex = _histories(rng, users, n_items, top=want)
        model.prepare_recommend_exclusions(ex)
        got, vals = model.recommend(users, k, exclude_seen=True, return_values=True)
        want = _rank(lg, k, [ex[int(u)] for u in users])
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        np.testing.assert_array_equal(vals.cpu().numpy(), np.take_along_axis(lg, want, 1))
    finally:
        dist.destroy_process_group()


def test_sharded_recommend_between_steps_graphs(dev):
    """step, recommend, step, recommend with graph segments: losses and every table bit-identical to the same steps
    without the recommends; each recommend equals the oracle on the tables as they stood."""
    import torch
    import torch.distributed as dist
    from arx.dist import ShardedHMF
    from arx.utils.synthetic import SyntheticHMF
    _init_world1(dev, 29772)
    try:
        n_users, n_items, d, B, S, k = 300, 500, 64, 32, 64, 30
        syn = SyntheticHMF(n_users=n_users, n_items=n_items, seed=1, permute_logits=False, n_pos=8)
        params = syn.glorot_params(d, seed=2, scale=0.5)
        tables = {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
                  'item_bias': params['item_bias_cat_0'][2:]}
        ptr = np.concatenate([syn.pos_ptr[:n_users + 1], [syn.pos_ptr[n_users]]]).astype(np.int32)
        models = [ShardedHMF(n_users, n_items, d, B, S, 0.5, 0, 1, dev, tables=tables, graphs=True) for _ in range(2)]
        for m in models:
            assert m.use_graphs
            m.set_positives(ptr, syn.pos_items)
        models[0].prepare_recommend_exclusions(syn.positives_dict())
        rng = np.random.default_rng(3)
        pool = syn.sample_pool(S, rng)
        for m in models:
            m.set_pool(pool)
        batches = [syn.sample_batch(B, rng) for _ in range(4)]
        ask = rng.choice(n_users, size=B, replace=False)
        losses = [[], []]
        for step, (users, items) in enumerate(batches):
            for i, m in enumerate(models):
                m.step(users, items)
                losses[i].append(float(m.read_loss().item()))
            if step % 2 == 0:
                m = models[0]
                U_all = torch.zeros(B, d, device=dev)
                U_all[:len(ask)] = m.E_user[torch.from_numpy(ask).to(dev)]
                lg = _shard_logits(U_all, m.E_item[:n_items], m.b_item[:n_items], 1, np.arange(len(ask)), dev)
                got = m.recommend(ask, k, exclude_seen=step == 2).cpu().numpy()
                pos = syn.positives_dict()
                want = _rank(lg, k, [pos.get(int(u), []) for u in ask] if step == 2 else None)
                np.testing.assert_array_equal(got, want, err_msg='step %d' % step)
        assert losses[0] == losses[1]
        assert models[0].n_replays > 0
        for name in ('E_user', 'A_user', 'E_item', 'A_item', 'b_item', 'Ab_item'):
            assert torch.equal(getattr(models[0], name), getattr(models[1], name)), name
    finally:
        dist.destroy_process_group()


def test_sharded_recommend_c5_shape_world1(dev):
    """The C5 shape at world 1: 100 M items x d 128, 1 M users, 1024 users per call, k 100, ~50 excluded items per
    user; 8 sampled rows against the oracle on the device logits of the whole vocabulary (in chunks)."""
    import torch
    import torch.distributed as dist
    from arx.dist import ShardedHMF
    _init_world1(dev, 29773)
    try:
        n_users, n_items, d, B_loc, k = 1000000, 100000000, 128, 1024, 100
        model = ShardedHMF(n_users, n_items, d, B_loc, 1024, 0.1, 0, 1, dev, seed=5)
        rng = np.random.default_rng(12)
        users = rng.choice(n_users, size=B_loc, replace=False)
        ex = {int(u): rng.integers(0, n_items, size=50).tolist() for u in users}
        model.prepare_recommend_exclusions(ex)
        got = model.recommend(users, k, exclude_seen=True).cpu().numpy()
        rows = np.sort(rng.choice(B_loc, size=8, replace=False))
        U_all = model.E_user[torch.from_numpy(users).to(dev)]
        lg = _shard_logits(U_all, model.E_item[:n_items], model.b_item[:n_items], 1, rows, dev)
        # the rows' own top-200 before the exclusion also lands in the lists: the excluded ones must be skipped
        want = _rank(lg, k, [ex[int(users[r])] for r in rows])
        np.testing.assert_array_equal(got[rows], want)
        assert (got >= 0).all() and (got < n_items).all()
    finally:
        dist.destroy_process_group()


# ---------------------------------------------------------------- two ranks on one GPU (gloo)
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

    # uneven shards, both past the first chunk and wide enough that a candidate segment spans two column tiles
    n_users, n_items, d, B_loc, k = 401, 2 * 100003 + 1, 64, 48, 100
    g = torch.Generator(device='cpu').manual_seed(9)
    U = torch.randn(n_users, d, generator=g) * 0.3
    I = torch.randn(n_items, d, generator=g) * 0.3
    b = torch.randn(n_items, generator=g) * 0.1
    b[0::2] += torch.linspace(0.0, 4000.0, (n_items + 1) // 2)         # shard 0: every column past its first chunk
    #                                                                     beats the threshold -> its lists overflow
    for a, c in ((10, 11), (1001, 2002), (5, 140000)):                  # equal rows on both shards: cross-shard ties
        I[c], b[c] = I[a], b[a]
    model = ShardedHMF(n_users, n_items, d, B_loc, 64, 0.1, rank, world, dev,
                       tables={'user': U.numpy(), 'item': I.numpy(), 'item_bias': b.numpy()})
    rng = np.random.default_rng(21)                                     # the same stream on both ranks
    asks = [rng.choice(np.arange(s, n_users, world), size=B_loc - 7 * s, replace=False) for s in range(world)]
    U_all = torch.zeros(world * B_loc, d, device=dev)
    for s in range(world):
        U_all[s * B_loc:s * B_loc + len(asks[s])] = U[torch.from_numpy(asks[s])].to(dev)
    mine = asks[rank]
    lg = _shard_logits(U_all, I.to(dev), b.to(dev), world, rank * B_loc + np.arange(len(mine)), dev)
    want = _rank(lg, k)
    np.testing.assert_array_equal(model.recommend(mine, k).cpu().numpy(), want)
    ov = [int(s.overflow.item()) for s in model.be._scans.values()]
    assert any(ov) == (rank == 0), ov
    ex_all = [_histories(np.random.default_rng(40 + s), asks[s], n_items, top=None) for s in range(world)]
    for j, u in enumerate(mine):
        ex_all[rank][int(u)] += want[j][:15].tolist()                   # the best ones of both shards
    model.prepare_recommend_exclusions(ex_all[rank])
    got = model.recommend(mine, k, exclude_seen=True).cpu().numpy()
    np.testing.assert_array_equal(got, _rank(lg, k, [ex_all[rank][int(u)] for u in mine]))
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_sharded_recommend_two_ranks_one_gpu(dev, tmp_path):
    """Two rank processes on the one GPU over gloo: uneven shards, cross-shard ties, exclusions, and rank 0's shard
    overflowing (re-run chunked on that rank only) while rank 1's does not."""
    import torch.multiprocessing as mp
    port = 29980 + (os.getpid() % 100)
    mp.spawn(_two_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))
