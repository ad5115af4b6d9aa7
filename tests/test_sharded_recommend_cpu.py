"""Recommend of the row-sharded HMF model (arx.dist.ShardedHMF.recommend) without a GPU: gloo worlds of 2, 3 and 4
ranks with a numpy compute double for the two recommend stages, against a numpy top-k over the GLOBAL tables --
n_items not divisible by the world, item rows duplicated across shards (the cross-shard tie rule), k larger than the
smallest shard, a rank without users, exclusions that leave a user fewer than k items, a user whose excluded items
all sit on one shard and a second prepare_recommend_exclusions that replaces the first.  Table entries are small
dyadic numbers: every score is exact in float32 and float64, so ties are real ties everywhere.  Also the argument
checks of arx_topk_merge_shards (no launch needed)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_recommend(U, I, b, users, k, ex=None):
    """global ids [len(users), k]: the top-k of U[u] . I^T + b by (score desc, id asc), excluded items and -inf
    entries -> -1 (float64)."""
    out = np.full((len(users), k), -1, dtype=np.int64)
    for j, u in enumerate(users):
        x = U[u].astype(np.float64) @ I.astype(np.float64).T + b.astype(np.float64)
        if ex is not None and len(ex.get(int(u), ())):
            x[np.asarray(sorted(ex[int(u)]), dtype=np.int64)] = -np.inf
        o = np.lexsort((np.arange(len(x)), -x))[:k]
        o = np.where(np.isneginf(x[o]), -1, o)
        out[j, :len(o)] = o
    return out


def _backend():
    from numpy_backend import NumpyBackend

    class RecBackend(NumpyBackend):
        """numpy doubles of HipBackend.shard_topk / topk_merge_shards."""

        def shard_topk(self, U, E, bias, k, ex, values, indices):
            u, e, b = (t.numpy().astype(np.float64) for t in (U, E, bias))
            x = u @ e.T + b[None, :]
            B, V = x.shape
            if ex is not None:
                keys, key_rows, ptr, cols = (t if isinstance(t, int) else t.numpy() for t in ex)
                for r in range(B):
                    key = int(keys[r % key_rows])
                    if key >= 0:
                        x[r, cols[ptr[key]:ptr[key + 1]].astype(np.int64)] = -np.inf
            vals = np.full((B, k), -np.inf)
            idx = np.full((B, k), -1, dtype=np.int64)
            for r in range(B):
                o = np.lexsort((np.arange(V), -x[r]))[:k]
                vals[r, :len(o)], idx[r, :len(o)] = x[r, o], o
            idx[np.isneginf(vals)] = -1
            values.numpy()[...] = vals.astype(np.float32)
            indices.numpy()[...] = idx.astype(np.int32)

        def topk_merge_shards(self, v, c, vo, io):
            vv, cc = v.numpy().astype(np.float64), c.numpy().astype(np.int64)
            W, B, k = vv.shape
            gid = cc * W + np.arange(W)[:, None, None]
            for r in range(B):
                x, g, ok = vv[:, r].ravel(), gid[:, r].ravel(), cc[:, r].ravel() >= 0
                x, g = x[ok], g[ok]
                o = np.lexsort((g, -x))[:k]
                rv = np.full(k, -np.inf)
                ri = np.full(k, -1, dtype=np.int64)
                rv[:len(o)], ri[:len(o)] = x[o], g[o]
                ri[np.isneginf(rv)] = -1
                vo.numpy()[r], io.numpy()[r] = rv.astype(np.float32), ri.astype(np.int32)
    return RecBackend()


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from arx.dist import ShardedHMF

    n_users, n_items, d, B_loc = 23, 37, 16, 6          # 37 % W != 0 for W = 2, 3, 4; the smallest shard: 9 rows
    rng = np.random.default_rng(7)                      # the same tables on every rank
    U = (rng.integers(-2, 3, size=(n_users, d)) / 2.0).astype(np.float32)
    I = (rng.integers(-2, 3, size=(n_items, d)) / 2.0).astype(np.float32)
    b = (rng.integers(-4, 5, size=n_items) / 4.0).astype(np.float32)
    for a, c in ((5, 6), (11, 8), (20, 33)):            # equal rows on different shards: ties across shards
        I[c], b[c] = I[a], b[a]
    U[3] = U[4]                                         # (and two users with equal latents)
    tables = {'user': U, 'item': I, 'item_bias': b}
    model = ShardedHMF(n_users, n_items, d, B_loc, 8, 0.5, rank, world, 'cpu', backend=_backend(), tables=tables)
    own = np.arange(rank, n_users, world)
    users = own[:B_loc] if rank != world - 1 else own[:0]      # the last rank asks for nobody
    if rank == 0:
        users = own[[0, 1, 2, 1]]                       # a user twice
    k = 12                                              # > the smallest shard (9 rows at W = 4)

    with pytest.raises(ValueError):
        model.recommend(users, k, exclude_seen=True)    # nothing prepared yet
    with pytest.raises(ValueError):
        model.prepare_recommend_exclusions({int(own[0]) + 1: [1]} if world > 1 else {n_users: [1]})
    got, vals = model.recommend(users, k, return_values=True)
    want = oracle_recommend(U, I, b, users, k)
    np.testing.assert_array_equal(got.numpy(), want)
    for j, u in enumerate(users):
        np.testing.assert_array_equal(vals.numpy()[j], (U[u] @ I.T + b)[want[j]].astype(np.float32))
    np.testing.assert_array_equal(model.recommend(users, 1).numpy(), want[:, :1])

    # exclusions: every rank passes the histories of its own users
    def history(g, which):
        ex = {}
        for u in np.arange(g, n_users, world):
            r = np.random.default_rng(1000 * which + int(u))
            if which == 0 and u % 5 == 0:
                ex[int(u)] = r.choice(n_items, size=n_items - 4, replace=False).tolist()   # 4 eligible < k
            elif which == 0 and u % 5 == 1:
                ex[int(u)] = list(range(1, n_items, world)) * 2                           # all on shard 1, twice
            else:
                ex[int(u)] = r.integers(0, n_items, size=int(r.integers(0, 12))).tolist()
        return ex
    hist = [history(g, 0) for g in range(world)]
    model.prepare_recommend_exclusions(hist[rank])
    ex_all = {u: set(v) for h in hist for u, v in h.items()}
    got = model.recommend(users, k, exclude_seen=True).numpy()
    want = oracle_recommend(U, I, b, users, k, ex_all)
    np.testing.assert_array_equal(got, want)
    short = [j for j, u in enumerate(users) if u % 5 == 0]
    assert all((want[j, 4:] == -1).all() and (want[j, :4] >= 0).all() for j in short)
    # ... and the same through a (users, ptr, items) CSR triple; then a second set that replaces the first
    hist2 = [history(g, 1) for g in range(world)]
    mine = sorted(hist2[rank])
    ptr = np.concatenate([[0], np.cumsum([len(hist2[rank][u]) for u in mine])]).astype(np.int64)
    its = np.concatenate([np.asarray(hist2[rank][u], dtype=np.int64) for u in mine] + [np.zeros(0, np.int64)])
    model.prepare_recommend_exclusions((np.asarray(mine), ptr, its))
    ex2 = {u: set(v) for h in hist2 for u, v in h.items()}
    got = model.recommend(users, k, exclude_seen=True).numpy()
    np.testing.assert_array_equal(got, oracle_recommend(U, I, b, users, k, ex2))
    np.testing.assert_array_equal(model.recommend(users, k).numpy(), oracle_recommend(U, I, b, users, k))
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_sharded_recommend_matches_global_topk_gloo(tmp_path, world):
    import torch.multiprocessing as mp
    port = 31300 + 10 * world + (os.getpid() % 50) * 40
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(world))


def test_bag_models_have_no_recommend_yet():
    from arx.dist import ShardedHMFBags, ShardedHMFRepTokens
    for cls in (ShardedHMFBags, ShardedHMFRepTokens):
        with pytest.raises(NotImplementedError):
            cls.recommend(object.__new__(cls), [0], 5)


def test_topk_merge_shards_argument_validation_without_gpu():
    """arx_topk_merge_shards refuses null pointers, W outside [1, 64] and k outside [1, 1024] before any launch
    (small integers stand in for device pointers: they are only compared with NULL)."""
    from arx import _lib
    lib = _lib.lib
    EINVAL = -1
    f = lib.arx_topk_merge_shards

    def err():
        m = lib.arx_last_error()
        return m.decode() if m else ""
    for args in ((None, 1, 4, 2, 10, 1, 1), (1, None, 4, 2, 10, 1, 1), (1, 1, 4, 2, 10, None, 1),
                 (1, 1, 4, 2, 10, 1, None), (1, 1, 4, 0, 10, 1, 1), (1, 1, 4, 65, 10, 1, 1),
                 (1, 1, 4, 2, 0, 1, 1), (1, 1, 4, 2, 1025, 1, 1), (1, 1, -1, 2, 10, 1, 1)):
        assert f(*args, None) == EINVAL, args
        assert "arx_topk_merge_shards" in err()
    assert f(1, 1, 0, 64, 1024, 1, 1, None) == 0          # B = 0: nothing to do, no launch
