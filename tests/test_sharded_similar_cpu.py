"""similar_items of the row-sharded models (arx.dist) without a GPU: gloo worlds of 2, 3 and 4 ranks with numpy doubles
of the two compute stages (tests/numpy_backend_similar.py), against a numpy cosine top-k over the GLOBAL table.
n_items = 37 (not divisible by the world), d = 16; the id-only tables are the exact data of tests/similar_oracle.py
(every cosine exact: ties are real ties, ids and values compare exactly) with equal rows on different shards; k larger
than the smallest shard, k = n_items, a rank without queries, a query twice, include_self both ways, a query the rank
does not own, ShardedW2V over its output table, and the serving view of the HET models refreshing after a step (its
latents are half sums, not exact data: the random rule of similar_oracle.check_random)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_USERS, N_ITEMS, D, B_LOC = 23, 37, 16, 6


def _table():
    import similar_oracle as S
    E = S.exact_table(np.random.default_rng(11), N_ITEMS, D)
    for a, c in ((5, 6), (11, 8), (20, 33)):              # equal rows on different shards: ties across shards
        E[c] = E[a]
    return E


def _queries(rank, world):
    own = np.arange(rank, N_ITEMS, world)
    q = own[:B_LOC] if rank != world - 1 else own[:0]     # the last rank asks for nothing
    if rank == 0:
        q = own[[0, 1, 2, 1]]                             # a query twice
    return own, q


def _check_exact(model, E, rank, world):
    import similar_oracle as S
    own, q = _queries(rank, world)
    C = S.cos64(E[q], E) if len(q) else np.zeros((0, N_ITEMS))
    for k in (12, 1, N_ITEMS):                            # 12 > the smallest shard (9 rows at W = 4)
        for include_self in (False, True):
            ids, vals = model.similar_items(q, k, include_self=include_self, return_values=True)
            wv, wi = S.topk_cos(C, k, None if include_self else q)
            np.testing.assert_array_equal(ids.numpy(), wi)
            np.testing.assert_array_equal(vals.numpy().astype(np.float64), wv)
            if include_self and len(q):
                first = ids.numpy()[:, 0]                   # the query or an equal direction below it: exactly 1
                assert all(C[r, f] == 1.0 and f <= g or not E[g].any() for r, (f, g) in enumerate(zip(first, q)))
            if not include_self and k == N_ITEMS and len(q):
                assert (ids.numpy()[:, -1] == -1).all() and np.isneginf(vals.numpy()[:, -1]).all()
    only = model.similar_items(q, 5)
    np.testing.assert_array_equal(only.numpy(), S.topk_cos(C, 5, q)[1])
    # refusals, before any collective: a query of another rank, ids out of range, too many, a bad k
    with pytest.raises(ValueError):
        model.similar_items([int(own[0]) + 1] if world > 1 else [N_ITEMS], 3)
    with pytest.raises(ValueError):
        model.similar_items([-1], 3)
    with pytest.raises(ValueError):
        model.similar_items(np.repeat(own[:1], B_LOC + 1), 3)
    for k in (0, N_ITEMS + 1):
        with pytest.raises(ValueError):
            model.similar_items(q, k)


def _check_view(cls_name, rank, world):
    import similar_oracle as S
    import test_sharded_het_view_cpu as thv
    from arx import dist as adist
    from numpy_backend_similar import NumpySimilarBackend
    U, I, b, T, bT, bags = thv._tables()
    tables = {'user': U, 'item': I, 'item_bias': b, 'token': T, 'token_bias': bT}
    model = getattr(adist, cls_name)(N_USERS, N_ITEMS, D, B_LOC, thv.S_POOL, 0.5, rank, world, 'cpu', bags, thv.N_TOK,
                                     backend=NumpySimilarBackend(), tables=tables)
    own, q = _queries(rank, world)
    k, atol = 12, S.cos_atol(D)

    def check(L):
        ids, vals = model.similar_items(q, k, return_values=True)          # through the model's own view
        if len(q):
            S.check_random(ids.numpy(), vals.numpy(), S.cos64(L[q], L), k, q, atol)
        inc = model.similar_items(q, 3, include_self=True).numpy()
        assert all(S.cos64(L[[g]], L[[f]])[0, 0] >= 1.0 - atol for f, g in zip(inc[:, 0], q))
    L, _ = thv._latents(I, b, T, bT, bags)
    check(L)
    view = model._sim_view
    assert isinstance(view, adist.ShardedHetView) and view.n_refresh == 1
    check(L)
    assert view.n_refresh == 1                                              # nothing stepped: no second materialisation
    # two step()s: the next call refreshes by itself, once
    rng = np.random.default_rng(77)                                         # the same stream on every rank
    uown = np.arange(rank, N_USERS, world)
    ptr = np.zeros(len(uown) + 2, dtype=np.int32)
    pitems = []
    for j, u in enumerate(uown):
        pitems.extend(np.random.default_rng(500 + int(u)).choice(N_ITEMS, size=3, replace=False).tolist())
        ptr[j + 1] = len(pitems)
    ptr[-1] = ptr[-2]
    model.set_positives(ptr, np.asarray(pitems, dtype=np.int32))
    for step in range(2):
        model.set_pool(rng.choice(N_ITEMS, size=thv.S_POOL, replace=False).astype(np.int32))
        gu = [rng.integers(0, len(np.arange(g, N_USERS, world)), size=B_LOC) * world + g for g in range(world)]
        gi = [rng.integers(0, N_ITEMS, size=B_LOC) for g in range(world)]
        model.step(gu[rank].astype(np.int32), gi[rank].astype(np.int32))
    g = model.gather_global_tables()
    L2, _ = thv._latents(g['item'], g['item_bias'], g['token'], g['token_bias'], bags)
    assert not np.array_equal(L2, L)                                        # the steps did move the latents
    check(L2)
    assert view.n_refresh == 2 and view.steps == model.steps


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from arx.dist import ShardedHMF, ShardedW2V
    from numpy_backend_similar import NumpySimilarBackend
    E = _table()
    rng = np.random.default_rng(7)
    U = (rng.integers(-2, 3, size=(N_USERS, D)) / 2.0).astype(np.float32)
    b = (rng.integers(-4, 5, size=N_ITEMS) / 4.0).astype(np.float32)         # (a bias: it plays no part)
    model = ShardedHMF(N_USERS, N_ITEMS, D, B_LOC, 8, 0.5, rank, world, 'cpu', backend=NumpySimilarBackend(),
                       tables={'user': U, 'item': E, 'item_bias': b})
    _check_exact(model, E, rank, world)
    ctx = (rng.integers(-2, 3, size=(N_ITEMS, D)) / 2.0).astype(np.float32)
    w2v = ShardedW2V(N_USERS, N_ITEMS, D, B_LOC, 8, 2, 0.5, rank, world, 'cpu', backend=NumpySimilarBackend(),
                     tables={'userembed_cat_0': U, 'itemembed_cat_0': ctx, 'item_outputembed_cat_0': E,
                             'item_output_bias_cat_0': b})
    _check_exact(w2v, E, rank, world)                                       # over the OUTPUT table
    for cls_name in ('ShardedHMFRepTokens', 'ShardedHMFBags'):
        _check_view(cls_name, rank, world)
    dist.barrier()
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_sharded_similar_items_match_global_cosine_topk_gloo(tmp_path, world):
    import torch.multiprocessing as mp
    port = 34300 + 10 * world + (os.getpid() % 50) * 40
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(world))
