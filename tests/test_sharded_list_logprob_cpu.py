"""ShardedHMF.list_logprob without a GPU: gloo worlds of 2 and 3 ranks with a numpy compute double of the two new stages
(tests/numpy_backend_list.py on top of tests/numpy_backend_sample.py), against ONE global oracle over global ids
(tests/list_logprob_oracle.py on the exact global logits): uneven shards, uneven asks including a rank without users,
per-user temperatures, lists that hold every reason code with entries owned by every shard; a list the model drew itself
comes back with its logged propensities bit for bit.  The host-side checks (every error before any collective), the
parameter lists, the ABI of include/arx_list_logp_shard.h against LIST_LOGP_SHARD_PROTOTYPES by type, and argument
validation of the two entries before any HIP call."""
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["arx_list_logp_merge_shards", "arx_list_logp_prepare_shard"]
EINVAL = -1


def check(name, L, lists, tau, filt, glp, gv, gwhy):
    """codes exact; logp within the oracle's own tolerance at the drawable entries, -inf at the codes 2-6, 0 at -1;
    values the bits of L at the drawable entries, -inf elsewhere"""
    import list_logprob_oracle as LL
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
    return codes


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from arx.dist import ShardedHMF
    from arx.utils.ope import list_weights
    from numpy_backend_list import ListRecBackend
    import list_logprob_oracle as LL

    n_users, n_items, d, B_loc = 23, 37, 16, 6                    # 37 items: uneven shards in both worlds
    rng = np.random.default_rng(7)                               # the same tables on every rank
    U = (rng.integers(-2, 3, size=(n_users, d)) / 2.0).astype(np.float32)
    I = (rng.integers(-2, 3, size=(n_items, d)) / 2.0).astype(np.float32)
    b = (rng.integers(-4, 5, size=n_items) / 4.0).astype(np.float32)
    dead = [30, 31, 32]                                          # one item per shard (worlds 2 and 3) never scores
    b[dead] = -np.inf
    tags = rng.integers(0, 16, n_items).astype(np.uint32)
    tags[dead] = 15
    model = ShardedHMF(n_users, n_items, d, B_loc, 8, 0.5, rank, world, 'cpu', backend=ListRecBackend(),
                       tables={'user': U, 'item': I, 'item_bias': b})
    own = np.arange(rank, n_users, world)
    users = own[:B_loc - (rank % 2)] if rank != world - 1 else own[:0]     # uneven asks; the last rank asks for nobody
    n = len(users)
    with np.errstate(invalid='ignore'):
        logits = (U.astype(np.float64) @ I.astype(np.float64).T + b.astype(np.float64)).astype(np.float32)   # exact
    L = logits[users]
    tau_u = np.random.default_rng(3).choice([0.25, 1.0, 3.0], n_users).astype(np.float32)
    tau = tau_u[users]

    # ---- every check runs before any collective: a rank that raises has not entered one (the others never call)
    k = 14
    good = np.zeros((n, k), dtype=np.int64)
    for bad in (dict(sample_temperature=0.0), dict(sample_temperature=-1.0), dict(sample_temperature=float('nan')),
                dict(sample_temperature=[1.0] * (n + 1)), dict(sample_temperature=None)):
        with pytest.raises(ValueError):
            model.list_logprob(users, good, **bad)
    for bad in (np.zeros((n + 1, k), dtype=np.int64), np.zeros((n, 0), dtype=np.int64),
                np.zeros((n, 1025), dtype=np.int64), np.zeros((n, k)), np.zeros(n, dtype=np.int64)):
        with pytest.raises(ValueError):
            model.list_logprob(users, bad, 1.0)
    with pytest.raises(ValueError):
        model.list_logprob(users, good, 1.0, exclude_seen=True)               # nothing prepared
    with pytest.raises(ValueError):
        model.list_logprob(users, good, 1.0, tags_any=1)                      # nothing prepared
    with pytest.raises(ValueError):
        model.list_logprob(np.arange(B_loc + 1) * world + rank, np.zeros((B_loc + 1, k), dtype=np.int64), 1.0)
    with pytest.raises(ValueError):
        model.list_logprob([(rank + 1) % world], np.zeros((1, k), dtype=np.int64), 1.0)     # not this rank's user

    # ---- no filters: every code but EXCLUDED / TAGS, entries of every shard; per-user temperatures
    def foreign(rr, ex_rows=None, bad_tag=None):
        ls = np.stack([rr.permutation(n_items)[:k] for _ in range(n)]) if n else np.zeros((0, k), dtype=np.int64)
        for r in range(n):
            ls[r, 1] = -1
            ls[r, 3] = n_items + r                               # RANGE
            ls[r, 4] = -7
            ls[r, 6] = ls[r, 0]                                  # REPEAT (whoever owns entry 0)
            ls[r, 7] = dead[r % 3]                               # NOSCORE
            ls[r, 8] = dead[r % 3]                               # ... and its second copy is a REPEAT
            for src, at in ((ex_rows, 9), (bad_tag, 11)):        # two entries each, of the owners r and r + 1 (mod W)
                for j in range(2):
                    mine = [c for c in src[r] if c % world == (r + j) % world] if src is not None else []
                    if mine:
                        ls[r, at + j] = mine[0]
        if n > 1:
            ls[1] = -1                                           # an empty row
        if n > 2:
            ls[2, :] = 2 ** 31 - 1                               # nothing in range
        return ls

    lists = foreign(np.random.default_rng(100 + rank))
    lp, vals, why = model.list_logprob(users, lists, tau, return_values=True, return_why=True)
    assert tuple(lp.shape) == (n, k) and lp.dtype.is_floating_point and tuple(why.shape) == (n, k)
    codes = check("world %d rank %d plain" % (world, rank), L, lists, tau, {}, lp.numpy(), vals.numpy(), why.numpy())
    if n:
        assert set(codes.ravel().tolist()) == {LL.OK, LL.EMPTY, LL.RANGE, LL.REPEAT, LL.NOSCORE}
        owners = set((lists[codes == LL.OK] % world).tolist())
        assert owners == set(range(world))                       # drawable entries of every shard
    only = model.list_logprob(users, lists, 0.5)                 # one number; the bare result
    assert tuple(only.shape) == (n, k)
    check("one tau", L, lists, np.full(n, 0.5, dtype=np.float32), {}, only.numpy(),
          model.list_logprob(users, lists, 0.5, return_values=True)[1].numpy(),
          model.list_logprob(users, lists, 0.5, return_why=True)[1].numpy())

    # ---- a list the model drew itself: logged propensities and values come back bit for bit; the weight is 1
    ids, v0, lp0 = model.recommend_sampled(users, 12, return_values=True, sample_temperature=tau, sample_seed=11,
                                           return_logprob=True)
    lp1, v1, why1 = model.list_logprob(users, ids, tau, return_values=True, return_why=True)
    np.testing.assert_array_equal(lp1.numpy(), lp0.numpy())
    np.testing.assert_array_equal(v1.numpy(), v0.numpy())
    assert (why1.numpy() == LL.OK).all()
    assert (list_weights(lp1.numpy(), lp0.numpy()) == 1.0).all()

    # ---- exclusions + tags: every code, each decided by the entry's owner
    model.prepare_item_tags(tags)
    hist = [{int(u): np.random.default_rng(500 + int(u)).integers(0, n_items, size=10).tolist()
             for u in np.arange(g, n_users, world)} for g in range(world)]
    model.prepare_recommend_exclusions(hist[rank])
    wr = np.random.default_rng(99)
    any_u = wr.integers(1, 16, n_users).astype(np.uint32)
    all_u = wr.integers(0, 4, n_users).astype(np.uint32)
    any_u[::4] = 0
    ex_rows = [sorted(set(hist[rank][int(u)])) for u in users]
    import tags_oracle as T
    tag_ok = T.eligible(tags, any_u[users], all_u[users]) if n else np.zeros((0, n_items), dtype=bool)
    bad_tag = [[c for c in np.nonzero(~tag_ok[r])[0].tolist() if c not in ex_rows[r]] for r in range(n)]
    filt = dict(tags=tags, want_any=any_u[users], want_all=all_u[users], ex_lists=ex_rows)
    lists = foreign(np.random.default_rng(200 + rank), ex_rows, bad_tag)
    lp, vals, why = model.list_logprob(users, lists, tau, exclude_seen=True, tags_any=any_u[users],
                                       tags_all=all_u[users], return_values=True, return_why=True)
    codes = check("world %d rank %d filtered" % (world, rank), L, lists, tau, filt, lp.numpy(), vals.numpy(),
                  why.numpy())
    if n:
        assert set(codes.ravel().tolist()) == set(range(7))
        for c in (LL.EXCLUDED, LL.TAGS):
            assert len(set((lists[codes == c] % world).tolist())) == world      # decided on every shard
    ids, v0, lp0 = model.recommend_sampled(users, 12, exclude_seen=True, return_values=True, tags_any=any_u[users],
                                           tags_all=all_u[users], sample_temperature=tau, sample_seed=21,
                                           return_logprob=True)
    lp1, v1 = model.list_logprob(users, ids, tau, exclude_seen=True, tags_any=any_u[users], tags_all=all_u[users],
                                 return_values=True)
    np.testing.assert_array_equal(lp1.numpy(), lp0.numpy())
    np.testing.assert_array_equal(v1.numpy(), v0.numpy())
    # another k right after: nothing stale
    lists = foreign(np.random.default_rng(300 + rank))[:, :9]
    lp, vals, why = model.list_logprob(users, lists, tau, return_values=True, return_why=True)
    check("k 9", L, lists, tau, {}, lp.numpy(), vals.numpy(), why.numpy())
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_list_logprob_matches_global_oracle_gloo(tmp_path, world):
    import torch.multiprocessing as mp
    port = 35900 + 10 * world + (os.getpid() % 50) * 40
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(world))


def test_parameter_lists_and_the_bag_models():
    from arx.dist import HipBackend, ShardedHMF, ShardedHetView, ShardedHMFBags, ShardedHMFRepTokens, ShardedW2V
    tail = ['lists', 'sample_temperature', 'exclude_seen', 'tags_any', 'tags_all', 'return_values', 'return_why']
    for cls in (ShardedHMF, ShardedHetView):
        p = inspect.signature(cls.list_logprob).parameters
        assert list(p)[1:] == ['users'] + tail
        assert p['exclude_seen'].default is False and p['tags_any'].default is None and p['tags_all'].default is None
        assert p['return_values'].default is False and p['return_why'].default is False
        assert 'sample_seed' not in p                             # the noise plays no part in a propensity
    assert list(inspect.signature(ShardedW2V.list_logprob).parameters)[1:] == ['users', 'context'] + tail
    for cls in (ShardedHMFBags, ShardedHMFRepTokens):
        with pytest.raises(NotImplementedError, match=r"item_view\(\)\.list_logprob"):
            cls.list_logprob(object.__new__(cls), [0], [[1]], 1.0)
    # recommend / recommend_sampled keep their parameter lists
    plain = ['users', 'k', 'exclude_seen', 'return_values', 'tags_any', 'tags_all']
    new = ['sample_temperature', 'sample_seed', 'return_logprob']
    for cls in (ShardedHMF, ShardedHetView):
        assert list(inspect.signature(cls.recommend).parameters)[1:] == plain
        assert list(inspect.signature(cls.recommend_sampled).parameters)[1:] == plain + new
    assert list(inspect.signature(ShardedW2V.recommend).parameters)[1:] == ['users', 'context'] + plain[1:]
    assert list(inspect.signature(ShardedW2V.recommend_sampled).parameters)[1:] == ['users', 'context'] + plain[1:] + new
    assert list(inspect.signature(HipBackend.shard_rest_mass).parameters)[1:12] == \
        ['U', 'E', 'bias', 'ex', 'picks', 'world', 'shard', 'sample', 'packed', 'P_max', 'tags']
    for name in ('shard_list_prepare', 'list_logp_merge_shards', 'list_logp_stamp'):
        assert callable(getattr(HipBackend, name))


def test_numpy_double_of_prepare_at_one_shard_is_the_single_device_rule():
    """prepare_shard at (1, 0) against tests/list_logprob_oracle.py's codes (all but NOSCORE, which only the stamp
    knows), and the merge over 3 shards puts the owners' verdicts together to the same codes."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import list_logprob_oracle as LL
    from numpy_backend_list import merge_shards, prepare_shard
    rng = np.random.default_rng(5)
    V, B, k = 50, 7, 20
    lists = rng.integers(-3, V + 3, size=(B, k))
    tags = rng.integers(0, 8, V).astype(np.uint32)
    wa, wl = rng.integers(0, 8, B).astype(np.uint32), rng.integers(0, 2, B).astype(np.uint32)
    ex_rows = [sorted(set(rng.integers(0, V, 6).tolist())) for _ in range(B)]
    L = np.zeros((B, V), dtype=np.float32)
    exp = LL.why(L, lists, tags, wa, wl, ex_rows)
    assert set(exp.ravel().tolist()) == set(range(6))

    def csr(W, s):
        rows = [[c // W for c in row if c % W == s] for row in ex_rows]
        ptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int32)
        cols = np.array([c for x in rows for c in x] + [0], dtype=np.int32)
        return (np.arange(B, dtype=np.int32), B, ptr, cols)

    clean, codes, pc, ps = prepare_shard(lists, V, 1, 0, csr(1, 0), (tags.view(np.int32), wa.view(np.int32),
                                                                      wl.view(np.int32), B))
    np.testing.assert_array_equal(codes, exp)
    np.testing.assert_array_equal(clean, LL.clean(lists, exp))
    slabs = np.stack([prepare_shard(lists, V, 3, s, csr(3, s), (tags[s::3].view(np.int32), wa.view(np.int32),
                                                                wl.view(np.int32), B))[1] for s in range(3)])
    cl, why = merge_shards(lists, V, slabs)
    np.testing.assert_array_equal(why, exp)
    np.testing.assert_array_equal(cl, LL.clean(lists, exp))


def test_list_logp_shard_header_and_its_table_stay_in_step():
    import test_abi_signatures_cpu as A
    from arx import _lib
    decls = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_list_logp_shard.h")).read())
    assert sorted(decls) == NAMES
    protos = _lib.LIST_LOGP_SHARD_PROTOTYPES
    assert sorted(protos) == NAMES
    bad = [m for name in NAMES for m in A.mismatches(name, decls[name], protos[name])]
    assert not bad, "\n".join(bad)
    others = [getattr(_lib, t) for t in dir(_lib) if t.endswith("PROTOTYPES") and t != "LIST_LOGP_SHARD_PROTOTYPES"]
    assert len(others) >= 9 and _lib.PROTOTYPES in others
    for name in NAMES:                                               # not vacuous: one i64 narrowed to i32 is reported
        res, args = protos[name]
        k64 = next(k for k, a in enumerate(args) if a is A.C.c_int64)
        narrowed = list(args)
        narrowed[k64] = A.C.c_int32
        assert any("parameter %d " % k64 in m for m in A.mismatches(name, decls[name], (res, narrowed)))
        assert hasattr(_lib.lib, name) and getattr(_lib.lib, name).argtypes == list(args)
        assert all(name not in t for t in others)
    assert len(_lib.PROTOTYPES) == A.N_ENTRY_POINTS
    assert '#include "arx_list_logp_shard.h"' in open(os.path.join(A.ROOT, "include", "arx.h")).read()
    # arx_list_logp.h keeps its two signatures
    d2 = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_list_logp.h")).read())
    assert sorted(d2) == sorted(_lib.LIST_LOGP_PROTOTYPES)
    assert not [m for name in d2 for m in A.mismatches(name, d2[name], _lib.LIST_LOGP_PROTOTYPES[name])]


def _err(lib):
    m = lib.arx_last_error()
    return m.decode() if m else ""


def test_shard_entries_validate_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib
    A = 4096                                  # stands in for a device pointer: only compared with NULL

    def prep(ls=A, ldl=8, B=4, k=8, V=100, W=3, s=2, keys=None, key_rows=0, ptr=None, cols=None, tags=None, wa=None,
             wl=None, want_rows=0, cl=A, ldc=8, why=A, ldw=8, pc=A, ps=A, ldp=8):
        return lib.arx_list_logp_prepare_shard(ls, ldl, B, k, V, W, s, keys, key_rows, ptr, cols, tags, wa, wl,
                                               want_rows, cl, ldc, why, ldw, pc, ps, ldp, None)
    wide = dict(ldl=2000, ldc=2000, ldw=2000, ldp=2000)
    for kw, text in ((dict(ls=None), "null"), (dict(cl=None), "null"), (dict(why=None), "null"), (dict(pc=None), "null"),
                     (dict(ps=None), "null"), (dict(B=-1), "B >= 0"), (dict(k=0), "1 <= k <= 1024"),
                     (dict(k=1025, **wide), "1 <= k <= 1024"), (dict(ldl=7), ">= k"), (dict(ldc=7), ">= k"),
                     (dict(ldw=7), ">= k"), (dict(ldp=7), ">= k"), (dict(V=0), "0 < V"), (dict(V=2 ** 31), "0 < V"),
                     (dict(W=0), "0 <= s < W"), (dict(s=3), "0 <= s < W"), (dict(s=-1), "0 <= s < W"),
                     (dict(keys=A), "go together"), (dict(ptr=A, cols=A), "go together"),
                     (dict(keys=A, ptr=A, cols=A, key_rows=0), "key_rows > 0"), (dict(tags=A), "go together"),
                     (dict(wa=A, wl=A), "go together"), (dict(tags=A, wa=A, wl=A, want_rows=0), "want_rows > 0")):
        assert prep(**kw) == EINVAL, kw
        assert "arx_list_logp_prepare_shard" in _err(lib) and text in _err(lib), (kw, _err(lib))
    assert prep(B=0) == 0 and prep(B=0, k=1024, **wide) == 0

    def merge(ls=A, ldl=8, B=4, k=8, V=100, cd=A, ldcode=24, slab=96, W=3, cl=A, ldc=8, why=A, ldw=8):
        return lib.arx_list_logp_merge_shards(ls, ldl, B, k, V, cd, ldcode, slab, W, cl, ldc, why, ldw, None)
    for kw, text in ((dict(ls=None), "null"), (dict(cd=None), "null"), (dict(cl=None), "null"), (dict(why=None), "null"),
                     (dict(B=-1), "B >= 0"), (dict(k=0), "1 <= k <= 1024"), (dict(V=0), "0 < V_global"),
                     (dict(W=0), "1 <= W <= 64"), (dict(W=65), "1 <= W <= 64"), (dict(ldl=7), ">= k"),
                     (dict(ldcode=7), ">= k"), (dict(ldc=7), ">= k"), (dict(ldw=7), ">= k"), (dict(slab=-1), "slab >= 0")):
        assert merge(**kw) == EINVAL, kw
        assert "arx_list_logp_merge_shards" in _err(lib) and text in _err(lib), (kw, _err(lib))
    assert merge(B=0) == 0
