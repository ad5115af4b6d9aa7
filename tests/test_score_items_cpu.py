"""score_items without a GPU: the ABI of include/arx_slate.h against SLATE_PROTOTYPES by type, argument validation of the
two exports before any HIP call, the host rules of arx/slate.py, the float64 oracle against a brute-force loop, and the
sharded flow of arx.dist (gloo worlds of 2 and 3 ranks with a numpy compute double, tests/numpy_backend_slate.py)
against the single-process oracle over the WHOLE table -- table entries are small dyadic numbers, so every score is
exact in float32 and equality is exact."""
import os
import sys

import numpy as np
import pytest

import slate_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["arx_slate_merge_shards", "arx_slate_scores"]


# ---------------------------------------------------------------- 1. the ABI
def test_slate_header_and_its_table_stay_in_step():
    """include/arx_slate.h against SLATE_PROTOTYPES of arx/_lib.py by TYPE, with the parser and the comparator of
    tests/test_abi_signatures_cpu.py; both names are exported by the library, arx.h includes the header, and neither
    name is in PROTOTYPES."""
    import test_abi_signatures_cpu as A
    from arx import _lib
    decls = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_slate.h")).read())
    assert sorted(decls) == NAMES
    lines = open(os.path.join(A.ROOT, "a-recsys_amd", "arx", "_lib.py")).read().split("\n")
    end = next(i for i, l in enumerate(lines) if l.startswith("class ArxError"))
    ns = {"__file__": "_lib.py"}
    exec(compile("\n".join(l for l in lines[:end] if not l.startswith("import torch")), "_lib.py(slate)", "exec"), ns)
    protos = ns["SLATE_PROTOTYPES"]
    assert sorted(protos) == sorted(decls) == sorted(_lib.SLATE_PROTOTYPES)
    bad = [m for name in sorted(decls) for m in A.mismatches(name, decls[name], protos[name])]
    assert not bad, "\n".join(bad)
    # not vacuous: one i64 narrowed to i32 is reported
    for name in NAMES:
        res, args = protos[name]
        k64 = next(k for k, a in enumerate(args) if a is A.C.c_int64)
        narrowed = list(args)
        narrowed[k64] = A.C.c_int32
        assert any("parameter %d " % k64 in m for m in A.mismatches(name, decls[name], (res, narrowed)))
    for name in decls:
        assert hasattr(_lib.lib, name) and name not in _lib.PROTOTYPES and name not in _lib.TAGS_PROTOTYPES
        assert getattr(_lib.lib, name).argtypes == list(protos[name][1])
    assert '#include "arx_slate.h"' in open(os.path.join(A.ROOT, "include", "arx.h")).read()
    assert len(A.load_prototypes()) == A.N_ENTRY_POINTS


# ---------------------------------------------------------------- 2. argument validation
def test_slate_exports_validate_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib
    EINVAL, EUNSUPPORTED = -1, -4

    def err():
        m = lib.arx_last_error()
        return m.decode() if m else ""
    # (pointers are only compared with NULL and checked for alignment before the first HIP call: multiples of 16
    # stand in for them)
    P = 4096

    def sc(U=P, ldu=64, B=8, Pm=P, ldp=64, pbias=P, V=100, d=64, cand=P, ldc=10, C=10, out=P, lds=10):
        return lib.arx_slate_scores(U, ldu, B, Pm, ldp, pbias, V, d, cand, ldc, C, out, lds, None)
    for kw in (dict(U=None), dict(Pm=None), dict(cand=None), dict(out=None), dict(d=0), dict(d=2), dict(d=6),
               dict(ldu=60), dict(ldp=66), dict(ldu=66), dict(ldp=32), dict(U=P + 4), dict(Pm=P + 8), dict(ldc=9),
               dict(lds=9), dict(B=-1), dict(C=-1), dict(V=-1), dict(V=2 ** 31), dict(B=2 ** 16, C=2 ** 15, ldc=2 ** 15,
                                                                                       lds=2 ** 15)):
        assert sc(**kw) == EINVAL and "arx_slate_scores" in err(), kw
    assert sc(d=260, ldu=260, ldp=260) == EUNSUPPORTED and "arx_slate_scores" in err()
    assert sc(B=0) == 0 and sc(C=0) == 0 and sc(B=0, pbias=None) == 0
    assert sc(B=0, C=2 ** 40, ldc=2 ** 40, lds=2 ** 40) == 0              # (nothing to do is not a size violation)

    def mg(parts=P, B=8, C=10, W=3, out=P, ldo=10):
        return lib.arx_slate_merge_shards(parts, B, C, W, out, ldo, None)
    for kw in (dict(parts=None), dict(out=None), dict(W=0), dict(W=65), dict(W=-1), dict(B=-1), dict(C=-1),
               dict(ldo=9), dict(B=2 ** 16, C=2 ** 15, ldo=2 ** 15)):
        assert mg(**kw) == EINVAL and "arx_slate_merge_shards" in err(), kw
    assert mg(B=0) == 0 and mg(C=0) == 0


# ---------------------------------------------------------------- 3. host rules
def test_check_slate_and_check_k():
    import torch
    from arx.slate import check_k, check_slate
    V, rows = 10, 3
    good = np.array([[0, 9, -1, 4], [-1, -1, -1, -1], [3, 3, 3, 0]])
    for form in (good, good.astype(np.int32), good.tolist(), torch.from_numpy(good), good.astype(np.uint8) % 10):
        out = check_slate(form, rows, V)
        assert out.dtype == np.int32 and out.flags['C_CONTIGUOUS'] and out.shape == (3, 4)
    np.testing.assert_array_equal(check_slate(good, rows, V), good)
    np.testing.assert_array_equal(check_slate(good.T[:, :3].T[:, ::2], rows, V), good[:, ::2])    # a strided view
    assert check_slate(np.zeros((0, 5), dtype=np.int64), 0, V).shape == (0, 5)       # a rank without users
    bad = [good[0], good[None], good[:2], good.astype(np.float32), good >= 0, np.zeros((rows, 0), dtype=np.int64)]
    for v in (-2, V, 2 ** 31):
        b = good.copy()
        b[2, 1] = v
        bad.append(b)
    for b in bad:
        with pytest.raises(ValueError, match="score_items"):
            check_slate(b, rows, V)
    assert check_k(None, 5) is None and check_k(5, 5) == 5 and check_k(np.int64(1), 5) == 1
    assert check_k(1024, 5000) == 1024
    for k in (0, -1, 6, 2.0, True, "3"):
        with pytest.raises(ValueError):
            check_k(k, 5)
    with pytest.raises(ValueError):
        check_k(1025, 5000)


# ---------------------------------------------------------------- 4. the oracle
def test_oracle_matches_a_brute_force_loop():
    rng = np.random.default_rng(3)
    B, C, V, d = 4, 12, 9, 8
    U, P, b = SO.dyadic(rng, B, V, d)
    cand = SO.slate(rng, B, C, V)
    cand[0, :4] = [5, 5, -1, 5]                          # duplicates around an empty slot
    cand[1, 0], cand[1, 1] = V, SO.KEY_NONE
    for bias in (b, None):
        got = SO.scores(U, P, bias, cand)
        for r in range(B):
            for j in range(C):
                c = int(cand[r, j])
                if 0 <= c < V:
                    want = sum(float(U[r, i]) * float(P[c, i]) for i in range(d)) + (float(b[c]) if bias is not None else 0.0)
                else:
                    want = -np.inf
                assert got[r, j] == want, (r, j)
    sc = SO.scores(U, P, b, cand)
    assert np.isneginf(sc[B - 1]).all() and sc[0, 0] == sc[0, 1] == sc[0, 3]
    k = 7
    ids, vals = SO.order(sc, cand, k)
    for r in range(B):
        live = [(-sc[r, j], j) for j in range(C) if sc[r, j] > -np.inf]
        live.sort()
        want_i = [int(cand[r, j]) for _, j in live[:k]] + [-1] * max(0, k - len(live))
        want_v = [-s for s, _ in live[:k]] + [-np.inf] * max(0, k - len(live))
        assert ids[r].tolist() == want_i and vals[r].tolist() == want_v
    assert (ids[B - 1] == -1).all()
    a = SO.abs_scores(U, P, b, cand)
    assert (a >= np.abs(np.where(np.isneginf(sc), 0.0, sc))).all() and not a[B - 1].any()


# ---------------------------------------------------------------- 5. the sharded flow
N_USERS, N_ITEMS, D, B_LOC, C_SLATE, K = 23, 37, 16, 6, 9, 5


def _tables():
    rng = np.random.default_rng(7)                      # the same tables on every rank
    U, I, b = SO.dyadic(rng, N_USERS, N_ITEMS, D)
    Cx = (rng.integers(-2, 3, size=(N_ITEMS, D)) / 2.0).astype(np.float32)
    return U, I, b, Cx


def _slates(users):
    """One slate per GLOBAL user (so every rank can compute every row's oracle): items of every owner, a duplicate,
    -1 slots; the first user of a rank has an all-empty row."""
    out = np.zeros((len(users), C_SLATE), dtype=np.int64)
    for j, u in enumerate(users):
        r = np.random.default_rng(1000 + int(u))
        row = r.integers(0, N_ITEMS, size=C_SLATE)
        row[:3] = [(3 * int(u)) % N_ITEMS, (3 * int(u) + 1) % N_ITEMS, (3 * int(u) + 2) % N_ITEMS]    # three owners
        row[5] = row[1]                                  # a duplicate
        row[[4, 7]] = -1
        out[j] = row if j else -1
    return out


def _check(model, call, lat, I, b, users):
    cand = _slates(users)
    want = SO.scores(lat, I, b, cand).astype(np.float32)                  # exact
    got = call(cand, None)
    assert got.dtype.is_floating_point and tuple(got.shape) == (len(users), C_SLATE)
    np.testing.assert_array_equal(got.numpy(), want)
    ids, vals = call(cand, K)
    wi, wv = SO.order(want, cand, K)
    np.testing.assert_array_equal(ids.numpy(), wi)
    np.testing.assert_array_equal(vals.numpy(), wv)
    if len(users):
        assert (wi[0] == -1).all() and (wi[1:, -1] >= 0).all() and (wi[1:] >= 0).all()
    ids1, _ = call(cand[:, :4], 4)                                        # a second (C, k): its own buffers
    np.testing.assert_array_equal(ids1.numpy(), SO.order(want[:, :4], cand[:, :4], 4)[0])
    np.testing.assert_array_equal(call(cand, None).numpy(), want)         # and the first again
    for bad_k in (0, C_SLATE + 1):
        with pytest.raises(ValueError):
            call(cand, bad_k)
    bad = cand.copy()
    if len(users):
        bad[0, 0] = N_ITEMS
        with pytest.raises(ValueError):
            call(bad, None)
        with pytest.raises(ValueError):
            call(cand[:-1], None)


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from arx.dist import ShardedHMF, ShardedW2V
    from numpy_backend_slate import SlateBackend

    U, I, b, Cx = _tables()
    own = np.arange(rank, N_USERS, world)
    users = own[:B_LOC - 1] if rank != world - 1 else own[:0]             # the last rank asks for nobody
    model = ShardedHMF(N_USERS, N_ITEMS, D, B_LOC, 8, 0.5, rank, world, 'cpu', backend=SlateBackend(),
                       tables={'user': U, 'item': I, 'item_bias': b})
    _check(model, lambda c, k: model.score_items(users, c, k=k), U[users], I, b, users)
    with pytest.raises(ValueError):
        model.score_items(own[:B_LOC + 1], np.zeros((B_LOC + 1, C_SLATE), dtype=np.int64))
    if world > 1:
        with pytest.raises(ValueError):
            model.score_items([(rank + 1) % world], np.zeros((1, C_SLATE), dtype=np.int64))     # not this rank's user

    n_in = 2
    w2v = ShardedW2V(N_USERS, N_ITEMS, D, B_LOC, 8, n_in, 0.5, rank, world, 'cpu', backend=SlateBackend(),
                     tables={'userembed_cat_0': U, 'itemembed_cat_0': Cx, 'item_outputembed_cat_0': I,
                             'item_output_bias_cat_0': b})
    ctx = np.stack([(5 * users + 1) % N_ITEMS, (7 * users + 2) % N_ITEMS]).astype(np.int64).reshape(n_in, len(users))
    lat = 0.5 * U[users].astype(np.float64) + (0.5 / n_in) * (Cx[ctx[0]].astype(np.float64) + Cx[ctx[1]])
    _check(w2v, lambda c, k: w2v.score_items(users, ctx, c, k=k), lat, I, b, users)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_score_items_matches_global_oracle_gloo(tmp_path, world):
    import torch.multiprocessing as mp
    port = 33900 + 10 * world + (os.getpid() % 50) * 40
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(world))


def test_bag_models_score_through_item_view_only():
    """The two HET training classes raise NotImplementedError naming item_view(); the view inherits ShardedHMF's
    method and refreshes in its own _score_items."""
    from arx.dist import ShardedHMF, ShardedHMFBags, ShardedHMFRepTokens, ShardedHetView
    for cls in (ShardedHMFBags, ShardedHMFRepTokens):
        with pytest.raises(NotImplementedError, match="item_view"):
            cls.score_items(object.__new__(cls), [0], [[0]])
    assert ShardedHetView.score_items is ShardedHMF.score_items
    assert ShardedHetView._score_items is not ShardedHMF._score_items
