"""Full-vocabulary evaluation of the row-sharded HMF model (arx.dist.ShardedHMF.evaluate) without a GPU: gloo worlds of
2, 3 and 4 ranks with numpy doubles of the two evaluation stages (HipBackend.shard_eval / eval_merge_shards), against a
float64 oracle over the GLOBAL tables -- n_items not divisible by the world, item rows equal to a target's row on
another shard (ties: they never count toward true_rank), a rank without rows, a user listed twice, targets inside and
outside the user's eval positives, positive sets with duplicates or entirely on one shard, all three losses with
return_rows, and a second prepare_eval_positives that replaces the first.  Table entries are small dyadic numbers:
every score is exact in float32 and float64, so ties are real ties and true_rank compares exactly.  Also every
ValueError of the interface, the NotImplementedError of the bag models and the argument checks of the three new
entry points (no launch needed)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(ROOT)


def oracle_eval(U, I, b, users, items, loss, pos):
    """per-row float64 results by the definitions of ShardedHMF.evaluate: 'ce' / 'warp' -> [n] losses,
    'warp_eval' -> ([n] margin_rank, [n] true_rank)."""
    x_all = U.astype(np.float64) @ I.astype(np.float64).T + b.astype(np.float64)[None, :]
    out, ranks = [], []
    for u, i in zip(users, items):
        x = x_all[u]
        t = x[i]
        if loss == 'ce':
            m = x.max()
            out.append(m + np.log(np.exp(x - m).sum()) - t)
            continue
        keep = np.ones(len(x), dtype=bool)
        keep[np.asarray(sorted(pos.get(int(u), ())), dtype=np.int64)] = False
        margin = np.maximum(x - t + 1.0, 0.0)[keep].sum()
        gt = (x > t) & keep
        gt[i] = False
        out.append(np.log1p(margin) if loss == 'warp' else margin)
        ranks.append(int(gt.sum()))
    out = np.asarray(out, dtype=np.float64)
    return (out, np.asarray(ranks, dtype=np.int64)) if loss == 'warp_eval' else out


def _backend():
    from numpy_backend import NumpyBackend

    class EvalBackend(NumpyBackend):
        """numpy doubles of HipBackend.shard_eval / eval_merge_shards."""

        def shard_eval(self, U, E, bias, t, tcol, loss, ex, part, cnt):
            u, e, b = (a.numpy().astype(np.float64) for a in (U, E, bias))
            x = u @ e.T + b[None, :]
            B, V = x.shape
            tt = t.numpy().astype(np.float64)
            if loss == 'ce':
                m = x.max(1) if V else np.full(B, -np.inf)
                lse = m + np.log(np.exp(x - m[:, None]).sum(1)) if V else m
                part.numpy()[...] = lse.astype(np.float32)
                return
            keep = np.ones((B, V), dtype=bool)
            if ex is not None:
                keys, key_rows, ptr, cols = (a if isinstance(a, int) else a.numpy() for a in ex)
                for r in range(B):
                    key = int(keys[r % key_rows])
                    if key >= 0:
                        keep[r, cols[ptr[key]:ptr[key + 1]].astype(np.int64)] = False
            m = np.maximum(x - tt[:, None] + 1.0, 0.0)
            gt = x > tt[:, None]
            tc = tcol.numpy().astype(np.int64)
            for r in range(B):
                if 0 <= tc[r] < V:
                    m[r, tc[r]], gt[r, tc[r]] = 1.0, False
            part.numpy()[...] = (m * keep).sum(1).astype(np.float32)
            if loss == 'warp_eval':
                cnt.numpy()[...] = (gt & keep).sum(1).astype(np.int32)

        def eval_merge_shards(self, loss, parts, cnts, t, out, cnt_out):
            p = parts.numpy().astype(np.float64)
            if loss == 'ce':
                m = p.max(0)
                out.numpy()[...] = (m + np.log(np.exp(p - m[None, :]).sum(0)) - t.numpy()).astype(np.float32)
            elif loss == 'warp':
                out.numpy()[...] = np.log1p(p.sum(0)).astype(np.float32)
            else:
                out.numpy()[...] = p.sum(0).astype(np.float32)
                cnt_out.numpy()[...] = cnts.numpy().astype(np.int64).sum(0).astype(np.int32)
    return EvalBackend()


N_USERS, N_ITEMS, D, B_LOC = 23, 37, 16, 6          # 37 % W != 0 for W = 2, 3, 4
TIES = ((5, 6), (11, 8), (20, 33), (2, 15))          # item c gets item a's row and bias: ties on other shards


def tables():
    rng = np.random.default_rng(11)
    U = (rng.integers(-2, 3, size=(N_USERS, D)) / 2.0).astype(np.float32)
    I = (rng.integers(-2, 3, size=(N_ITEMS, D)) / 2.0).astype(np.float32)
    b = (rng.integers(-4, 5, size=N_ITEMS) / 4.0).astype(np.float32)
    for a, c in TIES:
        I[c], b[c] = I[a], b[a]
    return U, I, b


def rows_of(g, world):
    """(users, items) of rank g: rank 0 lists a user twice, the last rank has no rows; targets with ties."""
    own = np.arange(g, N_USERS, world)
    if world > 1 and g == world - 1:
        return own[:0], np.zeros(0, dtype=np.int64)
    users = own[[0, 1, 2, 1]] if g == 0 else own[:B_LOC]
    rng = np.random.default_rng(100 + g)
    items = rng.integers(0, N_ITEMS, size=len(users))
    items[0] = TIES[g % len(TIES)][0]                      # a target with an equal row on another shard
    if len(items) > 2:
        items[2] = TIES[(g + 1) % len(TIES)][1]
    return users, items.astype(np.int64)


def positives(g, world, which):
    """eval positives of rank g's users: duplicates, a set entirely on one shard, the target inside / outside."""
    pos = {}
    users, items = rows_of(g, world)
    tgt = {int(u): int(i) for u, i in zip(users, items)}
    for u in np.arange(g, N_USERS, world):
        r = np.random.default_rng(1000 * which + int(u))
        if which == 0 and u % 4 == 0:
            pos[int(u)] = list(range(1, N_ITEMS, world)) * 2                  # all on shard 1 (if any), twice
        elif which == 0 and u % 4 == 1:
            pos[int(u)] = []                                                  # nothing masked
        else:
            s = r.integers(0, N_ITEMS, size=int(r.integers(1, 9))).tolist()
            pos[int(u)] = s + s[:2]                                           # duplicates
        if int(u) in tgt and (u + which) % 2 == 0:
            pos[int(u)].append(tgt[int(u)])                                   # the target itself is masked
    return pos


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from arx.dist import ShardedHMF

    U, I, b = tables()
    model = ShardedHMF(N_USERS, N_ITEMS, D, B_LOC, 8, 0.5, rank, world, 'cpu', backend=_backend(),
                       tables={'user': U, 'item': I, 'item_bias': b})
    users, items = rows_of(rank, world)
    all_rows = [rows_of(g, world) for g in range(world)]
    all_u = np.concatenate([r[0] for r in all_rows])
    all_i = np.concatenate([r[1] for r in all_rows])
    own = np.arange(rank, N_USERS, world)

    # ---- argument errors (rank-local, before any collective)
    with pytest.raises(ValueError):
        model.evaluate(users, items, loss='warp')                 # no eval positives yet
    with pytest.raises(ValueError):
        model.evaluate(users, items, loss='warp_eval')
    with pytest.raises(ValueError):
        model.evaluate(users, items, loss='mw')                   # unknown loss
    with pytest.raises(ValueError):
        model.evaluate(own[:2], [0], loss='ce')                   # len(users) != len(items)
    with pytest.raises(ValueError):
        model.evaluate(np.resize(own, B_LOC + 1), np.zeros(B_LOC + 1, dtype=np.int64), loss='ce')   # n > B_loc
    with pytest.raises(ValueError):
        model.evaluate([int(own[0]) + 1 if world > 1 else N_USERS], [0], loss='ce')   # a user of another rank
    with pytest.raises(ValueError):
        model.evaluate(own[:1], [N_ITEMS], loss='ce')             # item out of range
    with pytest.raises(ValueError):
        model.evaluate(own[:1], [-1], loss='ce')
    with pytest.raises(ValueError):
        model.prepare_eval_positives({int(own[0]) + 1: [1]} if world > 1 else {N_USERS: [1]})
    with pytest.raises(ValueError):
        model.prepare_eval_positives({int(own[0]): [N_ITEMS]})

    # ---- 'ce' needs no positives
    mean, rows = model.evaluate(users, items, loss='ce', return_rows=True)
    want = oracle_eval(U, I, b, users, items, 'ce', {})
    np.testing.assert_allclose(rows.numpy(), want, rtol=1e-5)
    np.testing.assert_allclose(mean, oracle_eval(U, I, b, all_u, all_i, 'ce', {}).mean(), rtol=1e-5)
    assert isinstance(mean, float) and rows.dtype.is_floating_point and tuple(rows.shape) == (len(users),)

    # ---- an empty dict: the explicit "mask nothing"
    model.prepare_eval_positives({})
    np.testing.assert_allclose(model.evaluate(users, items, loss='warp'),
                               oracle_eval(U, I, b, all_u, all_i, 'warp', {}).mean(), rtol=1e-5)

    def check(pos_all):
        mean, rows = model.evaluate(users, items, loss='warp', return_rows=True)
        np.testing.assert_allclose(rows.numpy(), oracle_eval(U, I, b, users, items, 'warp', pos_all), rtol=1e-5)
        np.testing.assert_allclose(mean, oracle_eval(U, I, b, all_u, all_i, 'warp', pos_all).mean(), rtol=1e-5)
        mr, tr = model.evaluate(users, items, loss='warp_eval')
        wm, wr = oracle_eval(U, I, b, users, items, 'warp_eval', pos_all)
        np.testing.assert_allclose(mr.numpy(), wm, rtol=1e-5)
        np.testing.assert_array_equal(tr.numpy(), wr)
        assert str(mr.dtype) == 'torch.float32' and str(tr.dtype) == 'torch.int32'
        # ('ce' ignores the positives)
        np.testing.assert_allclose(model.evaluate(users, items, loss='ce'),
                                   oracle_eval(U, I, b, all_u, all_i, 'ce', {}).mean(), rtol=1e-5)

    pos = [positives(g, world, 0) for g in range(world)]
    model.prepare_eval_positives(pos[rank])
    pos_all = {u: set(v) for p in pos for u, v in p.items()}
    check(pos_all)
    # the ties are there: a row whose target has an equal row elsewhere would rank 1 higher if ties counted
    x_all = U.astype(np.float64) @ I.astype(np.float64).T + b
    assert any((x_all[u] == x_all[u][i]).sum() > 1 for u, i in zip(all_u, all_i))

    # ... a second set through a (users, ptr, items) CSR triple replaces the first
    pos2 = [positives(g, world, 1) for g in range(world)]
    mine = sorted(pos2[rank])
    ptr = np.concatenate([[0], np.cumsum([len(pos2[rank][u]) for u in mine])]).astype(np.int64)
    its = np.concatenate([np.asarray(pos2[rank][u], dtype=np.int64) for u in mine] + [np.zeros(0, np.int64)])
    model.prepare_eval_positives((np.asarray(mine), ptr, its))
    pos2_all = {u: set(v) for p in pos2 for u, v in p.items()}
    check(pos2_all)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_sharded_evaluate_matches_global_oracle_gloo(tmp_path, world):
    import torch.multiprocessing as mp
    port = 32300 + 10 * world + (os.getpid() % 50) * 40
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(world))


def test_sharded_evaluate_world1_gloo(tmp_path):
    import torch.multiprocessing as mp
    port = 32250 + (os.getpid() % 50) * 40
    mp.spawn(_worker, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    assert os.path.exists(tmp_path / "ok0")


def test_bag_models_have_no_evaluate_yet():
    from arx.dist import ShardedHMFBags, ShardedHMFRepTokens
    for cls in (ShardedHMFBags, ShardedHMFRepTokens):
        with pytest.raises(NotImplementedError):
            cls.evaluate(object.__new__(cls), [0], [0])
        with pytest.raises(NotImplementedError):
            cls.evaluate(object.__new__(cls), [0], [0], loss='warp_eval')


def _lib_err():
    from arx import _lib
    m = _lib.lib.arx_last_error()
    return m.decode() if m else ""


def test_eval_rank_parts_argument_validation_without_gpu():
    """arx_gemm_nt_eval_rank_parts refuses null pointers, empty shapes, K outside {32, 64, 128} and unaligned operands
    before any launch (small integers stand in for device pointers: they are only compared with NULL / checked for
    alignment)."""
    from arx import _lib
    f = _lib.lib.arx_gemm_nt_eval_rank_parts
    ok = dict(A=16, lda=128, M=8, Bm=32, ldb=128, N=100, K=128, bias=0, t=48, tcol=64, rp=80, cp=96, ldl=4)
    order = ('A', 'lda', 'M', 'Bm', 'ldb', 'N', 'K', 'bias', 't', 'tcol', 'rp', 'cp', 'ldl')
    for bad in (dict(A=None), dict(Bm=None), dict(t=None), dict(tcol=None), dict(rp=None), dict(cp=None),
                dict(M=0), dict(N=0), dict(N=2 ** 31), dict(K=48), dict(K=256), dict(A=20), dict(Bm=36),
                dict(lda=130), dict(ldb=126)):
        a = dict(ok, **bad)
        assert f(*[a[k] for k in order], None) == -1, bad
        assert "arx_gemm_nt_eval_rank_parts" in _lib_err()


def test_eval_shard_reduce_argument_validation_without_gpu():
    from arx import _lib
    f = _lib.lib.arx_eval_shard_reduce
    ok = dict(mode=2, parts=16, ldp=4, npart=4, cp=32, ldc=4, U=48, ldu=16, E=64, lde=16, bias=0, d=16, V=10, t=80,
              tcol=96, keys=112, key_rows=8, ptr=128, cols=144, B=0, out=160, cnt_out=176)
    order = tuple(ok)
    for bad in (dict(mode=-1), dict(mode=3), dict(out=None), dict(B=-1), dict(npart=-1), dict(parts=None),
                dict(ldp=3), dict(cnt_out=None), dict(cp=None), dict(ldc=2), dict(t=None), dict(mode=1, t=None),
                dict(key_rows=0), dict(ptr=None), dict(cols=None), dict(U=None), dict(E=None), dict(tcol=None),
                dict(d=0), dict(d=260), dict(d=18), dict(ldu=18), dict(lde=6), dict(U=52), dict(E=68)):
        a = dict(ok, **bad)
        assert f(*[a[k] for k in order], None) == -1, bad
        assert "arx_eval_shard_reduce" in _lib_err()
    assert f(*[ok[k] for k in order], None) == 0                         # B = 0: nothing to do, no launch
    a = dict(ok, mode=0, t=None, keys=None, cp=None, cnt_out=None, U=None, E=None)
    assert f(*[a[k] for k in order], None) == 0                          # ce: no scores, masks or counts needed
    a = dict(ok, npart=0, parts=None, cp=None)
    assert f(*[a[k] for k in order], None) == 0                          # a shard without columns


def test_eval_merge_shards_argument_validation_without_gpu():
    from arx import _lib
    f = _lib.lib.arx_eval_merge_shards
    ok = dict(mode=2, parts=16, cnts=32, t=48, B=0, W=3, out=64, cnt_out=80)
    order = tuple(ok)
    for bad in (dict(mode=-1), dict(mode=3), dict(parts=None), dict(out=None), dict(mode=0, t=None),
                dict(cnts=None), dict(cnt_out=None), dict(W=0), dict(W=65), dict(B=-1)):
        a = dict(ok, **bad)
        assert f(*[a[k] for k in order], None) == -1, bad
        assert "arx_eval_merge_shards" in _lib_err()
    for W in (1, 64):
        assert f(*[dict(ok, W=W)[k] for k in order], None) == 0         # B = 0: nothing to do, no launch
    assert f(*[dict(ok, mode=1, t=None, cnts=None, cnt_out=None)[k] for k in order], None) == 0
