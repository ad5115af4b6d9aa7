"""The serving view of the sharded HET models (arx.dist.ShardedHetView, model.item_view()) without a GPU: gloo worlds
of 2, 3 and 4 ranks, both classes (ShardedHMFBags: token table striped, the latents summed through the reduce-scatter in
several chunks; ShardedHMFRepTokens: token table replicated), with numpy doubles of the compute stages -- the new
het_rows_range beside the recommend / evaluate doubles of the id-only tests -- against float64 oracles over the GLOBAL
latents 1/2 (I + mean tok), 1/2 (b + mean b_tok).  n_items = 37 (not divisible), d = 16, 11 tokens; tables are small
dyadic numbers and bag lengths are drawn from {1, 2, 4, 8}: every mean, every half, every cross-rank partial sum and
every score is exact in float32 and float64, so ties are real ties and ids compare exactly.  Covered: k larger than the
smallest shard, a rank without users, exclusions that leave fewer than k items, the three evaluation losses, the
snapshot semantics (a table row overwritten: stale until refresh()), the auto-refresh after step()s, the four training
methods (TypeError), the training classes' own recommend / evaluate (still NotImplementedError), and the argument
checks of arx_het_rows_range (no launch needed)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_TOK, S_POOL = 11, 8


def _backend():
    import test_sharded_eval_cpu as tec
    import test_sharded_recommend_cpu as trc

    class ViewBackend(type(trc._backend()), type(tec._backend())):
        """The recommend and evaluate doubles of the id-only tests + a numpy double of HipBackend.het_rows_range."""

        def het_rows_range(self, E_id, bias_id, E_tok, bias_tok, vals, starts, lens, n_items, world, rank, c0, c1, out,
                           bias_out=None, all_owners=False, scale=0.5, block_rows=0):
            eid, bid, et, bt = (t.numpy().astype(np.float64) for t in (E_id, bias_id, E_tok, bias_tok))
            v, st, ln = (t.numpy().astype(np.int64) for t in (vals, starts, lens))
            d = eid.shape[1]
            o = out.numpy()
            ob = o[:, d] if bias_out is None else bias_out.numpy()
            assert world == 1 or not all_owners or block_rows >= c1 - c0
            for s in (range(world) if all_owners else [rank]):
                base = s * block_rows if all_owners else 0
                for c in range(c0, c1):
                    g, row = c * world + s, base + c - c0
                    if g >= n_items:
                        o[row, :d], ob[row] = 0.0, 0.0
                        continue
                    tok = v[st[g]:st[g] + ln[g]]
                    r, rb = et[tok].sum(0) / float(ln[g]), bt[tok].sum() / float(ln[g])
                    if s == rank:
                        r, rb = r + eid[c], rb + bid[c]
                    o[row, :d], ob[row] = scale * r, scale * rb
    return ViewBackend()


def _tables(d=None):
    """Dyadic global tables (d wide; default: the width of the id-only CPU tests) and the bag index; items TIES[.][1]
    repeat the id row AND the bag of TIES[.][0]."""
    import test_sharded_eval_cpu as tec
    nu, ni, d = tec.N_USERS, tec.N_ITEMS, d or tec.D
    rng = np.random.default_rng(23)
    U = (rng.integers(-2, 3, size=(nu, d)) / 2.0).astype(np.float32)
    I = (rng.integers(-2, 3, size=(ni, d)) / 2.0).astype(np.float32)
    b = (rng.integers(-4, 5, size=ni) / 4.0).astype(np.float32)
    T = (rng.integers(-2, 3, size=(N_TOK, d)) / 2.0).astype(np.float32)
    bT = (rng.integers(-4, 5, size=N_TOK) / 4.0).astype(np.float32)
    bags = [rng.integers(0, N_TOK, size=int(rng.choice([1, 2, 4, 8]))) for _ in range(ni)]
    for a, c in tec.TIES:
        I[c], b[c], bags[c] = I[a], b[a], bags[a].copy()
    lens = np.asarray([len(x) for x in bags], dtype=np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    vals = np.concatenate(bags).astype(np.int32)
    return U, I, b, T, bT, (vals, starts, lens)


def _latents(I, b, T, bT, bags):
    """float64 global item latents 1/2 (I + mean tok) and biases."""
    vals, starts, lens = bags
    L = np.zeros(I.shape, dtype=np.float64)
    Lb = np.zeros(I.shape[0], dtype=np.float64)
    for g in range(I.shape[0]):
        tok = vals[starts[g]:starts[g] + lens[g]].astype(np.int64)
        L[g] = 0.5 * (I[g].astype(np.float64) + T[tok].astype(np.float64).mean(0))
        Lb[g] = 0.5 * (float(np.asarray(b).reshape(-1)[g]) + np.asarray(bT).reshape(-1)[tok].astype(np.float64).mean())
    return L, Lb


def _history(g, world, n_users, n_items):
    ex = {}
    for u in np.arange(g, n_users, world):
        r = np.random.default_rng(3000 + int(u))
        if u % 5 == 0:
            ex[int(u)] = r.choice(n_items, size=n_items - 4, replace=False).tolist()     # 4 eligible < k
        else:
            ex[int(u)] = r.integers(0, n_items, size=int(r.integers(0, 12))).tolist()
    return ex


def _check_view(cls_name, rank, world):
    import torch
    import torch.distributed as dist
    import test_sharded_eval_cpu as tec
    from test_sharded_recommend_cpu import oracle_recommend
    from arx import dist as adist
    cls = getattr(adist, cls_name)
    n_users, n_items, d, B_loc = tec.N_USERS, tec.N_ITEMS, tec.D, tec.B_LOC
    U, I, b, T, bT, bags = _tables()
    tables = {'user': U, 'item': I, 'item_bias': b, 'token': T, 'token_bias': bT}
    model = cls(n_users, n_items, d, B_loc, S_POOL, 0.5, rank, world, 'cpu', bags, N_TOK, backend=_backend(),
                tables=tables)
    # the training classes themselves still serve nothing
    with pytest.raises(NotImplementedError):
        model.recommend([rank], 3)
    with pytest.raises(NotImplementedError):
        model.evaluate([rank], [0])
    view = model.item_view(chunk_cols=4)                  # Bags: several chunks, the last one short
    assert isinstance(view, adist.ShardedHetView) and isinstance(view, adist.ShardedHMF)
    assert view.E_user is model.E_user and view.E_item is not model.E_item
    assert tuple(view.E_item.shape) == (model.ni_loc + 1, d) and tuple(view.b_item.shape) == (model.ni_loc + 1,)
    for name, args in (('step', ([0], [0])), ('set_pool', ([0] * S_POOL,)), ('prepare_route', ([0], [0])),
                       ('set_positives', ([0, 0], [0]))):
        with pytest.raises(TypeError):
            getattr(view, name)(*args)
    with pytest.raises(TypeError):
        adist.ShardedHetView(adist.ShardedHMF(n_users, n_items, d, B_loc, S_POOL, 0.5, rank, world, 'cpu',
                                              backend=_backend(), tables=tables))

    L, Lb = _latents(I, b, T, bT, bags)
    own = np.arange(rank, n_users, world)
    users = own[:B_loc] if rank != world - 1 else own[:0]           # the last rank asks for nobody
    if rank == 0:
        users = own[[0, 1, 2, 1]]
    k = 12                                                          # > the smallest shard (9 rows at W = 4)

    # ---- recommend (the first call materialises the latents)
    assert view.n_refresh == 0
    got, vals = view.recommend(users, k, return_values=True)
    assert view.n_refresh == 1
    want = oracle_recommend(U, L, Lb, users, k)
    np.testing.assert_array_equal(got.numpy(), want)
    for j, u in enumerate(users):
        x = U[u].astype(np.float64) @ L.T + Lb
        np.testing.assert_array_equal(vals.numpy()[j], x[want[j]].astype(np.float32))
    # the materialised shard itself: exact, a zero row behind it
    ni = model.ni_loc
    np.testing.assert_array_equal(view.E_item.numpy()[:ni], L[rank::world].astype(np.float32))
    np.testing.assert_array_equal(view.b_item.numpy()[:ni], Lb[rank::world].astype(np.float32))
    assert not view.E_item.numpy()[ni].any() and view.b_item.numpy()[ni] == 0
    with pytest.raises(ValueError):
        view.recommend(users, k, exclude_seen=True)                 # nothing prepared yet
    hist = [_history(g, world, n_users, n_items) for g in range(world)]
    view.prepare_recommend_exclusions(hist[rank])
    ex_all = {u: set(v) for h in hist for u, v in h.items()}
    got = view.recommend(users, k, exclude_seen=True).numpy()
    want_ex = oracle_recommend(U, L, Lb, users, k, ex_all)
    np.testing.assert_array_equal(got, want_ex)
    short = [j for j, u in enumerate(users) if u % 5 == 0]
    assert all((want_ex[j, 4:] == -1).all() and (want_ex[j, :4] >= 0).all() for j in short)

    # ---- evaluate: the three losses against the global oracle
    eu, ei = tec.rows_of(rank, world)
    all_rows = [tec.rows_of(g, world) for g in range(world)]
    all_u = np.concatenate([r[0] for r in all_rows])
    all_i = np.concatenate([r[1] for r in all_rows])
    mean, rows = view.evaluate(eu, ei, loss='ce', return_rows=True)
    np.testing.assert_allclose(rows.numpy(), tec.oracle_eval(U, L, Lb, eu, ei, 'ce', {}), rtol=1e-5)
    np.testing.assert_allclose(mean, tec.oracle_eval(U, L, Lb, all_u, all_i, 'ce', {}).mean(), rtol=1e-5)
    with pytest.raises(ValueError):
        view.evaluate(eu, ei, loss='warp')                          # no eval positives yet
    pos = [tec.positives(g, world, 0) for g in range(world)]
    view.prepare_eval_positives(pos[rank])
    pos_all = {u: set(v) for p in pos for u, v in p.items()}
    mean, rows = view.evaluate(eu, ei, loss='warp', return_rows=True)
    np.testing.assert_allclose(rows.numpy(), tec.oracle_eval(U, L, Lb, eu, ei, 'warp', pos_all), rtol=1e-5)
    np.testing.assert_allclose(mean, tec.oracle_eval(U, L, Lb, all_u, all_i, 'warp', pos_all).mean(), rtol=1e-5)
    mr, tr = view.evaluate(eu, ei, loss='warp_eval')
    wm, wr = tec.oracle_eval(U, L, Lb, eu, ei, 'warp_eval', pos_all)
    np.testing.assert_allclose(mr.numpy(), wm, rtol=1e-5)
    np.testing.assert_array_equal(tr.numpy(), wr)
    x_all = U.astype(np.float64) @ L.T + Lb                         # (the ties are there)
    assert any((x_all[u] == x_all[u][i]).sum() > 1 for u, i in zip(all_u, all_i))
    assert view.n_refresh == 1                                      # nothing stepped: one materialisation so far

    # ---- a snapshot: rows written directly show after an explicit refresh() only
    I2, b2, T2, bT2 = I.copy(), b.copy(), T.copy(), bT.copy()
    b2[7] = 256.0                                                   # item 7: everybody's first choice ...
    tok = int(bags[0][bags[1][9]])                                  # ... and a token of item 9 sinks its items
    bT2[tok] = -8.0
    T2[tok] = 1.0
    if 7 % world == rank:
        model.b_item[7 // world] = 256.0
    if cls_name == 'ShardedHMFBags':
        if tok % world == rank:
            model.b_tok[tok // world] = -8.0
            model.E_tok[tok // world] = 1.0
    else:
        model.b_tok[tok] = -8.0
        model.E_tok[tok] = 1.0
    np.testing.assert_array_equal(view.recommend(users, k).numpy(), want)          # stale: the old snapshot
    view.refresh()
    assert view.n_refresh == 2
    L2, Lb2 = _latents(I2, b2, T2, bT2, bags)
    want2 = oracle_recommend(U, L2, Lb2, users, k)
    assert len(users) == 0 or ((want2[:, 0] == 7).all() and not np.array_equal(want2, want))
    np.testing.assert_array_equal(view.recommend(users, k).numpy(), want2)
    mr, tr = view.evaluate(eu, ei, loss='warp_eval')
    wm, wr = tec.oracle_eval(U, L2, Lb2, eu, ei, 'warp_eval', pos_all)
    np.testing.assert_allclose(mr.numpy(), wm, rtol=1e-5)
    np.testing.assert_array_equal(tr.numpy(), wr)

    # ---- two step()s: the next recommend refreshes by itself, once
    rng = np.random.default_rng(77)                                 # the same stream on every rank
    ptr = np.zeros(len(own) + 2, dtype=np.int32)
    pitems = []
    for j, u in enumerate(own):
        pitems.extend(np.random.default_rng(500 + int(u)).choice(n_items, size=3, replace=False).tolist())
        ptr[j + 1] = len(pitems)
    ptr[-1] = ptr[-2]
    model.set_positives(ptr, np.asarray(pitems, dtype=np.int32))
    for step in range(2):
        model.set_pool(rng.choice(n_items, size=S_POOL, replace=False).astype(np.int32))
        gu = [rng.integers(0, len(np.arange(g, n_users, world)), size=B_loc) * world + g for g in range(world)]
        gi = [rng.integers(0, n_items, size=B_loc) for g in range(world)]
        model.step(gu[rank].astype(np.int32), gi[rank].astype(np.int32))
    assert view.n_refresh == 2 and view.steps != model.steps
    got = view.recommend(users, k).numpy()
    assert view.n_refresh == 3 and view.steps == model.steps
    g = model.gather_global_tables()
    L3, Lb3 = _latents(g['item'], g['item_bias'], g['token'], g['token_bias'], bags)
    assert not np.array_equal(L3, L2)                               # the steps did move the latents
    np.testing.assert_array_equal(got, oracle_recommend(g['user'], L3, Lb3, users, k))
    np.testing.assert_array_equal(view.recommend(users, 3).numpy(), got[:, :3])
    assert view.n_refresh == 3                                      # no step since: no second materialisation
    dist.barrier()


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    for cls_name in ('ShardedHMFRepTokens', 'ShardedHMFBags'):
        _check_view(cls_name, rank, world)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_het_view_recommend_evaluate_match_global_oracle_gloo(tmp_path, world):
    import torch.multiprocessing as mp
    port = 33300 + 10 * world + (os.getpid() % 50) * 40
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(world))


def test_bag_models_serve_through_item_view_only():
    """The training classes keep raising NotImplementedError (their message names item_view()), and both have
    item_view."""
    from arx.dist import ShardedHMFBags, ShardedHMFRepTokens
    for cls in (ShardedHMFBags, ShardedHMFRepTokens):
        with pytest.raises(NotImplementedError, match="item_view"):
            cls.recommend(object.__new__(cls), [0], 5)
        with pytest.raises(NotImplementedError, match="item_view"):
            cls.evaluate(object.__new__(cls), [0], [0])
        assert callable(getattr(cls, 'item_view'))


def test_het_rows_range_argument_validation_without_gpu():
    """arx_het_rows_range refuses null pointers, world < 1, rank outside [0, world), c0 > c1, d % 4 != 0, ldo < d,
    unaligned tables and owner blocks that overlap before any launch (small integers stand in for device pointers:
    they are only compared with NULL / checked for alignment); an empty range is not an error."""
    from arx import _lib
    lib = _lib.lib
    f = lib.arx_het_rows_range
    EINVAL, EUNS = -1, -4
    ok = dict(E_id=16, bias_id=32, E_tok=48, bias_tok=64, vals=80, starts=96, lens=112, n_items=37, world=3, rank=1,
              c0=4, c1=4, all_owners=1, d=16, scale=0.5, out=128, ldo=20, bias_out=144, ldb=20, block_rows=8)
    order = tuple(ok)

    def err():
        m = lib.arx_last_error()
        return m.decode() if m else ""
    for bad in ([{p: None} for p in ('E_id', 'bias_id', 'E_tok', 'bias_tok', 'vals', 'starts', 'lens', 'out',
                                      'bias_out')] +
                [dict(world=0), dict(rank=-1), dict(rank=3), dict(c0=5), dict(c0=-1, c1=0), dict(n_items=-1),
                 dict(ldo=12), dict(ldo=18), dict(ldb=0), dict(E_id=20), dict(E_tok=52), dict(out=132),
                 dict(c1=13, block_rows=8)]):
        a = dict(ok, **bad)
        assert f(*[a[k] for k in order], None) == EINVAL, bad
        assert "arx_het_rows_range" in err(), bad
    for bad in (dict(d=18), dict(d=0), dict(d=260)):
        a = dict(ok, **bad)
        assert f(*[a[k] for k in order], None) == EUNS, bad
        assert "arx_het_rows_range" in err(), bad
    assert f(*[ok[k] for k in order], None) == 0                       # c0 == c1: nothing to do, no launch
    assert f(*[dict(ok, all_owners=0, block_rows=0)[k] for k in order], None) == 0
    assert f(*[dict(ok, world=1, rank=0, block_rows=0)[k] for k in order], None) == 0
