"""Full-vocabulary evaluation of the row-sharded HMF model (ShardedHMF.evaluate) and its three kernels on the GPU.

Oracles: the kernels against numpy on their own inputs; the model against the device's own logits (ops.gemm over the
item table in chunks, reduced in float64) where the data are random floats -- margins and losses at rtol 1e-5, the
rank counts bracketed by the counts at t -/+ a few ulps -- and against a float64 oracle over the global tables where
the tables are dyadic (every score exact: counts and ties compare exactly).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dyadic(rng, *shape, lo=-2, hi=3, den=2.0):
    return (rng.integers(lo, hi, size=shape) / den).astype(np.float32)


# ---------------------------------------------------------------- the rank-parts GEMM
def _check_rank_parts(dev, d, dyadic, M, N, tcol, rng, rand_rows):
    """One launch of arx_gemm_nt_eval_rank_parts on seeded [M, d] x [N, d] tables against the device's own logits:
    tcol [M] int32 (outside [0, N): the target is elsewhere); t = the target's logit, an unrelated value in rand_rows.
    -> the rows' counts.  (test_gemm_nt_fused_gpu.py runs it at the shape edges.)"""
    import torch
    from arx import ops
    if dyadic:
        A, Bm, bias = _dyadic(rng, M, d), _dyadic(rng, N, d), _dyadic(rng, N, lo=-4, hi=5, den=4.0)
    else:
        A = (rng.standard_normal((M, d)) * 0.3).astype(np.float32)
        Bm = (rng.standard_normal((N, d)) * 0.3).astype(np.float32)
        bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    At, Bt, bt = (torch.from_numpy(x).to(dev) for x in (A, Bm, bias))
    L = torch.empty((M, N), dtype=torch.float32, device=dev)
    ops.gemm(At, Bt, L, ops.Workspace(dev), transB=True, col_bias=bt)
    lg = L.cpu().numpy().astype(np.float64)
    t = lg[np.arange(M), np.clip(tcol, 0, N - 1)].astype(np.float32)
    t[rand_rows] = (rng.standard_normal(len(t[rand_rows])) * 0.5).astype(np.float32)
    if dyadic:
        t[rand_rows] = np.round(t[rand_rows] * 4) / 4
    npart = ops.gemm_nt_topk_parts(M, N)
    rp = torch.full((M, npart + 3), 7.0, dtype=torch.float32, device=dev)
    cp = torch.full((M, npart + 3), 7, dtype=torch.int32, device=dev)
    ops.gemm_nt_eval_rank_parts(At, Bt, bt, torch.from_numpy(t).to(dev), torch.from_numpy(tcol).to(dev), rp, cp)
    got_m = rp.cpu().numpy()[:, :npart].astype(np.float64).sum(1)
    got_c = cp.cpu().numpy()[:, :npart].astype(np.int64).sum(1)
    assert (rp.cpu().numpy()[:, npart:] == 7.0).all() and (cp.cpu().numpy()[:, npart:] == 7).all()
    tt = t.astype(np.float64)[:, None]
    on = (tcol >= 0) & (tcol < N)
    hit = np.zeros((M, N), dtype=bool)
    hit[np.nonzero(on)[0], tcol[on]] = True
    marg = np.where(hit, 1.0, np.maximum((lg - tt) + 1.0, 0.0)).sum(1)
    np.testing.assert_allclose(got_m, marg, rtol=1e-5)
    if dyadic:
        np.testing.assert_array_equal(got_c, ((lg > tt) & ~hit).sum(1))
    else:
        sp = 4.0 * np.spacing(np.abs(t)).astype(np.float64)[:, None]
        lo, hi = ((lg > tt + sp) & ~hit).sum(1), ((lg > tt - sp) & ~hit).sum(1)
        assert ((got_c >= lo) & (got_c <= hi)).all()
    return got_c


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("dyadic", [True, False])
def test_gemm_nt_eval_rank_parts_matches_numpy(dev, d, dyadic):
    """margins at rtol 1e-5 against the device's own logits (ops.gemm); counts exact on dyadic data, on random floats
    between the counts at t + 4 ulp and t - 4 ulp; the target column adds exactly (1, 0); rows whose target is
    elsewhere (tcol -1 or N) count every column."""
    rng = np.random.default_rng(d + 7 * dyadic)
    M, N = 300, 20011
    tcol = np.random.default_rng(d + 70 * dyadic + 1).integers(0, N, size=M).astype(np.int32)
    tcol[::5], tcol[1::7] = -1, N                                      # targets on other shards
    got_c = _check_rank_parts(dev, d, dyadic, M, N, tcol, rng, slice(None, None, 5))
    assert (got_c > 0).any() and (got_c < N - 1).any()


# ---------------------------------------------------------------- the shard reduce
def _reduce_ref(mode, parts, cparts, U, E, bias, t, tcol, keys, ptr, cols):
    B = parts.shape[0] if parts is not None else len(t)
    V = E.shape[0]
    if mode == 'ce':
        if parts is None:
            return np.full(B, -np.inf), None
        m = parts.max(1)
        m0 = np.where(np.isneginf(m), 0.0, m)
        with np.errstate(divide='ignore'):
            return m0 + np.log(np.exp(parts - m0[:, None]).sum(1)), None
    s = parts.sum(1) if parts is not None else np.zeros(B)
    c = cparts.sum(1) if cparts is not None else np.zeros(B, dtype=np.int64)
    for r in range(B):
        if keys is None or keys[r] < 0:
            continue
        for j in cols[ptr[keys[r]]:ptr[keys[r] + 1]]:
            if not 0 <= j < V:
                continue
            if j == tcol[r]:
                s[r] -= 1.0
                continue
            x = float(U[r].astype(np.float64) @ E[j].astype(np.float64) + bias[j])
            s[r] -= max(x - t[r] + 1.0, 0.0)
            c[r] -= int(x > t[r])
    return np.maximum(s, 0.0), np.maximum(c, 0)


@pytest.mark.parametrize("mode", ['ce', 'warp', 'warp_eval'])
@pytest.mark.parametrize("masked", [False, True])
def test_eval_shard_reduce_matches_numpy(dev, mode, masked):
    """arx_eval_shard_reduce == numpy: parts folded (logsumexp / sum / int sum), masked local columns taken out with
    dyadic U / E (exact scores), the target column as (1, 0), keys < 0 and a row_keys period (key_rows < B), columns
    past V skipped, the clamp at 0, and a shard without columns (npart 0)."""
    import torch
    from arx import ops
    rng = np.random.default_rng(5)
    B, V, d, n_users = 200, 900, 64, 50
    U, E, bias = _dyadic(rng, B, d), _dyadic(rng, V, d), _dyadic(rng, V, lo=-4, hi=5, den=4.0)
    t = _dyadic(rng, B, lo=-8, hi=9, den=2.0)
    tcol = rng.integers(0, V + 1, size=B).astype(np.int32)              # V: the target is elsewhere
    npart = 37
    if mode == 'ce':
        parts = (rng.standard_normal((B, npart)) * 3).astype(np.float32)
        parts[3] = -np.inf
        parts[4, :-1] = -np.inf
    else:
        parts = (rng.random((B, npart)) * 4).astype(np.float32)
    cparts = rng.integers(0, 40, size=(B, npart)).astype(np.int32)
    key_rows = 150
    keys = rng.integers(-1, n_users, size=key_rows).astype(np.int32)
    lists = [np.unique(rng.integers(0, V + 20, size=int(rng.integers(0, 60)))) for _ in range(n_users)]
    for r in range(0, key_rows, 9):                                      # some lists hold the row's target
        if keys[r] >= 0 and tcol[r] < V:
            lists[keys[r]] = np.unique(np.append(lists[keys[r]], tcol[r]))
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    cols = np.concatenate(lists).astype(np.int32)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ex = (T(keys), key_rows, T(ptr), T(cols)) if masked else None
    wev = mode == 'warp_eval'
    for np_ in (npart, 0):
        out = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
        cnt = torch.full((B,), 7, dtype=torch.int32, device=dev) if wev else None
        p_t = T(parts[:, :np_]) if np_ else None
        c_t = T(cparts[:, :np_]) if (np_ and wev) else None
        ops.eval_shard_reduce(mode, p_t, c_t, T(U), T(E), T(bias), T(t), T(tcol), ex, out, cnt)
        kk = np.asarray([keys[r % key_rows] for r in range(B)]) if masked else None
        want, wc = _reduce_ref(mode, parts[:, :np_].astype(np.float64) if np_ else None,
                               cparts[:, :np_].astype(np.int64) if (np_ and wev) else None, U, E, bias,
                               t.astype(np.float64), tcol, kk, ptr, cols)
        np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-5, atol=1e-4, err_msg=str(np_))
        if wev:
            np.testing.assert_array_equal(cnt.cpu().numpy(), wc)
        if masked and mode != 'ce' and np_:
            assert 0 < (want == 0).sum() < B                            # the clamp at 0 is exercised, not everywhere


# ---------------------------------------------------------------- the merge
@pytest.mark.parametrize("W", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("mode", ['ce', 'warp', 'warp_eval'])
def test_eval_merge_shards_matches_numpy(dev, W, mode):
    import torch
    from arx import ops
    rng = np.random.default_rng(W)
    for B in (1, 7, 4097):
        parts = (rng.standard_normal((W, B)) * 3).astype(np.float32)
        if mode == 'ce':
            parts[rng.random((W, B)) < 0.3] = -np.inf                  # shards without columns
            parts[0] = np.where(np.isneginf(parts).all(0), 0.5, parts[0])
        else:
            parts = np.abs(parts)
        cnts = rng.integers(0, 10 ** 6, size=(W, B)).astype(np.int32)
        t = rng.standard_normal(B).astype(np.float32)
        out = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
        cnt = torch.full((B,), 7, dtype=torch.int32, device=dev)
        T = lambda x: torch.from_numpy(x).to(dev)
        wev = mode == 'warp_eval'
        ops.eval_merge_shards(mode, T(parts), T(cnts) if wev else None, T(t), out, cnt if wev else None)
        p = parts.astype(np.float64)
        if mode == 'ce':
            m = p.max(0)
            want = m + np.log(np.exp(p - m).sum(0)) - t
        else:
            want = np.log1p(p.sum(0)) if mode == 'warp' else p.sum(0)
        np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-5, atol=1e-6, err_msg=str(B))   # (ce: lse - t cancels)
        if wev:
            np.testing.assert_array_equal(cnt.cpu().numpy(), cnts.astype(np.int64).sum(0))
        else:
            assert (cnt.cpu().numpy() == 7).all()
        out2 = torch.empty_like(out)
        ops.eval_merge_shards(mode, T(parts), T(cnts) if wev else None, T(t), out2, cnt if wev else None)
        assert torch.equal(out, out2)                                  # deterministic


# ---------------------------------------------------------------- model-level oracle on the device logits
def _init_world1(dev, port):
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)


def _device_oracle(U_rows, E, b, targets, pos, dev, chunk=1 << 22):
    """per row (float64, from the device's float32 logits of ops.gemm, t from ops.dot_score as evaluate forms it):
    lse - t, the masked margin, and the masked count at t +/- 4 ulp (lo, hi)."""
    import torch
    from arx import ops
    R, V = int(U_rows.shape[0]), int(E.shape[0])
    tg = torch.from_numpy(np.asarray(targets, dtype=np.int64)).to(dev)
    t_d = torch.empty(R, dtype=torch.float32, device=dev)
    ops.dot_score(U_rows.contiguous(), E[tg].contiguous(), b[tg].contiguous(), t_d)
    t = t_d.cpu().numpy().astype(np.float64)
    sp = 4.0 * np.spacing(np.abs(t_d.cpu().numpy())).astype(np.float64)
    ws = ops.Workspace(dev)
    buf = torch.empty((R, min(chunk, V)), dtype=torch.float32, device=dev)
    mx, se = np.full(R, -np.inf), np.zeros(R)
    marg, lo, hi = np.zeros(R), np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    masks = [np.asarray(sorted(p), dtype=np.int64) for p in pos]
    for c0 in range(0, V, chunk):
        c1 = min(V, c0 + chunk)
        lg = buf[:, :c1 - c0]
        ops.gemm(U_rows, E[c0:c1], lg, ws, transB=True, col_bias=b[c0:c1])
        x = lg.cpu().numpy().astype(np.float64)
        m2 = np.maximum(mx, x.max(1))
        se = se * np.exp(mx - m2) + np.exp(x - m2[:, None]).sum(1)
        mx = m2
        keep = np.ones(x.shape, dtype=bool)
        for r in range(R):
            mk = masks[r][(masks[r] >= c0) & (masks[r] < c1)] - c0
            keep[r, mk] = False
            if c0 <= targets[r] < c1:
                keep[r, targets[r] - c0] = False                       # (added back below unless masked)
        marg += (np.maximum(x - t[:, None] + 1.0, 0.0) * keep).sum(1)
        lo += ((x > (t + sp)[:, None]) & keep).sum(1)
        hi += ((x > (t - sp)[:, None]) & keep).sum(1)
    for r in range(R):
        if targets[r] not in set(masks[r].tolist()):
            marg[r] += 1.0
    return mx + np.log(se) - t, marg, lo, hi


def _check_model(model, users, items, pos, U_rows, E, b, dev, rows=None, warp_eval=True):
    """evaluate(...) of every loss against _device_oracle on `rows` of the call (default: all)."""
    rows = np.arange(len(users)) if rows is None else rows
    ce, marg, lo, hi = _device_oracle(U_rows[rows], E, b, np.asarray(items)[rows], [pos.get(int(users[r]), ())
                                                                                     for r in rows], dev)
    m_ce, r_ce = model.evaluate(users, items, loss='ce', return_rows=True)
    np.testing.assert_allclose(r_ce.cpu().numpy()[rows], ce, rtol=1e-5, atol=1e-6)
    m_w, r_w = model.evaluate(users, items, loss='warp', return_rows=True)
    np.testing.assert_allclose(r_w.cpu().numpy()[rows], np.log1p(marg), rtol=1e-5)
    np.testing.assert_allclose(m_w, float(r_w.double().mean()), rtol=1e-5)
    np.testing.assert_allclose(m_ce, float(r_ce.double().mean()), rtol=1e-5)
    if warp_eval:
        mr, tr = model.evaluate(users, items, loss='warp_eval')
        np.testing.assert_allclose(mr.cpu().numpy()[rows], marg, rtol=1e-5)
        got = tr.cpu().numpy()[rows].astype(np.int64)
        assert ((got >= lo) & (got <= hi)).all(), (got, lo, hi)


@pytest.mark.parametrize("d", [128, 48])
def test_sharded_evaluate_world1(dev, d):
    """World 1 (an nccl group of one): the fused eval GEMM at d 128 and the chunked path at d 48 (where 'warp_eval'
    raises NotImplementedError naming the widths), masks with the target inside and outside, n < B_loc."""
    import torch
    import torch.distributed as dist
    from arx.dist import ShardedHMF
    _init_world1(dev, 29871 + d)
    try:
        n_users, n_items, B_loc = 500, 200003, 64
        g = torch.Generator(device='cpu').manual_seed(3)
        U = torch.randn(n_users, d, generator=g) * 0.3
        I = torch.randn(n_items, d, generator=g) * 0.3
        b = torch.randn(n_items, generator=g) * 0.1
        model = ShardedHMF(n_users, n_items, d, B_loc, 64, 0.1, 0, 1, dev,
                           tables={'user': U.numpy(), 'item': I.numpy(), 'item_bias': b.numpy()})
        rng = np.random.default_rng(4)
        users = rng.choice(n_users, size=B_loc - 5, replace=False)
        items = rng.integers(0, n_items, size=len(users))
        pos = {int(u): rng.integers(0, n_items, size=40).tolist() for u in users}
        for j, u in enumerate(users[::3]):
            pos[int(u)].append(int(items[3 * j]))                          # the target masked
        model.prepare_eval_positives(pos)
        U_rows = U[torch.from_numpy(users)].to(dev)
        _check_model(model, users, items, pos, U_rows, I.to(dev), b.to(dev), dev, warp_eval=d == 128)
        if d != 128:
            with pytest.raises(NotImplementedError, match="32, 64 and 128"):
                model.evaluate(users, items, loss='warp_eval')
    finally:
        dist.destroy_process_group()


def test_sharded_evaluate_between_steps_graphs(dev):
    """step, evaluate, step, evaluate with graph segments: losses and every table bit-identical to the same steps
    without the evaluations; each evaluation equals the oracle on the tables as they stood."""
    import torch
    import torch.distributed as dist
    from arx.dist import ShardedHMF
    from arx.utils.synthetic import SyntheticHMF
    _init_world1(dev, 29874)
    try:
        n_users, n_items, d, B, S = 300, 500, 64, 32, 64
        syn = SyntheticHMF(n_users=n_users, n_items=n_items, seed=1, permute_logits=False, n_pos=8)
        params = syn.glorot_params(d, seed=2, scale=0.5)
        tables = {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
                  'item_bias': params['item_bias_cat_0'][2:]}
        ptr = np.concatenate([syn.pos_ptr[:n_users + 1], [syn.pos_ptr[n_users]]]).astype(np.int32)
        models = [ShardedHMF(n_users, n_items, d, B, S, 0.5, 0, 1, dev, tables=tables, graphs=True) for _ in range(2)]
        for m in models:
            assert m.use_graphs
            m.set_positives(ptr, syn.pos_items)
        pos = syn.positives_dict()
        models[0].prepare_eval_positives(pos)
        rng = np.random.default_rng(3)
        pool = syn.sample_pool(S, rng)
        for m in models:
            m.set_pool(pool)
        batches = [syn.sample_batch(B, rng) for _ in range(4)]
        ask = rng.choice(n_users, size=B, replace=False)
        tgt = rng.integers(0, n_items, size=B)
        losses = [[], []]
        for step, (users, items) in enumerate(batches):
            for i, m in enumerate(models):
                m.step(users, items)
                losses[i].append(float(m.read_loss().item()))
            if step % 2 == 0:
                m = models[0]
                U_rows = m.E_user[torch.from_numpy(ask).to(dev)]
                _check_model(m, ask, tgt, pos, U_rows, m.E_item[:n_items], m.b_item[:n_items], dev)
        assert losses[0] == losses[1]
        assert models[0].n_replays > 0
        for name in ('E_user', 'A_user', 'E_item', 'A_item', 'b_item', 'Ab_item'):
            assert torch.equal(getattr(models[0], name), getattr(models[1], name)), name
    finally:
        dist.destroy_process_group()


def test_sharded_evaluate_c5_shape_world1(dev):
    """The C5 shape at world 1: 100 M items x d 128, 1 M users, 1024 rows per call, ~50 eval positives per user;
    'warp_eval' and 'warp' on 8 sampled rows against the device logits of the whole vocabulary (in chunks)."""
    import torch
    import torch.distributed as dist
    from arx.dist import ShardedHMF
    _init_world1(dev, 29875)
    try:
        n_users, n_items, d, B_loc = 1000000, 100000000, 128, 1024
        model = ShardedHMF(n_users, n_items, d, B_loc, 1024, 0.1, 0, 1, dev, seed=5)
        rng = np.random.default_rng(12)
        users = rng.choice(n_users, size=B_loc, replace=False)
        items = rng.integers(0, n_items, size=B_loc)
        pos = {int(u): rng.integers(0, n_items, size=50).tolist() for u in users}
        for u, i in zip(users[::2], items[::2]):
            pos[int(u)].append(int(i))
        model.prepare_eval_positives(pos)
        mr, tr = model.evaluate(users, items, loss='warp_eval')
        mean, rw = model.evaluate(users, items, loss='warp', return_rows=True)
        rows = np.sort(rng.choice(B_loc, size=8, replace=False))
        U_rows = model.E_user[torch.from_numpy(users[rows]).to(dev)]
        _, marg, lo, hi = _device_oracle(U_rows, model.E_item[:n_items], model.b_item[:n_items], items[rows],
                                         [pos[int(users[r])] for r in rows], dev)
        np.testing.assert_allclose(mr.cpu().numpy()[rows], marg, rtol=1e-5)
        got = tr.cpu().numpy()[rows].astype(np.int64)
        assert ((got >= lo) & (got <= hi)).all(), (got, lo, hi)
        np.testing.assert_allclose(rw.cpu().numpy()[rows], np.log1p(marg), rtol=1e-5)
        assert np.isfinite(mean) and (tr.cpu().numpy() >= 0).all() and (tr.cpu().numpy() < n_items).all()
    finally:
        dist.destroy_process_group()


# ---------------------------------------------------------------- two ranks on one GPU (gloo)
def _oracle_global(U, I, b, users, items, loss, pos):
    x_all = U.astype(np.float64)[users] @ I.astype(np.float64).T + b.astype(np.float64)[None, :]
    out, ranks = [], []
    for r, (u, i) in enumerate(zip(users, items)):
        x = x_all[r]
        t = x[i]
        if loss == 'ce':
            m = x.max()
            out.append(m + np.log(np.exp(x - m).sum()) - t)
            continue
        keep = np.ones(len(x), dtype=bool)
        keep[np.asarray(sorted(pos.get(int(u), ())), dtype=np.int64)] = False
        gt = (x > t) & keep
        gt[i] = False
        mg = np.maximum(x - t + 1.0, 0.0)[keep].sum()
        out.append(np.log1p(mg) if loss == 'warp' else mg)
        ranks.append(int(gt.sum()))
    return np.asarray(out), np.asarray(ranks, dtype=np.int64)


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

    n_users, n_items, d, B_loc = 401, 2 * 30011 + 1, 64, 48            # uneven shards
    rng = np.random.default_rng(9)                                      # the same stream on both ranks
    U, I = _dyadic(rng, n_users, d), _dyadic(rng, n_items, d)
    b = _dyadic(rng, n_items, lo=-4, hi=5, den=4.0)
    for a, c in ((10, 11), (1001, 2002), (5, 40000), (7, 8)):          # equal rows on both shards: cross-shard ties
        I[c], b[c] = I[a], b[a]
    model = ShardedHMF(n_users, n_items, d, B_loc, 64, 0.1, rank, world, dev,
                       tables={'user': U, 'item': I, 'item_bias': b})
    asks = [rng.choice(np.arange(s, n_users, world), size=B_loc - 7 * s, replace=False) for s in range(world)]
    tgts = [rng.integers(0, n_items, size=len(a)) for a in asks]
    tgts[0][:4] = (10, 1001, 5, 7)
    tgts[1][:2] = (2002, 8)
    pos_all = [{int(u): rng.integers(0, n_items, size=30).tolist() for u in a} for a in asks]
    for s in range(world):
        for u, i in list(zip(asks[s], tgts[s]))[::3]:
            pos_all[s][int(u)].append(int(i))                               # the target masked
        u0 = int(asks[s][5])
        pos_all[s][u0] = list(range(1, n_items, 2))[:300] * 2             # all on shard 1, duplicated
    mine, tg = asks[rank], tgts[rank]
    all_u, all_i = np.concatenate(asks), np.concatenate(tgts)
    pos = {u: v for p in pos_all for u, v in p.items()}
    model.prepare_eval_positives(pos_all[rank])
    for loss in ('ce', 'warp'):
        mean, rows = model.evaluate(mine, tg, loss=loss, return_rows=True)
        want, _ = _oracle_global(U, I, b, mine, tg, loss, pos)
        np.testing.assert_allclose(rows.cpu().numpy(), want, rtol=1e-5)
        np.testing.assert_allclose(mean, _oracle_global(U, I, b, all_u, all_i, loss, pos)[0].mean(), rtol=1e-5)
    mr, tr = model.evaluate(mine, tg, loss='warp_eval')
    wm, wr = _oracle_global(U, I, b, mine, tg, 'warp_eval', pos)
    np.testing.assert_allclose(mr.cpu().numpy(), wm, rtol=1e-5)
    np.testing.assert_array_equal(tr.cpu().numpy(), wr)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_sharded_evaluate_two_ranks_one_gpu(dev, tmp_path):
    """Two rank processes on the one GPU over gloo, dyadic tables (exact scores): uneven shards, targets with equal
    rows on the other shard (ties never count), masks with the target inside and outside and a mask set entirely on
    one shard; every loss against the float64 oracle over the global tables, true_rank exactly."""
    import torch.multiprocessing as mp
    port = 30180 + (os.getpid() % 100)
    mp.spawn(_two_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))
