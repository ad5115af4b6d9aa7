"""The row-sharded skip-gram / CBOW recommender (arx.dist.ShardedW2V) on the HIP backend:

  1. arx_window_slots_fwd / _bwd against numpy: leading dimensions wider than d, slots a random permutation of a
     block larger than n * mb (what no slot names comes back bit-unchanged), acc_dbase 0 and 1
  2. world-1 steps (1-rank RCCL group), captured and kernel by kernel, against RefW2VSampled in fp64 -- the batches
     and tolerances of tests/test_sharded_w2v_cpu.py -- and bit-identical to each other
  3. world-1 ShardedW2V against the single-process LinearSeq (CBOW, 'mw', fused window): product against product
  4. two rank processes on the one GPU (gloo underneath), three CBOW 'mw' steps against the oracle, one recommend."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_sharded_w2v_cpu as C                                      # noqa: E402  (batches, oracle, comparisons)

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 300, 500
# 'mw': fp32 and fp64 must take the same side of the hinge.  A pool logit is a d-term fp32 dot product of entries
# below 0.5 in magnitude: its error stays below d * 2^-24 * 0.25 < 2e-6 at d = 128, so a clearance of 1e-5 on the fp64
# reference is five times that bound (the CPU test's 1e-4 cannot be had from any seed at B * S = 16384 logits per
# step).  The seeds are chosen so; asserted on the reference at every step.
KINK = 1e-5
SHAPES = [(32, 64, 32, 3), (128, 128, 128, 5)]                        # (B, S, d, n_input)
SEEDS = {(32, True): 5, (32, False): 5, (128, True): 9, (128, False): 14}


def _group(dev, port):
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    return dist


# ------------------------------------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("mb,n,d", [(1, 1, 32), (3, 2, 20), (64, 3, 64), (200, 5, 128), (37, 4, 256)])
def test_window_slots_kernels_match_numpy(dev, mb, n, d, acc):
    import torch
    from arx import ops
    rng = np.random.default_rng(1000 * mb + 10 * n + d)
    ld, n_rows = d + 4, n * mb + 7
    SENT = np.float32(9.0)
    slots = rng.permutation(n_rows)[:n * mb].astype(np.int32)
    R = rng.standard_normal((n_rows, ld)).astype(np.float32)
    base = rng.standard_normal((mb, ld)).astype(np.float32)
    scale, bs = np.float32(0.5 / n), np.float32(0.5)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Rd, based, sd = up(R), up(base), up(slots)
    # forward: at most n + 1 fp32 terms in a fixed order
    out = torch.full((mb, ld), float(SENT), dtype=torch.float32, device=dev)
    ops.window_slots_fwd(Rd[:, :d], sd, n, out[:, :d], scale=float(scale), base=based[:, :d], base_scale=float(bs))
    got = out.cpu().numpy()
    want = float(bs) * base[:, :d].astype(np.float64)
    for t in range(n):
        want = want + float(scale) * R[slots[t * mb:(t + 1) * mb], :d].astype(np.float64)
    np.testing.assert_allclose(got[:, :d], want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
    assert (got[:, d:].view(np.uint32) == SENT.view(np.uint32)).all()
    nob = torch.full((mb, ld), float(SENT), dtype=torch.float32, device=dev)
    ops.window_slots_fwd(Rd[:, :d], sd, n, nob[:, :d], scale=float(scale))            # no base
    np.testing.assert_allclose(nob.cpu().numpy()[:, :d], want - float(bs) * base[:, :d].astype(np.float64),
                               rtol=1e-6, atol=1e-6 * np.abs(want).max())
    # backward: one multiply per element (acc_dbase: and one add) -- bit for bit fp32 numpy
    dX = rng.standard_normal((mb, ld)).astype(np.float32)
    db0 = rng.standard_normal((mb, ld)).astype(np.float32)
    dbase, dR = up(db0), torch.full((n_rows, ld), float(SENT), dtype=torch.float32, device=dev)
    ops.window_slots_bwd(up(dX)[:, :d], sd, n, dbase[:, :d], dR[:, :d], scale=float(scale), base_scale=float(bs),
                         acc_dbase=bool(acc))
    gdb, gdr = dbase.cpu().numpy(), dR.cpu().numpy()
    u = bs * dX[:, :d]
    want_db = (db0[:, :d] + u) if acc else u
    np.testing.assert_array_equal(gdb[:, :d].view(np.uint32), want_db.astype(np.float32).view(np.uint32))
    np.testing.assert_array_equal(gdb[:, d:].view(np.uint32), db0[:, d:].view(np.uint32))
    r = (scale * dX[:, :d]).astype(np.float32)
    for t in range(n):
        np.testing.assert_array_equal(gdr[slots[t * mb:(t + 1) * mb], :d].view(np.uint32), r.view(np.uint32))
    named = np.zeros(n_rows, dtype=bool)
    named[slots] = True
    assert (~named).sum() == 7
    assert (gdr[~named].view(np.uint32) == SENT.view(np.uint32)).all()                # rows no slot names
    assert (gdr[:, d:].view(np.uint32) == SENT.view(np.uint32)).all()                 # the pad columns


# ------------------------------------------------------------------------------------------- 2. steps at world 1
def _w2v(dev, tables, B, S, d, n_in, cbow, loss, graphs, rank=0, world=1, b_loc=None):
    from arx.dist import ShardedW2V
    return ShardedW2V(N_USERS, N_ITEMS, d, b_loc or B, S, n_in, C.LR, rank, world, dev, cbow=cbow, loss=loss,
                      tables=tables, graphs=graphs)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


WORLD1 = [(sh, c, l) for sh in SHAPES for c, l in ((True, 'mw'), (False, 'mw'), (True, 'mce'), (False, 'mce'))]


@pytest.mark.parametrize("shape,cbow,loss", WORLD1,
                         ids=['%d-%d-%d-%d-%s-%s' % (sh + ('cbow' if c else 'skipgram', l)) for sh, c, l in WORLD1])
def test_sharded_w2v_steps_world1(dev, shape, cbow, loss):
    """Five steps (eager, captured, three replays on fresh batches and pools) with graphs, the same five kernel by
    kernel: each against the oracle, and bit-identical to each other."""
    B, S, d, n_in = shape
    dist = _group(dev, 29751)
    syn, params, tables = C.w2v_world(N_USERS, N_ITEMS, d)
    batches = C.w2v_batches(syn, 1, SEEDS[(B, cbow)], b_loc=B, n_sampled=S, n_in=n_in)
    C.check_batches(1, batches, n_in)
    ref = C.w2v_ref(syn, params, cbow, loss, B, d=d, n_sampled=S, n_in=n_in)
    l_ref = []
    for pool, gu, gi, gc in batches:
        users, targets = np.concatenate(gu).tolist(), np.concatenate(gi).tolist()
        if pool is not None:
            ref.stage_pool(pool, {int(v): i for i, v in enumerate(pool)})
        if loss == 'mw':
            gap = C.hinge_gap(ref, users, np.concatenate(gc, axis=1).tolist(), targets)
            assert gap > KINK, gap
        l_ref.append(float(ref.step(users, np.concatenate(gc, axis=1).tolist(), targets)))
    runs = {}
    for graphs in (True, False):
        model = _w2v(dev, tables, B, S, d, n_in, cbow, loss, graphs)
        C.set_positives(model, syn, 0, 1)
        counts = []
        for step, (pool, gu, gi, gc) in enumerate(batches):
            if pool is not None:
                model.set_pool(pool)
            model.step(gu[0], gi[0], gc[0])
            l_got = float(model.read_loss().item())
            print("graphs=%s step %d loss %.9g (oracle %.9g)" % (graphs, step, l_got, l_ref[step]))
            assert abs(l_got - l_ref[step]) <= 1e-5 * abs(l_ref[step]), (graphs, step, l_got, l_ref[step])
            counts.append((model.n_captures, model.n_replays))
        if graphs:
            assert model.use_graphs and counts == [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3)], counts
        else:
            assert not model.use_graphs and counts[-1] == (0, 0)
        got = model.gather_global_tables(slots=True)
        C.compare_tables(got, ref)
        runs[graphs] = got
    for k in runs[True]:
        np.testing.assert_array_equal(_bits(runs[True][k]), _bits(runs[False][k]), err_msg=k)


# ------------------------------------------------------------------------------------- 3. product against product
def test_sharded_w2v_world1_matches_linear_seq(dev):
    """The same tables, pools and batches through the single-process LinearSeq (CBOW, 'mw', fused window) and the
    world-1 ShardedW2V: four steps, losses and all tables and slots."""
    from arx.word2vec import cbow_model
    B, S, d, n_in = 32, 64, 32, 3
    _group(dev, 29751)
    syn, params, tables = C.w2v_world(N_USERS, N_ITEMS, d)
    seq = cbow_model.Model(syn.n_users, syn.n_items, d, B, C.LR, 1.0, syn.u_attr, syn.i_attr,
                           syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind, n_input_items=n_in,
                           loss_function='mw', use_sep_item=True, top_N_items=8, n_sampled=S,
                           params={k: v.copy() for k, v in params.items()}, fuse_window=True)
    assert seq.fuse_window
    pos = syn.positives_dict()
    seq.prepare_warp(pos, pos)
    model = _w2v(dev, tables, B, S, d, n_in, True, 'mw', None)
    C.set_positives(model, syn, 0, 1)
    for step, (pool, gu, gi, gc) in enumerate(C.w2v_batches(syn, 1, SEEDS[(B, True)], n_steps=4, b_loc=B,
                                                            n_sampled=S, n_in=n_in)):
        id2idx = {int(v): i for i, v in enumerate(pool)} if pool is not None else None
        l_seq = seq.step(None, gu[0].tolist(), gc[0].tolist(), gi[0].tolist(), item_sampled=pool,
                         item_sampled_id2idx=id2idx)
        if pool is not None:
            model.set_pool(pool)
        model.step(gu[0], gi[0], gc[0])
        l_got = float(model.read_loss().item())
        print("step %d loss %.9g (LinearSeq %.9g)" % (step, l_got, l_seq))
        assert abs(l_got - l_seq) <= 1e-5 * abs(l_seq), (step, l_got, l_seq)
    got = model.gather_global_tables(slots=True)
    P, A = seq.att_emb.get_params(), seq.att_emb.get_slots()
    for name in C.NAMES:
        for suffix, src in (('', P), ('/Adagrad', A)):
            want = np.asarray(src[name])[2:]
            np.testing.assert_allclose(got[name + suffix].reshape(want.shape), want, rtol=1e-4, atol=1e-6,
                                       err_msg=name + suffix)


# ------------------------------------------------------------------------------------- 4. two ranks on one GPU
def _two_rank_main(rank, world, port, out_dir):
    """One rank of the two-rank test: its own process (gloo underneath: RCCL refuses two ranks on one device)."""
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    B_loc, S, d, n_in = 16, 64, 32, 3
    syn, params, tables = C.w2v_world(N_USERS, N_ITEMS, d)
    model = _w2v(dev, tables, B_loc * world, S, d, n_in, True, 'mw', None, rank=rank, world=world, b_loc=B_loc)
    C.set_positives(model, syn, rank, world)
    ref = C.w2v_ref(syn, params, True, 'mw', B_loc * world, d=d, n_sampled=S, n_in=n_in)
    batches = C.w2v_batches(syn, world, C.W2V_SEED, n_steps=3, b_loc=B_loc, n_sampled=S, n_in=n_in)
    for step, (pool, gu, gi, gc) in enumerate(batches):
        users, targets = np.concatenate(gu).tolist(), np.concatenate(gi).tolist()
        ctx = np.concatenate(gc, axis=1).tolist()
        if pool is not None:
            ref.stage_pool(pool, {int(v): i for i, v in enumerate(pool)})
            model.set_pool(pool)
        gap = C.hinge_gap(ref, users, ctx, targets)
        assert gap > KINK, gap
        l_ref = float(ref.step(users, ctx, targets))
        model.step(gu[rank], gi[rank], gc[rank])
        l_got = float(model.read_loss().item())
        print("rank %d step %d loss %.9g (oracle %.9g)" % (rank, step, l_got, l_ref), flush=True)
        assert abs(l_got - l_ref) <= 1e-5 * abs(l_ref), (step, l_got, l_ref)
    T = model.gather_global_tables(slots=True)
    C.compare_tables(T, ref)
    rows = [C.serve_rows(syn, g, world, B_loc, n_in) for g in range(world)]
    users, ctx, _ = rows[rank]
    k = 7
    got = model.recommend(users, ctx, k)
    np.testing.assert_array_equal(got.cpu().numpy(), C.topk_ref(C.scores(T, users, ctx), users, k))
    torch.cuda.synchronize()
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_sharded_w2v_two_ranks_one_gpu(dev, tmp_path):
    """The N > 1 branches on the HIP backend: two fresh rank processes, each under its own time limit, share the one
    GPU and exchange over gloo -- three CBOW 'mw' steps (graph segments) against the oracle, then one recommend."""
    port = 29560 + (os.getpid() % 100)
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), str(r), "2",
                               str(port), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate()[0].decode(errors='replace') for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d exited with %d:\n%s" % (r, p.returncode, o[-4000:])
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))


if __name__ == "__main__":
    _two_rank_main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
