"""Checkpoints of the row-sharded models on the GPU: arx_rows_fingerprint against its numpy twin (exact), save /
restore into a model with captured step graphs (world 1, RCCL; in place: nothing is re-captured, the run continues
bit for bit), the serving view after a restore, re-striping between two gloo ranks on the one GPU and world 1 (rows
placed by arx_copy_2d / arx_copy_strided_f32), and the striped sequence model (SeqHybridParallel: model.saver)."""
import glob
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
TABLES = ('E_user', 'A_user', 'E_item', 'A_item', 'b_item', 'Ab_item')
TOKENS = ('E_tok', 'A_tok', 'b_tok', 'Ab_tok')


# ---------------------------------------------------------------- the kernel
def _special(rng, rows, ldx):
    """Random floats with the patterns a value compare would miss: -0.0, denormals, infinities, NaNs with payloads."""
    x = rng.standard_normal((rows, ldx)).astype(np.float32)
    bits = x.view(np.uint32).reshape(-1)
    if bits.size:
        pats = np.asarray([0x80000000, 0x00000001, 0x807fffff, 0x7fc00001, 0xffc12345, 0x7f800000, 0x00000000],
                          dtype=np.uint32)
        at = rng.choice(bits.size, size=min(bits.size, max(1, bits.size // 5)), replace=False)
        bits[at] = pats[rng.integers(0, len(pats), size=len(at))]
    return x


def _fp(ops, torch, t, row0, step, out=None):
    out = torch.zeros(1, dtype=torch.int64, device=t.device) if out is None else out
    ops.rows_fingerprint(t, row0, step, out)
    return int(out.item()) & M64


@pytest.mark.parametrize("width", [1, 4, 20, 64, 132])
def test_rows_fingerprint_equals_numpy_twin(dev, width):
    """rows 0 / 1 / 257 / 1003 (one lane group, several workgroups, a ragged tail), packed rows and rows d + 4 apart,
    three stripings, bit patterns that are not values; two calls accumulate into one word."""
    import torch
    from arx import ops
    from arx.utils.checkpoint import rows_fingerprint
    rng = np.random.default_rng(width)
    for rows in (0, 1, 257, 1003):
        for ldx in (width, width + 4):
            host = _special(rng, rows, ldx)
            buf = torch.from_numpy(host).to(dev)
            x = buf[:, :width]
            if ldx == 1:
                x, ref = buf.reshape(-1), host.reshape(-1)
            else:
                ref = host[:, :width]
            for row0, step in ((0, 1), (2, 3), (6, 7)):
                want = rows_fingerprint(ref, row0, step)
                assert _fp(ops, torch, x, row0, step) == want, (rows, ldx, row0, step)
            # two halves into ONE word == the whole
            h = rows // 3
            out = torch.zeros(1, dtype=torch.int64, device=dev)
            _fp(ops, torch, x[:h], 2, 3, out)
            assert _fp(ops, torch, x[h:], 2 + 3 * h, 3, out) == rows_fingerprint(ref, 2, 3), (rows, ldx)
    if width % 4 == 0:                                      # rows that are NOT 16-byte aligned: the scalar reads
        host = _special(rng, 257, width + 4)
        flat = torch.from_numpy(host).to(dev).reshape(-1)
        x = flat[1:1 + 256 * (width + 4)].view(256, width + 4)[:, :width]
        want = rows_fingerprint(host.reshape(-1)[1:1 + 256 * (width + 4)].reshape(256, width + 4)[:, :width], 6, 7)
        assert _fp(ops, torch, x, 6, 7) == want


# ---------------------------------------------------------------- world 1, captured graphs
def _init_world1(dev, port):
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)


def _setup(kind, n_users, n_items, V, d):
    from arx.utils.synthetic import SyntheticHMF
    het = kind != 'ShardedHMF'
    syn = SyntheticHMF(n_users=n_users, n_items=n_items, seed=1, permute_logits=False, n_pos=8,
                       **(dict(item_mulhot=True, mulhot_vocab=V, avg_len=5, max_len=12) if het else {}))
    params = syn.glorot_params(d, seed=2, scale=0.5)
    tables = {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
              'item_bias': params['item_bias_cat_0'][2:]}
    extra = ()
    if het:
        ia = syn.i_attr
        tables.update(token=params['itemembed_mulhot_0'], token_bias=params['item_bias_mulhot_0'])
        extra = ((np.asarray(ia.features_mulhot[0]), np.asarray(ia.mulhot_starts[0]),
                  np.asarray(ia.mulhot_lengths[0])), ia._embedding_classes_list_mulhot[0])
    return syn, params, tables, extra


def _positives(syn, n_users, rank, world):
    own = np.arange(rank, n_users, world)
    ptr = np.zeros(len(own) + 2, dtype=np.int32)
    its = []
    for k, u in enumerate(own):
        its.extend(syn.pos_items[syn.pos_ptr[u]:syn.pos_ptr[u + 1]].tolist())
        ptr[k + 1] = len(its)
    ptr[-1] = ptr[-2]
    return ptr, np.asarray(its, dtype=np.int32)


def _same(a, b, names):
    import torch
    for n in names:
        assert torch.equal(getattr(a, n).view(torch.int32), getattr(b, n).view(torch.int32)), n


SHAPES = {'ShardedHMF': (301, 503, 0, 64, 128, 128),            # (B, S): a shape the bf16-pipe scorer takes
          'ShardedHMFRepTokens': (300, 500, 120, 64, 32, 64), 'ShardedHMFBags': (300, 500, 120, 64, 32, 64)}


@pytest.mark.parametrize("kind", ["ShardedHMF", "ShardedHMFRepTokens", "ShardedHMFBags"])
def test_restore_into_captured_model_world1(dev, tmp_path, kind):
    """graphs=True.  Four steps (eager, captured, replayed twice), save; two more steps on other batches; restore into
    the SAME object; three further steps: tables and slots bit-identical to a twin that was never interrupted, and
    nothing was captured again -- the buffers were written in place.  Two uninterrupted twins are compared first, so a
    step that is not reproducible cannot be read as a checkpoint failure."""
    import torch
    import torch.distributed as dist
    from arx import dist as adist
    from arx.utils.checkpoint import ShardedSaver
    _init_world1(dev, 29791)
    try:
        n_users, n_items, V, d, B, S = SHAPES[kind]
        syn, params, tables, extra = _setup(kind, n_users, n_items, V, d)
        names = TABLES + (TOKENS if extra else ())
        ptr, its = _positives(syn, n_users, 0, 1)
        models = [getattr(adist, kind)(n_users, n_items, d, B, S, 0.5, 0, 1, dev, *extra, tables=tables, graphs=True)
                  for _ in range(3)]
        rng = np.random.default_rng(3)
        pool = syn.sample_pool(S, rng)
        for m in models:
            assert m.use_graphs and isinstance(m.saver, ShardedSaver)
            m.set_positives(ptr, syn.pos_items)
            m.set_pool(pool)
            m.saver.chunk_bytes = 4096
        batches = [syn.sample_batch(B, rng) for _ in range(9)]
        m0, m1, m2 = models
        for users, items in batches[:4]:
            for m in models:
                m.step(users, items)
        path = m0.saver.save(None, str(tmp_path / 'ckpt'), global_step=m0.steps)
        assert path.endswith('ckpt-4') and os.path.isfile(path + '.manifest.json')
        for users, items in batches[7:]:                    # the run goes somewhere else ...
            m0.step(users, items)
        assert not torch.equal(m0.E_user, m1.E_user) and m0.steps == 6
        ptrs = [getattr(m0, n).data_ptr() for n in names]
        caps = m0.n_captures
        m0.lr.fill_(0.125)
        m0.saver.restore(None, path)                        # ... and comes back
        assert m0.steps == 4 and float(m0.lr.item()) == 0.5 and m0.n_restores == 1
        assert ptrs == [getattr(m0, n).data_ptr() for n in names]
        _same(m0, m1, names)
        replays = m0.n_replays
        for users, items in batches[4:7]:
            for m in models:
                m.step(users, items)
        _same(m1, m2, names)                                # the step itself is reproducible
        _same(m0, m1, names)
        assert m0.n_captures == caps >= 1 and m0.n_replays == replays + 3
        assert m0.steps == m1.steps == 7
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["ShardedHMFRepTokens", "ShardedHMFBags"])
def test_view_refreshes_after_restore(dev, tmp_path, kind):
    """A view taken (and refreshed) before a restore that lands on the SAME step count serves the restored tables:
    its recommend equals a fresh view's, and it refreshed once more."""
    import torch
    import torch.distributed as dist
    from arx import dist as adist
    _init_world1(dev, 29792)
    try:
        n_users, n_items, V, d, B, S = SHAPES[kind]
        syn, params, tables, extra = _setup(kind, n_users, n_items, V, d)
        ptr, its = _positives(syn, n_users, 0, 1)
        a, b = [getattr(adist, kind)(n_users, n_items, d, B, S, 0.5, 0, 1, dev, *extra, tables=tables, graphs=True)
                for _ in range(2)]
        rng = np.random.default_rng(3)
        pool = syn.sample_pool(S, rng)
        for m in (a, b):
            m.set_positives(ptr, syn.pos_items)
            m.set_pool(pool)
        for k in range(3):                                  # two runs, three steps each, on different batches
            a.step(*syn.sample_batch(B, rng))
            b.step(*syn.sample_batch(B, rng))
        path = a.saver.save(None, str(tmp_path / 'a'))
        view = b.item_view()
        assert not hasattr(view, 'saver')
        ask = rng.choice(n_users, size=B, replace=False)
        before = view.recommend(ask, 30)
        assert view.n_refresh == 1
        b.saver.restore(None, path)
        assert b.steps == 3 == view.steps                   # (a bare step compare would call the view fresh)
        got = view.recommend(ask, 30)
        assert view.n_refresh == 2
        want = b.item_view().recommend(ask, 30)
        assert torch.equal(got, want) and torch.equal(got, a.item_view().recommend(ask, 30))
        assert not torch.equal(got, before)
    finally:
        dist.destroy_process_group()


# ---------------------------------------------------------------- two gloo ranks on the one GPU <-> world 1
N_USERS, N_ITEMS, D, B_LOC, S_POOL = 301, 503, 64, 32, 60


def _train(model, syn, rank, world, steps=3):
    rng = np.random.default_rng(5)                          # identical stream on every rank
    for step in range(steps):
        if step == 0:
            model.set_pool(rng.choice(N_ITEMS, size=S_POOL, replace=False).astype(np.int32))
        gu, gi = [], []
        for g in range(world):
            users = rng.integers(0, len(np.arange(g, N_USERS, world)), size=B_LOC) * world + g
            gu.append(users)
            gi.append(syn.pos_items[syn.pos_ptr[users] + rng.integers(0, syn.n_pos, size=B_LOC)])
        model.step(gu[rank].astype(np.int32), gi[rank].astype(np.int32))


def _hmf(rank, world, dev, syn, tables=None, seed=0):
    from arx.dist import ShardedHMF
    model = ShardedHMF(N_USERS, N_ITEMS, D, B_LOC, S_POOL, 0.5, rank, world, dev, tables=tables, seed=seed)
    model.set_positives(*_positives(syn, N_USERS, rank, world))
    model.saver.chunk_bytes = 1024                          # (four table rows: every progression spans many chunks)
    return model


def _bitwise(got, want):
    assert set(got) == set(want.files)
    for k in want.files:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), k


def _two_rank_worker(rank, world, port, out_dir, mode):
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
    syn, params, tables, _ = _setup('ShardedHMF', N_USERS, N_ITEMS, 0, D)
    if mode == 'save':
        model = _hmf(rank, world, dev, syn, tables=tables)
        _train(model, syn, rank, world)
        model.saver.save(None, os.path.join(out_dir, 'w2'), global_step=model.steps)
        got = model.gather_global_tables(slots=True)
        if rank == 0:
            np.savez(os.path.join(out_dir, 'w2.npz'), **got)
    else:
        model = _hmf(rank, world, dev, syn, seed=9)
        model.saver.restore(None, os.path.join(out_dir, 'w1-3'))
        _bitwise(model.gather_global_tables(slots=True), np.load(os.path.join(out_dir, 'w1.npz')))
        assert model.steps == 3 and not model.E_item[model.ni_loc].any()
        _train(model, syn, rank, world, steps=2)            # (and it trains on: eager, then captured)
    dist.barrier()
    with open(os.path.join(out_dir, "%s%d" % (mode, rank)), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_restripe_two_ranks_one_gpu_and_world1(dev, tmp_path):
    """Saved by two rank processes sharing the GPU (gloo), restored at world 1 in this process (rows of the two files
    interleaved by arx_copy_2d / arx_copy_strided_f32 into E[l0::2]) -- and saved here, restored by two ranks (every
    second row of the one file).  Tables and slots bit for bit.  At most three processes hold the GPU."""
    import torch.distributed as dist
    import torch.multiprocessing as mp
    out = str(tmp_path)
    port = 29620 + (os.getpid() % 100)
    mp.spawn(_two_rank_worker, args=(2, port, out, 'save'), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("save%d" % r)) for r in range(2))
    ni = [(N_ITEMS - r + 1) // 2 for r in range(2)]
    assert [np.load(os.path.join(out, 'w2-3.item.r%dof2.npy' % r)).shape for r in range(2)] == [(n, D) for n in ni]
    _init_world1(dev, 29793)
    try:
        syn, params, tables, _ = _setup('ShardedHMF', N_USERS, N_ITEMS, 0, D)
        model = _hmf(0, 1, dev, syn, seed=9)
        model.saver.restore(None, os.path.join(out, 'w2-3'))
        _bitwise(model.gather_global_tables(slots=True), np.load(os.path.join(out, 'w2.npz')))
        assert model.steps == 3 and not model.E_item[N_ITEMS].any() and float(model.b_item[N_ITEMS]) == 0.0
        _train(model, syn, 0, 1, steps=2)
        # ... and the other way
        model = _hmf(0, 1, dev, syn, tables=tables)
        _train(model, syn, 0, 1)
        model.saver.save(None, os.path.join(out, 'w1'), global_step=model.steps)
        np.savez(os.path.join(out, 'w1.npz'), **model.gather_global_tables(slots=True))
    finally:
        dist.destroy_process_group()
    mp.spawn(_two_rank_worker, args=(2, port + 100, out, 'restore'), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("restore%d" % r)) for r in range(2))


# ---------------------------------------------------------------- the striped sequence model
CFG_ID = dict(n_users=301, n_items=503, logit_size=503)
SEQ = dict(size=64, B_loc=16, L=5, S=128)


def _seq_worker(rank, world, port, out_dir, mode):
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from arx.dist import SeqHybridParallel
    from arx.utils.checkpoint import ShardedSaver, array_file, latest_checkpoint
    from test_lstm_gpu import _build, _batch, RTOL

    size, L, S = SEQ['size'], SEQ['L'], SEQ['S']
    B = SEQ['B_loc'] * 2                                     # the global batch of the saved run
    B_here = B // world
    syn, emb, model, remb, ref = _build(CFG_ID, 'mw', size, B_here, L, S, 5.0, seed=4)
    if world > 1:
        ref = remb = None
    dp = SeqHybridParallel(model)
    assert isinstance(model.saver, ShardedSaver) and model.saver is dp.saver
    model.saver.chunk_bytes = 4096
    rng = np.random.default_rng(7)
    pool = syn.sample_pool(S, rng)
    id2idx = {int(v): i for i, v in enumerate(pool)}
    sl = slice(rank * B_here, (rank + 1) * B_here)
    batches = [_batch(syn, rng, L, B) for _ in range(3)]

    def step(k, ps, oracle_only=False):
        """Batch k on the oracle (which sees the pool with batch 0) and -- unless oracle_only -- on the model, fed
        the pool `ps` (None: the one it has)."""
        users, inp, tg, w = batches[k]
        l_ref = None
        if ref is not None:
            l_ref = ref.step(list(users), inp.tolist(), tg.tolist(), w.tolist(), pool if k == 0 else None, id2idx)
        if oracle_only:
            return None, l_ref
        return model.step(None, list(users[sl]), inp[:, sl].tolist(), tg[:, sl].tolist(), w[:, sl].tolist(), 0,
                          ps, id2idx), l_ref

    def state():
        st = {'p/' + k: v for k, v in dp.global_params().items()}
        st.update({'s/' + k: v for k, v in dp.global_params(slots=True).items()})
        for p in model.rt.dense.values():
            st['d/' + p.name] = p.w.cpu().numpy()
            st['a/' + p.name] = p.acc.cpu().numpy()
        return st

    if mode == 'save':
        step(0, pool)
        step(1, None)
        path = model.saver.save(None, os.path.join(out_dir, 'seq'), global_step=model.rt.global_step)
        assert path == os.path.join(out_dir, 'seq-2')
        for t in emb.tables.values():                       # the owned rows: not the stripe's padding, not rows + 1
            f = np.load(array_file(path, t.name, 'rows', rank, world))
            assert f.shape == (t.shard['count'], t.E.shape[1]) and t.E.shape[0] == t.shard['rows'] + 1
            if t.bias is not None:
                assert np.load(array_file(path, t.bias_name, 'rows', rank, world)).shape == (t.shard['count'],)
        for p in model.rt.dense.values():                   # replicated: rank 0's copy, once
            assert os.path.isfile(array_file(path, p.name, 'replicated', 0, 1))
            assert not glob.glob(array_file(path, p.name, 'rows', 0, 1).replace('r0of1', 'r[0-9]*of*'))
        st = state()
        if rank == 0:
            np.savez(os.path.join(out_dir, 'seq.npz'), **st)
    else:
        with torch.no_grad():                               # a model that knows nothing
            for t in emb.tables.values():
                t.E[:t.shard['count']].normal_()
                t.acc[:t.shard['count']].fill_(7.0)
            for p in model.rt.dense.values():
                p.w.zero_()
                p.acc.fill_(3.0)
        ptrs = [t.data_ptr() for _, t, _, _ in dp._checkpoint_arrays()]
        model.rt.set_learning_rate(0.01)
        path = latest_checkpoint(out_dir)
        model.saver.restore(None, path)
        assert ptrs == [t.data_ptr() for _, t, _, _ in dp._checkpoint_arrays()]
        want = np.load(os.path.join(out_dir, 'seq.npz'))
        got = state()
        assert set(got) == set(want.files)
        for k in want.files:
            a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
        assert model.rt.global_step == 2 and model.rt.lr_host == 0.5
        assert abs(float(model.rt.lr.item()) - 0.5) == 0.0
        for t in emb.tables.values():
            assert not t.E[t.shard['zero_row']].any()
        # one further step against the oracle, which is advanced through the two saved steps first
        step(0, None, oracle_only=True)
        step(1, None, oracle_only=True)
        l_got, l_ref = step(2, pool)                        # (the pool is input data: fed again)
        np.testing.assert_allclose(dp.global_loss(l_got), l_ref, rtol=RTOL)
        for k, v in dp.global_params().items():
            np.testing.assert_allclose(v, remb.params[k], rtol=RTOL, atol=3e-6, err_msg=k)
        for k, v in dp.global_params(slots=True).items():
            np.testing.assert_allclose(v, remb.slots[k], rtol=RTOL, atol=3e-6, err_msg='slot ' + k)
        np.testing.assert_allclose(model.W.w.cpu().numpy(), ref.W, rtol=RTOL, atol=3e-6, err_msg='lstm_w')
        np.testing.assert_allclose(model.b.w.cpu().numpy(), ref.b, rtol=RTOL, atol=3e-6, err_msg='lstm_b')
    dist.barrier()
    with open(os.path.join(out_dir, "seq_%s%d" % (mode, rank)), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_seq_hybrid_saver_world2_to_world1(dev, tmp_path):
    """model.saver of a wrapped SeqModel: saved by two ranks after two steps, restored by a fresh model wrapped at world
    1 -- global_params(), their slots, every dense weight and slot, global_step and the learning rate equal bit for
    bit; one further step matches the oracle; the files hold `count` rows per table."""
    import torch.multiprocessing as mp
    port = 29400 + (os.getpid() % 100)
    mp.spawn(_seq_worker, args=(2, port, str(tmp_path), 'save'), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("seq_save%d" % r)) for r in range(2))
    mp.spawn(_seq_worker, args=(1, port + 100, str(tmp_path), 'restore'), nprocs=1, join=True)
    assert os.path.exists(tmp_path / "seq_restore0")
