"""Checkpoints of the row-sharded models (arx.utils.checkpoint.ShardedSaver; model.saver of arx.dist.ShardedHMF and its
subclasses) without a GPU: gloo ranks over the numpy compute double.  A run saved on W ranks is restored on W' --
tables, Adagrad slots, step count and learning rate bit for bit, the run continuing as if never interrupted (W' = W)
or matching the single-process oracle (W' != W); token tables cross between the striped and the replicated layout;
checkpoints that do not fit are refused before anything is overwritten, damaged files are found by the fingerprint.
chunk_bytes is tiny throughout (320 B: five table rows; 96 B for the HET models: one table row, 24 bias entries): at
these table sizes every stripe then spans several chunks of the staging slab and chunk boundaries fall inside the
arithmetic progressions of a re-stripe.  Plus the numpy twin of arx_rows_fingerprint and the entry's argument
checks (no device is touched)."""
import glob
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "a-recsys_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

N_USERS, N_ITEMS, D, B_LOC, S, V_TOK = 60, 91, 16, 8, 16, 37     # (91 items: a ragged last stripe at every world)
CHUNK = {'hmf': 320, 'bags': 96, 'rep': 96}
LR = 0.5
M64 = (1 << 64) - 1


# ---- the numpy twin ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 4, 20])
def test_fingerprint_twin_is_striping_independent(width):
    from arx.utils.checkpoint import rows_fingerprint
    rng = np.random.default_rng(width)
    x = rng.standard_normal((1003, width)).astype(np.float32)
    if width == 1:
        x = x.reshape(-1)
    whole = rows_fingerprint(x)
    assert 0 <= whole <= M64
    for world in (1, 2, 3, 4, 7):
        assert sum(rows_fingerprint(x[r::world], r, world) for r in range(world)) & M64 == whole, world
    y = x.copy()
    y[[5, 700]] = y[[700, 5]]                                    # every row still there, two in the wrong place
    assert rows_fingerprint(y) != whole
    z = x.copy()
    z.view(np.uint32)[(501, 0) if width > 1 else 501] ^= 1       # one bit
    assert rows_fingerprint(z) != whole
    # written out: K = 0x9E3779B97F4A7C15, row factor (2 g + 1) K, column factor 2 c + 1, bit patterns zero-extended
    a = np.asarray([[1.0, -0.0], [np.nan, 2.5]], dtype=np.float32)
    bits = a.view(np.uint32).tolist()
    K = 0x9E3779B97F4A7C15
    want = sum((2 * g + 1) * K * (row[0] * 1 + row[1] * 3) for g, row in zip((2, 5), bits)) & M64
    assert rows_fingerprint(a, 2, 3) == want
    assert rows_fingerprint(a[:0]) == 0


def test_stripe_progression_covers_every_row_once():
    from arx.utils.checkpoint import owned_rows, stripe_progression
    n = 103
    for N in (1, 2, 3, 4, 6):
        for Np in (1, 2, 3, 4, 6):
            seen = {}
            for rp in range(Np):
                for r in range(N):
                    prog = stripe_progression(r, N, rp, Np)
                    if prog is None:
                        assert not any((r + N * j) % Np == rp for j in range(owned_rows(n, 'rows', r, N)))
                        continue
                    j0, P, l0, Q = prog
                    for t in range(max(0, (owned_rows(n, 'rows', r, N) - j0 + P - 1) // P)):
                        g = r + N * (j0 + t * P)
                        assert g % Np == rp and g // Np == l0 + t * Q and g not in seen
                        seen[g] = rp
            assert sorted(seen) == list(range(n)), (N, Np)


# ---- the entry's argument checks: before the first HIP call ----------------------------------------------------
def test_rows_fingerprint_abi_argument_checks():
    from arx import _lib
    fn, err = _lib.lib.arx_rows_fingerprint, _lib.lib.arx_last_error
    fake = 4096                                                   # (never dereferenced: every call returns first)
    for args in ((None, 4, 3, 4, 0, 1, None, None), (None, 4, 3, 4, 0, 1, fake, None), (fake, 4, 3, 4, 0, 1, None, None),
                 (fake, 4, -1, 4, 0, 1, fake, None), (fake, 3, 2, 4, 0, 1, fake, None), (fake, 4, 2, 0, 0, 1, fake, None),
                 (fake, 4, 2, 4, -1, 1, fake, None), (fake, 4, 2, 4, 0, 0, fake, None)):
        assert fn(*args) == -1, args                              # ARX_EINVAL
        assert b"arx_rows_fingerprint" in err(), args
    assert fn(fake, 4, 0, 4, 0, 1, fake, None) == 0               # rows == 0: legal, nothing to add
    assert fn(None, 4, 0, 4, 2, 3, fake, None) == 0


# ---- models ----------------------------------------------------------------------------------------------------
def _bitwise_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _init(rank, world, port):
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _world(kind):
    from arx.utils.synthetic import SyntheticHMF
    het = kind != 'hmf'
    syn = SyntheticHMF(n_users=N_USERS, n_items=N_ITEMS, seed=1, permute_logits=False, n_pos=6,
                       **(dict(item_mulhot=True, mulhot_vocab=V_TOK, avg_len=4, max_len=9) if het else {}))
    params = syn.glorot_params(D, seed=2, scale=0.5)
    tables = {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
              'item_bias': params['item_bias_cat_0'][2:]}
    extra = ()
    if het:
        ia = syn.i_attr
        tables.update(token=params['itemembed_mulhot_0'], token_bias=params['item_bias_mulhot_0'])
        extra = ((np.asarray(ia.features_mulhot[0]), np.asarray(ia.mulhot_starts[0]),
                  np.asarray(ia.mulhot_lengths[0])), ia._embedding_classes_list_mulhot[0])
    return syn, params, tables, extra


def _model(kind, syn, rank, world, extra, tables=None, seed=0, n_items=N_ITEMS, d=D):
    from arx import dist as adist
    from numpy_backend import NumpyBackend
    cls = {'hmf': adist.ShardedHMF, 'bags': adist.ShardedHMFBags, 'rep': adist.ShardedHMFRepTokens}[kind]
    model = cls(N_USERS, n_items, d, B_LOC, S, LR, rank, world, 'cpu', *extra, backend=NumpyBackend(), tables=tables,
                seed=seed)
    own = np.arange(rank, N_USERS, world)
    ptr = np.zeros(len(own) + 2, dtype=np.int32)
    items = []
    for k, u in enumerate(own):
        items.extend(syn.pos_items[syn.pos_ptr[u]:syn.pos_ptr[u + 1]].tolist())
        ptr[k + 1] = len(items)
    ptr[-1] = ptr[-2]
    model.set_positives(ptr, np.asarray(items, dtype=np.int32))
    model.saver.chunk_bytes = CHUNK[kind]
    return model


def _draw(rng, syn, world, step):
    """Step `step` of the shared input stream at `world` ranks: (pool or None, users per rank, targets per rank)."""
    pool = rng.choice(N_ITEMS, size=S, replace=False).astype(np.int32) if step % 2 == 0 else None
    gu, gi = [], []
    for g in range(world):
        users = rng.integers(0, len(np.arange(g, N_USERS, world)), size=B_LOC) * world + g
        gu.append(users)
        gi.append(syn.pos_items[syn.pos_ptr[users] + rng.integers(0, syn.n_pos, size=B_LOC)])
    gu[0][1] = gu[0][0]                                          # duplicate user / target rows
    gi[-1][2] = gi[-1][3]
    return pool, gu, gi


def _run(model, ref, rng, syn, world, rank, steps, state):
    """`steps` steps of the stream on the model (and the oracle, if any); state: the current pool and its id map."""
    for step in steps:
        pool, gu, gi = _draw(rng, syn, world, step)
        if pool is not None:
            state['pool'], state['id2idx'] = pool, {int(v): i for i, v in enumerate(pool)}
            if model is not None:
                model.set_pool(pool)
        if ref is not None:
            ref.step(np.concatenate(gu).tolist(), np.concatenate(gi).tolist(), pool, state['id2idx'], loss='mw')
        if model is not None:
            model.step(gu[rank].astype(np.int32), gi[rank].astype(np.int32))


def _oracle(syn, params, world):
    from oracle import ref_graph as rg
    ref = rg.RefLatentProductModel(D, B_LOC * world, LR, syn.u_attr, syn.i_attr, syn.item_ind2logit_ind_dict(),
                                   syn.logit_ind2item_ind, loss_function='mw', n_sampled=S, params=params,
                                   dtype=np.float64)
    pos = syn.positives_dict()
    ref.prepare_warp(pos, pos)
    return ref


def _save_worker(rank, world, port, out_dir, kind, more):
    """Three steps at `world`, save (twice for the id-only model: steps 2 and 3, for the index file); the gathered
    tables and slots go to saved.npz; `more` further steps on the same model -> cont.npz (the uninterrupted run)."""
    dist = _init(rank, world, port)
    from arx.utils.checkpoint import ShardedSaver
    syn, params, tables, extra = _world(kind)
    model = _model(kind, syn, rank, world, extra, tables=tables)
    assert isinstance(model.saver, ShardedSaver)
    rng, state = np.random.default_rng(5), {}
    _run(model, None, rng, syn, world, rank, range(2), state)
    if kind == 'hmf':
        p = model.saver.save(None, os.path.join(out_dir, 'ckpt'), global_step=model.steps)
        assert p == os.path.join(out_dir, 'ckpt-2')
    _run(model, None, rng, syn, world, rank, range(2, 3), state)
    p = model.saver.save(None, os.path.join(out_dir, 'ckpt'), global_step=model.steps)
    assert p == os.path.join(out_dir, 'ckpt-3') and os.path.isfile(p + '.manifest.json')
    # the files hold the owned rows: no zero row, no padding
    ni = (N_ITEMS - rank + world - 1) // world
    assert np.load(p + '.item.r%dof%d.npy' % (rank, world)).shape == (ni, D)
    assert np.load(p + '.item_bias.Adagrad.r%dof%d.npy' % (rank, world)).shape == (ni,)
    if kind == 'rep':
        assert np.load(p + '.token.rep.npy').shape == (model.n_tokens, D)
        assert not glob.glob(p + '.token.r*of*.npy')
    got = model.gather_global_tables(slots=True)
    assert set(model.gather_global_tables()) == {k for k in got if not k.endswith('/Adagrad')}
    if rank == 0:
        np.savez(os.path.join(out_dir, 'saved.npz'), **got)
    if more:
        _run(model, None, rng, syn, world, rank, range(3, 3 + more), state)
        got = model.gather_global_tables(slots=True)
        if rank == 0:
            np.savez(os.path.join(out_dir, 'cont.npz'), **got)
    dist.barrier()
    with open(os.path.join(out_dir, "saved%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def _assert_restored(model, saved, kind):
    got = model.gather_global_tables(slots=True)
    assert set(got) == set(saved.files)
    for k in saved.files:
        assert _bitwise_equal(got[k], saved[k]), k
    assert model.steps == 3 and float(model.lr.item()) == LR
    ni, acc0 = model.ni_loc, float(np.float32(model.acc0))
    assert model.E_item.shape[0] == ni + 1 and not model.E_item[ni].any() and float(model.b_item[ni]) == 0.0
    assert bool((model.A_item[ni] == acc0).all()) and float(model.Ab_item[ni]) == acc0
    if kind != 'hmf':
        nt = model.nt_loc if kind == 'bags' else model.n_tokens
        assert model.E_tok.shape[0] == nt + 1 and not model.E_tok[nt].any() and float(model.b_tok[nt]) == 0.0
        assert bool((model.A_tok[nt] == acc0).all()) and float(model.Ab_tok[nt]) == acc0


def _restore_worker(rank, world, port, out_dir, kind, src_world, src_kind, more):
    """A fresh model (another seed) at `world` restores the latest checkpoint of out_dir (written at src_world by a
    src_kind model), then continues: `more` steps against cont.npz (same world) or one step against the oracle."""
    dist = _init(rank, world, port)
    from arx.utils.checkpoint import latest_checkpoint, read_manifest
    syn, params, tables, extra = _world(kind)
    model = _model(kind, syn, rank, world, extra, seed=77)
    ptrs = [t.data_ptr() for _, t, _, _ in model._checkpoint_arrays()]
    path = latest_checkpoint(out_dir)
    assert path == os.path.join(out_dir, 'ckpt-3')
    assert read_manifest(path)['world'] == src_world
    model.saver.restore(None, path)
    assert ptrs == [t.data_ptr() for _, t, _, _ in model._checkpoint_arrays()]       # written in place
    assert model.n_restores == 1
    saved = np.load(os.path.join(out_dir, 'saved.npz'))
    _assert_restored(model, saved, kind)
    if kind == 'hmf':
        rng, state = np.random.default_rng(5), {}
        if world == src_world:
            _run(None, None, rng, syn, src_world, rank, range(3), state)     # (the stream up to the save)
            model.set_pool(state['pool'])                                    # input data: the caller's, not saved
            _run(model, None, rng, syn, world, rank, range(3, 3 + more), state)
            cont = np.load(os.path.join(out_dir, 'cont.npz'))
            got = model.gather_global_tables(slots=True)
            for k in cont.files:
                assert _bitwise_equal(got[k], cont[k]), k
            assert model.steps == 3 + more
        else:
            ref = _oracle(syn, params, src_world)
            _run(None, ref, rng, syn, src_world, rank, range(3), state)      # the oracle carries its own slots
            model.set_pool(state['pool'])
            _run(model, ref, rng, syn, world, rank, range(3, 4), state)
            got = model.gather_global_tables(slots=True)
            P, A = ref.att_emb.params, ref.att_emb.slots
            for name, key, col in (('user', 'userembed_cat_0', None), ('item', 'itemembed_cat_0', None),
                                   ('item_bias', 'item_bias_cat_0', 0)):
                for suffix, src in (('', P), ('/Adagrad', A)):
                    want = src[key][2:] if col is None else src[key][2:, col]
                    np.testing.assert_allclose(got[name + suffix], want, rtol=1e-4, atol=1e-6, err_msg=name + suffix)
    with open(os.path.join(out_dir, "restored%d" % rank), "w") as f:
        f.write("ok")
    dist.barrier()
    dist.destroy_process_group()


def _spawn(fn, world, port, *args):
    import torch.multiprocessing as mp
    mp.spawn(fn, args=(world, port) + args, nprocs=world, join=True)


@pytest.mark.parametrize("w_save,w_load", [(2, 3), (3, 2), (2, 2), (4, 1)])
def test_sharded_hmf_save_restore_restripe(tmp_path, w_save, w_load):
    port = 28100 + (os.getpid() % 400) + 10 * w_save + w_load
    more = 2 if w_save == w_load else 0
    _spawn(_save_worker, w_save, port, str(tmp_path), 'hmf', more)
    assert all(os.path.exists(tmp_path / ("saved%d" % r)) for r in range(w_save))
    _spawn(_restore_worker, w_load, port + 1000, str(tmp_path), 'hmf', w_save, 'hmf', more)
    assert all(os.path.exists(tmp_path / ("restored%d" % r)) for r in range(w_load))


@pytest.mark.parametrize("src,dst", [('bags', 'rep'), ('rep', 'bags')])
def test_het_token_tables_cross_layouts(tmp_path, src, dst):
    """Token tables striped by token at world 2 (ShardedHMFBags) -> replicated at world 3 (ShardedHMFRepTokens), and
    replicated at world 2 -> striped at world 3: tables and slots bit for bit, 'token' / 'token_bias' included."""
    port = 28600 + (os.getpid() % 400) + (0 if src == 'bags' else 7)
    _spawn(_save_worker, 2, port, str(tmp_path), src, 0)
    _spawn(_restore_worker, 3, port + 1000, str(tmp_path), dst, 2, src, 0)
    assert all(os.path.exists(tmp_path / ("restored%d" % r)) for r in range(3))


# ---- refusals, unfinished saves, damaged files -------------------------------------------------------------------
def _refusal_worker(rank, world, port, out_dir, same_world):
    dist = _init(rank, world, port)
    from arx.utils.checkpoint import array_file
    syn, params, tables, extra = _world('hmf')
    good = os.path.join(out_dir, 'ckpt-3')

    def snapshot(m):
        return [t.clone() for _, t, _, _ in m._checkpoint_arrays()]

    def unchanged(m, snap):
        return all(_bitwise_equal(t.numpy(), s.numpy()) for (_, t, _, _), s in zip(m._checkpoint_arrays(), snap))

    if same_world:
        # another embedding width / another item count: refused, nothing written
        for kw, word in ((dict(d=20), 'd '), (dict(n_items=N_ITEMS - 1), 'n_items')):
            other = _model('hmf', syn, rank, world, extra, seed=3, **kw)
            snap, steps = snapshot(other), other.steps
            with pytest.raises(ValueError) as e:
                other.saver.restore(None, good)
            assert word in str(e.value) and 'item' in str(e.value), str(e.value)
            assert unchanged(other, snap) and other.steps == steps and other.n_restores == 0
        # array files without their manifest: an unfinished save, not a checkpoint
        model = _model('hmf', syn, rank, world, extra, seed=3)
        snap = snapshot(model)
        with pytest.raises((FileNotFoundError, ValueError)):
            model.saver.restore(None, os.path.join(out_dir, 'orphan-9'))
        assert unchanged(model, snap)
    # one float of rank 1's item file is overwritten
    model = _model('hmf', syn, rank, world, extra, seed=3)
    bad = os.path.join(out_dir, 'bad-3')
    with pytest.raises(ValueError) as e:
        model.saver.restore(None, bad)
    msg = str(e.value)
    assert 'fingerprint' in msg and 'item' in msg and 'UNDEFINED' in msg, msg
    assert 'item_bias' not in msg and 'item/Adagrad' not in msg and 'Adagrad' not in msg, msg
    if same_world:
        assert array_file(bad, 'item', 'rows', 1, 2) in msg, msg
    model.saver.restore(None, good)                                  # (and the sound one still loads)
    with open(os.path.join(out_dir, "refused%d_%d" % (world, rank)), "w") as f:
        f.write("ok")
    dist.barrier()
    dist.destroy_process_group()


def test_refusals_index_file_and_damaged_files(tmp_path):
    from arx.utils.checkpoint import get_checkpoint_state, latest_checkpoint
    port = 28900 + (os.getpid() % 400)
    out = str(tmp_path)
    _spawn(_save_worker, 2, port, out, 'hmf', 0)
    # the index file: both saves listed, the second is the latest -- exactly as for the .npz checkpoints
    st = get_checkpoint_state(out)
    assert st.all_model_checkpoint_paths == [os.path.join(out, 'ckpt-2'), os.path.join(out, 'ckpt-3')]
    assert latest_checkpoint(out) == os.path.join(out, 'ckpt-3') == st.model_checkpoint_path
    for f in glob.glob(os.path.join(out, 'ckpt-3.*')):
        tail = os.path.basename(f)[len('ckpt-3'):]
        shutil.copy(f, os.path.join(out, 'bad-3' + tail))
        if not tail.endswith('.manifest.json'):
            shutil.copy(f, os.path.join(out, 'orphan-9' + tail))
    assert not os.path.exists(os.path.join(out, 'orphan-9.manifest.json'))
    assert all('orphan' not in p for p in get_checkpoint_state(out).all_model_checkpoint_paths)
    victim = np.load(os.path.join(out, 'bad-3.item.r1of2.npy'), mmap_mode='r+')
    victim[17, 5] += np.float32(0.25)
    victim.flush()
    del victim
    _spawn(_refusal_worker, 2, port + 1000, out, True)
    assert all(os.path.exists(tmp_path / ("refused2_%d" % r)) for r in range(2))
    _spawn(_refusal_worker, 3, port + 2000, out, False)
    assert all(os.path.exists(tmp_path / ("refused3_%d" % r)) for r in range(3))
