"""Flat {name -> array} checkpoints carrying the reference's variable names.

Replaces tf.train.Saver(tf.global_variables()) (hmf_model.py:156, seqModel.py:184):
tables 'userembed_cat_0', 'itemembed_mulhot_0', biases 'item_bias_cat_0' ([Vf,1]),
dense weights, and the Adagrad slots as '<name>/Adagrad'.

Like tf.train.Saver, save() also maintains a small text file `checkpoint` next to the data file
naming the latest checkpoint, so runner code written as
    ckpt = get_checkpoint_state(dir);  saver.restore(sess, ckpt.model_checkpoint_path)
(run_hmf.py:131-137, lstm/run.py:345-353) finds it: `get_checkpoint_state` / `latest_checkpoint`
below.

The row-sharded models of arx/dist.py (ShardedHMF and its subclasses, SeqHybridParallel) keep the same surface
through ShardedSaver: per-rank .npy files of the owned rows plus one manifest, restorable on another world size.
DESIGN.md section 7 ('Checkpoints of the sharded models') has the format."""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch


INDEX_NAME = 'checkpoint'


class CheckpointState(object):
    """The two fields of tf.train.get_checkpoint_state()'s result the runners read."""

    def __init__(self, model_checkpoint_path, all_model_checkpoint_paths):
        self.model_checkpoint_path = model_checkpoint_path
        self.all_model_checkpoint_paths = all_model_checkpoint_paths


def get_checkpoint_state(checkpoint_dir):
    """None when `checkpoint_dir` holds no index file (the runners then initialise fresh)."""
    idx = os.path.join(checkpoint_dir, INDEX_NAME)
    if not os.path.isfile(idx):
        return None
    latest, every = None, []
    for line in open(idx):
        key, _, val = line.strip().partition(': ')
        val = val.strip('"')
        if not os.path.isabs(val):
            val = os.path.join(checkpoint_dir, val)
        if key == 'model_checkpoint_path':
            latest = val
        elif key == 'all_model_checkpoint_paths':
            every.append(val)
    return CheckpointState(latest, every) if latest else None


def latest_checkpoint(checkpoint_dir):
    st = get_checkpoint_state(checkpoint_dir)
    return st.model_checkpoint_path if st else None


def _update_index(path):
    d = os.path.dirname(path) or '.'
    st = get_checkpoint_state(d)
    every = [os.path.relpath(p, d) for p in (st.all_model_checkpoint_paths if st else [])]
    rel = os.path.relpath(path, d)
    every = [p for p in every if p != rel] + [rel]
    with open(os.path.join(d, INDEX_NAME), 'w') as f:
        f.write('model_checkpoint_path: "%s"\n' % rel)
        for p in every:
            f.write('all_model_checkpoint_paths: "%s"\n' % p)


class Saver(object):
    def __init__(self, model):
        self.model = model

    def _state(self):
        m = self.model
        rt = m.rt
        st = {}
        for t in m.att_emb.tables.values():
            st[t.name] = t.E.cpu().numpy()
            st[t.name + '/Adagrad'] = t.acc.cpu().numpy()
            if t.bias is not None:
                st[t.bias_name] = t.bias.cpu().numpy().reshape(-1, 1)
                st[t.bias_name + '/Adagrad'] = t.bias_acc.cpu().numpy().reshape(-1, 1)
        for p in rt.dense.values():
            st[p.name] = p.w.cpu().numpy()
            st[p.name + '/Adagrad'] = p.acc.cpu().numpy()
        st['global_step'] = np.asarray(rt.global_step, dtype=np.int64)
        st['learning_rate'] = np.asarray(rt.lr_host, dtype=np.float32)
        return st

    def save(self, session, path, global_step=None, write_meta_graph=False):
        if global_step is not None:
            path = '%s-%d' % (path, global_step)
        d = os.path.dirname(path)
        if d and not os.path.isdir(d):
            os.makedirs(d)
        np.savez(path + '.npz', **self._state())
        _update_index(path)
        return path

    def restore(self, session, path):
        if not path.endswith('.npz'):
            path = path + '.npz'
        z = np.load(path)
        m = self.model
        rt = m.rt
        # every variable (and slot) of THIS model must be in the file, with its shape: a checkpoint
        # of a differently configured model (nonlinear / use_concat / other attribute set) is refused
        # before anything is overwritten
        want = {}
        for t in m.att_emb.tables.values():
            want[t.name] = want[t.name + '/Adagrad'] = tuple(t.E.shape)
            if t.bias is not None:
                want[t.bias_name] = want[t.bias_name + '/Adagrad'] = (int(t.bias.shape[0]), 1)
        for p in rt.dense.values():
            want[p.name] = want[p.name + '/Adagrad'] = tuple(p.w.shape)
        missing = sorted(k for k in want if k not in z.files)
        if missing:
            raise KeyError("checkpoint %s lacks %d variable(s) of this model: %s%s"
                           % (path, len(missing), ', '.join(missing[:6]), ' ...' if len(missing) > 6 else ''))
        bad = sorted(k for k, shp in want.items() if tuple(z[k].shape) != shp)
        if bad:
            raise ValueError("checkpoint %s: shape mismatch for %s (file %s, model %s)"
                             % (path, bad[0], tuple(z[bad[0]].shape), want[bad[0]]))
        for t in m.att_emb.tables.values():
            t.E.copy_(torch.from_numpy(z[t.name]))
            t.acc.copy_(torch.from_numpy(z[t.name + '/Adagrad']))
            if t.bias is not None:
                t.bias.copy_(torch.from_numpy(z[t.bias_name].reshape(-1)))
                t.bias_acc.copy_(torch.from_numpy(z[t.bias_name + '/Adagrad'].reshape(-1)))
        for p in rt.dense.values():
            p.w.copy_(torch.from_numpy(z[p.name]))
            p.acc.copy_(torch.from_numpy(z[p.name + '/Adagrad']))
        rt.global_step = int(z['global_step'])
        rt.set_learning_rate(float(z['learning_rate']))


# ---------------------------------------------------------------------------------------------------------------
# Sharded checkpoints
# ---------------------------------------------------------------------------------------------------------------
FORMAT_VERSION = 1
MANIFEST_SUFFIX = '.manifest.json'
FP_K = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1
_CONFIG_KEYS = ('d', 'n_users', 'n_items', 'n_tokens')


def rows_fingerprint(x, row0=0, row_step=1):
    """numpy twin of arx_rows_fingerprint (include/arx.h): sum_j ((2 g_j + 1) K) * sum_c bits(x[j, c]) (2c + 1) mod
    2^64 with g_j = row0 + row_step * j, as a Python int.  x: [rows] (width 1) or [rows, width] float32.  Integer
    arithmetic only, so the sum over the stripes of ANY striping of one table is the same number."""
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise ValueError("rows_fingerprint: float32 rows")
    if x.shape[0] == 0:
        return 0
    x = np.ascontiguousarray(x).reshape(x.shape[0], -1)
    rows, width = x.shape
    bits = x.view(np.uint32).astype(np.uint64)
    inner = (bits * (2 * np.arange(width, dtype=np.uint64) + 1)).sum(axis=1, dtype=np.uint64)
    g = np.uint64(row0) + np.uint64(row_step) * np.arange(rows, dtype=np.uint64)
    return int(((2 * g + 1) * np.uint64(FP_K) * inner).sum(dtype=np.uint64))


def owned_rows(n, layout, rank, world):
    """Rows of an array of n global rows this rank holds: all of them ('replicated') or its stripe ('rows')."""
    return int(n) if layout == 'replicated' else (int(n) - rank + world - 1) // world


def stripe_progression(r, N, rp, Np):
    """Rows of source stripe r of N that belong to destination stripe rp of Np (owner = row % world, local row =
    row // world on both sides): source-local rows j0 + t P land on destination-local rows l0 + t Q, t = 0, 1, ...
    Returns (j0, P, l0, Q), or None when gcd(N, Np) does not divide rp - r (the two stripes share no row)."""
    g = math.gcd(N, Np)
    if (rp - r) % g:
        return None
    P, Q = Np // g, N // g
    j0 = next(j for j in range(P) if (r + N * j) % Np == rp)
    return j0, P, (r + N * j0) // Np, Q


def array_file(path, name, layout, rank, world):
    stem = '%s.%s' % (path, name.replace('/', '.'))
    return stem + ('.rep.npy' if layout == 'replicated' else '.r%dof%d.npy' % (rank, world))


def read_manifest(path):
    """The manifest of checkpoint `path`; a checkpoint without one does not exist (FileNotFoundError)."""
    mf = path + MANIFEST_SUFFIX
    if not os.path.isfile(mf):
        raise FileNotFoundError("no sharded checkpoint at %s: %s is missing (array files without their manifest are "
                                "an unfinished save)" % (path, mf))
    with open(mf) as f:
        m = json.load(f)
    if m.get('format') != 'arx-sharded' or m.get('version') != FORMAT_VERSION:
        raise ValueError("%s: not a sharded checkpoint of format version %d" % (mf, FORMAT_VERSION))
    return m


class ShardedSaver(object):
    """tf.train.Saver's surface (save / restore, the `checkpoint` index file) for the row-sharded models.  Both calls
    are COLLECTIVES: every rank of the owner's group makes them, with the same arguments.

    A checkpoint P (`path`, or `path-<global_step>`) is, per rank and array, one plain .npy file with exactly the rows
    the rank owns (never the zero / padding rows behind them; replicated arrays: rank 0's copy only), and
    P.manifest.json, which rank 0 writes last -- after every rank's files are complete -- and then enters into the
    index file.  Without its manifest a checkpoint does not exist.  The manifest names every array (global rows,
    width, layout 'rows' -- owner = row % world, local row = row // world -- or 'replicated', one fingerprint per
    source rank) and the scalars (step count, learning rate, the owner's sizes).

    restore() takes a checkpoint of ANY world size, and of either layout per array: each destination rank reads, from
    every source file, the arithmetic progression of rows that are its own (stripe_progression) and puts it into the
    strided view of its buffer.  It validates first -- every array of the model in the manifest with the model's
    global rows and width, equal sizes -- and raises before anything is overwritten; then it writes IN PLACE (captured
    step graphs and serving views keep their pointers), resets the padding rows, sets the scalars and tells the owner
    (views refresh).  What it wrote is fingerprinted (arx_rows_fingerprint: exact, independent of the striping) and
    compared with the manifest; a mismatch raises ValueError naming the array -- the tables are then UNDEFINED.

    Rows travel through one pinned staging slab of chunk_bytes (and, where rows are placed by kernel, a device slab
    of the same size): neither call holds a stripe in pageable host memory.

    Not saved: the sampled pool, the positives CSR, exclusion lists and sampler state -- input data that the driver
    owns.  After restore() the caller sets them as after construction (set_pool / set_positives).

    The owner provides rank, world, group, device, _checkpoint_arrays() -> [(name, tensor, global rows, layout)],
    _checkpoint_scalars() -> dict, _checkpoint_set_scalars(dict) and _checkpoint_restored()."""

    def __init__(self, owner, chunk_bytes=64 << 20):
        if int(chunk_bytes) < 4:
            raise ValueError("chunk_bytes must hold at least one float")
        self.owner = owner
        self.chunk_bytes = int(chunk_bytes)

    # ---- plumbing ---------------------------------------------------------------------------------------------
    def _backend(self):
        o = self.owner
        be = getattr(o, 'be', None)
        if be is None and torch.device(o.device).type == 'cuda':
            from ..dist import HipBackend
            be = o.be = HipBackend(torch.device(o.device))
        return be

    def _quiet(self):
        """The owner's stream, joined with the caller's on both sides (ops.joined); None on a CPU device."""
        from .. import ops
        o = self.owner
        return ops.joined(getattr(o, '_stream', None) if getattr(o, 'use_graphs', False) else None)

    def _slabs(self, need_device):
        dev = torch.device(self.owner.device)
        n = self.chunk_bytes // 4
        host = torch.empty(n, dtype=torch.float32, pin_memory=dev.type == 'cuda')
        return host, (torch.empty(n, dtype=torch.float32, device=dev) if need_device and dev.type == 'cuda' else None)

    def _gather_u64(self, vals):
        """[W][len(vals)] Python ints: every rank's 64-bit words (no arithmetic inside the collective)."""
        import torch.distributed as dist
        o = self.owner
        if o.world == 1:
            return [list(vals)]
        cdev = 'cpu' if dist.get_backend(o.group) == 'gloo' else o.device
        mine = torch.tensor([v - (1 << 64) if v >> 63 else v for v in vals] + [0], dtype=torch.int64, device=cdev)
        parts = [torch.empty_like(mine) for _ in range(o.world)]
        dist.all_gather(parts, mine, group=o.group)
        return [[int(v) & _M64 for v in p.cpu().tolist()[:-1]] for p in parts]

    def _fingerprint(self, t, row0, row_step):
        """Fingerprint of the 1-D / 2-D tensor t on its device: the kernel where the backend has it, else the twin."""
        be = self._backend()
        if t.dim() > 2:
            t = t.reshape(t.shape[0], -1)
        if hasattr(be, 'rows_fingerprint'):
            out = torch.zeros(1, dtype=torch.int64, device=t.device)
            be.rows_fingerprint(t, row0, row_step, out)
            return int(out.item()) & _M64
        a = t.detach().numpy()
        width = 1 if a.ndim == 1 else int(a.shape[1])
        step = max(1, self.chunk_bytes // (4 * width))
        fp = 0
        for c0 in range(0, a.shape[0], step):
            fp += rows_fingerprint(a[c0:c0 + step], row0 + row_step * c0, row_step)
        return fp & _M64

    @staticmethod
    def _width(t):
        return int(np.prod(t.shape[1:], dtype=np.int64))      # (1 for a vector)

    # ---- save -------------------------------------------------------------------------------------------------
    def save(self, session, path, global_step=None, write_meta_graph=False):
        o = self.owner
        if global_step is not None:
            path = '%s-%d' % (path, global_step)
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        if o.rank == 0 and os.path.isfile(path + MANIFEST_SUFFIX):
            os.remove(path + MANIFEST_SUFFIX)              # rewritten in place: it does not exist until done again
        host, _ = self._slabs(False)
        arrays, fps = o._checkpoint_arrays(), []
        with self._quiet():
            for name, t, n, layout in arrays:
                if layout == 'replicated' and o.rank != 0:
                    fps.append(0)
                    continue
                rows, width = owned_rows(n, layout, o.rank, o.world), self._width(t)
                src = t[:rows]
                mm = np.lib.format.open_memmap(array_file(path, name, layout, o.rank, o.world), mode='w+',
                                               dtype=np.float32, shape=tuple(src.shape))
                step = max(1, host.numel() // width)
                for c0 in range(0, rows, step):
                    blk = src[c0:c0 + step]
                    stage = host[:blk.numel()].view(blk.shape)
                    stage.copy_(blk)                       # (device -> pinned slab: waits for the owner's stream)
                    mm[c0:c0 + blk.shape[0]] = stage.numpy()
                mm.flush()
                del mm
                r0, rs = (0, 1) if layout == 'replicated' else (o.rank, o.world)
                fps.append(self._fingerprint(src, r0, rs))
        every = self._gather_u64(fps)       # (also the barrier: no rank passes before all files are complete)
        if o.rank == 0:
            man = {'format': 'arx-sharded', 'version': FORMAT_VERSION, 'world': o.world,
                   'scalars': o._checkpoint_scalars(), 'arrays': []}
            for k, (name, t, n, layout) in enumerate(arrays):
                man['arrays'].append({'name': name, 'rows': int(n), 'width': self._width(t), 'layout': layout,
                                      'fingerprints': ['%016x' % every[r][k] for r in
                                                       range(1 if layout == 'replicated' else o.world)]})
            tmp = path + MANIFEST_SUFFIX + '.tmp'
            with open(tmp, 'w') as f:
                json.dump(man, f, indent=1)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path + MANIFEST_SUFFIX)
            _update_index(path)
        self._gather_u64([0])               # (no rank returns before the checkpoint exists)
        return path

    # ---- restore ----------------------------------------------------------------------------------------------
    def _validate(self, path, man, arrays):
        o = self.owner
        have = {a['name']: a for a in man['arrays']}
        bad = []
        mine = o._checkpoint_scalars()
        for k in _CONFIG_KEYS:
            if k in mine and man['scalars'].get(k) != mine[k]:
                bad.append('%s (file %s, model %s)' % (k, man['scalars'].get(k), mine[k]))
        for name, t, n, layout in arrays:
            a = have.get(name)
            if a is None:
                bad.append('%s (not in the file)' % name)
            elif (a['rows'], a['width']) != (int(n), self._width(t)):
                bad.append('%s (file [%d, %d], model [%d, %d])' % (name, a['rows'], a['width'], n, self._width(t)))
            elif layout not in ('rows', 'replicated') or a['layout'] not in ('rows', 'replicated'):
                bad.append('%s (layout %r)' % (name, a['layout']))
            elif (t.dim() > 1 and self._width(t) % 4 and t.device.type != 'cpu' and a['layout'] == 'rows'
                  and (1 if layout == 'replicated' else o.world) % man['world']):
                bad.append('%s (rows of width %d are placed by arx_copy_2d when re-striped: a multiple of 4)'
                           % (name, a['width']))
        if bad:
            raise ValueError("checkpoint %s does not fit this model: %s" % (path, '; '.join(bad)))
        # every source file is there and holds the rows the manifest implies (the header alone is read)
        for name, t, n, layout in arrays:
            a = have[name]
            N = 1 if a['layout'] == 'replicated' else man['world']
            for r in range(N):
                fn = array_file(path, name, a['layout'], r, N)
                if not os.path.isfile(fn):
                    raise ValueError("checkpoint %s: array %s: %s is missing" % (path, name, fn))
                mm = np.load(fn, mmap_mode='r')
                rows = owned_rows(n, a['layout'], r, N)
                if mm.dtype != np.float32 or mm.shape[0] != rows or \
                        int(np.prod(mm.shape[1:], dtype=np.int64)) != a['width']:
                    raise ValueError("checkpoint %s: array %s: %s holds %s %s, not %d float32 rows of width %d"
                                     % (path, name, fn, mm.shape, mm.dtype, rows, a['width']))
                del mm
        return have

    def _load(self, path, name, t, n, layout, src_layout, N, host, dev_slab):
        """The rows of this rank's part of array `name`, from the files of all N source ranks into t, in place."""
        o, be = self.owner, self._backend()
        rp, Np = (0, 1) if layout == 'replicated' else (o.rank, o.world)
        width = self._width(t)
        flat = t if t.dim() <= 2 else t.reshape(t.shape[0], -1)
        cpu = t.device.type == 'cpu'
        for r in range(N):
            prog = stripe_progression(r, N, rp, Np)
            if prog is None:
                continue
            j0, P, l0, Q = prog
            fn = array_file(path, name, src_layout, r, N)
            mm = np.load(fn, mmap_mode='r')
            src_rows = owned_rows(n, src_layout, r, N)                 # (checked against the file in _validate)
            mm = mm.reshape(src_rows, -1) if flat.dim() == 2 else mm.reshape(src_rows)
            count = max(0, (src_rows - j0 + P - 1) // P)
            step = max(1, host.numel() // width)
            for t0 in range(0, count, step):
                k = min(step, count - t0)
                stage = host[:k * width].view((k, width) if flat.dim() == 2 else (k,))
                a = j0 + t0 * P
                np.copyto(stage.numpy(), mm[a:a + (k - 1) * P + 1:P])
                b = l0 + t0 * Q
                dst = flat[b:b + (k - 1) * Q + 1:Q]
                if dst.shape[0] != k:
                    raise ValueError("checkpoint %s: array %s: rows of %s fall outside this rank's stripe" % (path, name, fn))
                if cpu or Q == 1:
                    dst.copy_(stage)                            # contiguous rows (or a CPU device): no kernel
                else:
                    dv = dev_slab[:k * width].view(stage.shape)
                    dv.copy_(stage, non_blocking=True)
                    if flat.dim() == 2:
                        be.copy_2d(dv, dst)
                    else:
                        be.copy_strided(dv, dst)
                if not cpu:
                    torch.cuda.current_stream(t.device).synchronize()   # the slab is free again
            del mm

    def restore(self, session, path):
        o = self.owner
        man = read_manifest(path)
        arrays = o._checkpoint_arrays()
        have = self._validate(path, man, arrays)
        N_src = int(man['world'])
        acc0 = getattr(o, 'acc0', None)
        host, dev_slab = self._slabs(True)
        got = []
        with self._quiet():
            for name, t, n, layout in arrays:
                a = have[name]
                N = 1 if a['layout'] == 'replicated' else N_src
                self._load(path, name, t, n, layout, a['layout'], N, host, dev_slab)
                rows = owned_rows(n, layout, o.rank, o.world)
                if t.shape[0] > rows:                           # the zero / padding rows behind the owned ones
                    if not name.endswith('/Adagrad'):
                        t[rows:].zero_()
                    elif acc0 is not None:
                        t[rows:].fill_(float(acc0))
                r0, rs = (0, 1) if layout == 'replicated' else (o.rank, o.world)
                got.append(self._fingerprint(t[:rows], r0, rs))
            o._checkpoint_set_scalars(man['scalars'])
        o._checkpoint_restored()
        every = self._gather_u64(got)
        wrong = []
        for k, (name, t, n, layout) in enumerate(arrays):
            a = have[name]
            want = [int(x, 16) for x in a['fingerprints']]
            if a['layout'] == layout and (layout == 'replicated' or N_src == o.world):
                for r in range(o.world):                        # file by file (a replicated array: the one file)
                    w = want[0] if layout == 'replicated' else want[r]
                    if every[r][k] != w:
                        wrong.append('%s (rank %d, file %s)' % (name, r, array_file(
                            path, name, layout, 0 if layout == 'replicated' else r, N_src)))
            elif layout == 'replicated':                        # every replica alone holds the whole table
                wrong += ['%s (rank %d)' % (name, r) for r in range(o.world) if every[r][k] != sum(want) & _M64]
            elif sum(every[r][k] for r in range(o.world)) & _M64 != sum(want) & _M64:
                wrong.append(name)
        if wrong:
            raise ValueError("checkpoint %s: fingerprint mismatch after restore for %s -- a file is damaged or rows "
                             "went astray; the model's tables are now UNDEFINED (restore another checkpoint or "
                             "rebuild the model)" % (path, ', '.join(wrong)))
