"""Thin tensor-level wrappers over the C ABI (include/arx.h).

torch tensors are used ONLY as device-memory holders: every function passes
`tensor.data_ptr()` and explicit sizes to libarx.so; no torch arithmetic runs
on the hot path.  All launches go to torch's current HIP stream so that
torch.cuda events / torch.distributed (RCCL) order correctly against them.
"""
from __future__ import annotations

import contextlib
import gc
import math

import os

import torch

from . import _lib
from ._lib import call

KEY_NONE = 0x7FFFFFFF


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_dev_index = None


def _stream():
    """hipStream_t of torch's current stream on the current device.  torch.cuda.current_stream()
    spends ~8 us in device-index plumbing per call -- a third of the host time of a B=64 step --
    so the raw-handle accessor is used where this torch build has it."""
    global _dev_index
    if _raw_stream is None:
        return torch.cuda.current_stream().cuda_stream
    if _dev_index is None:
        _dev_index = torch.cuda.current_device()
    return _raw_stream(_dev_index)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _chk(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise ValueError("%s must be a device tensor (the HIP path has no CPU fallback)" % name)
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous() and t.dim() == 1:
        raise ValueError("%s must be contiguous" % name)


def _ld(t):
    """leading dimension (elements) of a 2-D row-major tensor or view"""
    if t.dim() == 1:
        return t.shape[0]
    if t.stride(-1) != 1:
        raise ValueError("inner dimension must be contiguous")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


class Workspace(object):
    """Grow-only device scratch buffer (caller-owned workspace of the C ABI)."""

    def __init__(self, device):
        self.device = device
        self.buf = None

    def get(self, nbytes):
        nbytes = int(nbytes)
        if nbytes <= 0:
            return 0, 0
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=self.device)
        return self.buf.data_ptr(), self.buf.numel()


def device_info():
    import ctypes as C
    cu, wave, lds = C.c_int(), C.c_int(), C.c_int()
    arch = C.create_string_buffer(64)
    call("arx_device_info", C.byref(cu), C.byref(wave), C.byref(lds), arch, 64)
    return {"cu_count": cu.value, "wave_size": wave.value, "lds_bytes": lds.value,
            "arch": arch.value.decode()}


# ---- a4/a7 ---------------------------------------------------------------
def csr_expand(vals, starts, lens, row_ids, capacity, ws, pad_token=KEY_NONE, pad_seg=-1,
               seg_base=0, coef_scale=1.0, want_coef=False, out=None):
    """batch_slice2 / batch_segids2 (mulhot_index.py:48-67) on device.

    Returns (token_ids[capacity], segids[capacity], offsets[B+1], total[1], coef or None)."""
    B = int(row_ids.shape[0]) if row_ids is not None else int(lens.shape[0])
    dev = vals.device
    for t, n in ((vals, 'vals'), (starts, 'starts'), (lens, 'lens'), (row_ids, 'row_ids')):
        _chk(t, torch.int32, n)
    if out is None:
        tok = torch.empty(capacity, dtype=torch.int32, device=dev)
        seg = torch.empty(capacity, dtype=torch.int32, device=dev)
        offs = torch.empty(B + 1, dtype=torch.int32, device=dev)
        tot = torch.empty(1, dtype=torch.int32, device=dev)
        coef = torch.empty(capacity, dtype=torch.float32, device=dev) if want_coef else None
    else:
        tok, seg, offs, tot, coef = out
    wsp, wsn = ws.get(_lib.lib.arx_csr_expand_workspace_bytes(B))
    call("arx_csr_expand", _p(vals), _p(starts), _p(lens), _p(row_ids), B, _p(tok), _p(seg),
         int(capacity), _p(offs), _p(tot), int(pad_token), int(pad_seg), int(seg_base),
         float(coef_scale), _p(coef), wsp, wsn, _stream())
    return tok, seg, offs, tot, coef


def bag_expand_padded(vals, starts, lens, row_ids, max_len, seg_base, coef_scale, keys_out, src_out,
                      coef_out, pad_token=KEY_NONE):
    """Un-compacted bag expansion for K7 (slot r*max_len + j; pads = pad_token): one launch."""
    B = int(row_ids.shape[0]) if row_ids is not None else int(lens.shape[0])
    if int(keys_out.shape[0]) < B * int(max_len):
        raise ValueError("bag_expand_padded: output buffers hold %d < %d entries"
                         % (int(keys_out.shape[0]), B * int(max_len)))
    call("arx_bag_expand_padded", _p(vals), _p(starts), _p(lens), _p(row_ids), B, int(max_len),
         int(pad_token), int(seg_base), float(coef_scale), _p(keys_out), _p(src_out), _p(coef_out),
         _stream())


def sparse_site_onehot(cat_map, ids, row_base, coef, keys_out, src_out, coef_out):
    call("arx_sparse_site_onehot", _p(cat_map), _p(ids), int(ids.shape[0]), int(row_base),
         float(coef), _p(keys_out), _p(src_out), _p(coef_out), _stream())


def sparse_site_window(cat_map, ids, n, row_base, coef, keys_out, src_out, coef_out):
    """K7 contributions of a context-window lookup (arx_sparse_site_window): ids = n * mb time-major lookups, the n
    lookups of batch row b share gradient row row_base + b."""
    total, n = int(ids.shape[0]), int(n)
    if n < 1 or total % n:
        raise ValueError("sparse_site_window: %d ids are not n = %d windows" % (total, n))
    if int(keys_out.shape[0]) < total:
        raise ValueError("sparse_site_window: output buffers hold %d < %d entries" % (int(keys_out.shape[0]), total))
    call("arx_sparse_site_window", _p(cat_map), _p(ids), n, total // n, int(row_base), float(coef),
         _p(keys_out), _p(src_out), _p(coef_out), _stream())


def gather_window(E, cat_map, ids, n, out, scale=1.0, base=None, base_scale=1.0):
    """out[b] = base_scale * base[b] + scale * sum_t E[cat_map[ids[t * mb + b]]] (arx_gather_window_fwd): the
    context window of mb = len(ids) / n batch rows in one launch; base: [mb, d] or None."""
    _chk(E, torch.float32, 'E'); _chk(ids, torch.int32, 'ids'); _chk(out, torch.float32, 'out')
    _chk(base, torch.float32, 'base')
    total, n = int(ids.shape[0]), int(n)
    if n < 1 or total % n or int(out.shape[0]) != total // n:
        raise ValueError("gather_window: %d ids, n = %d, %d output rows" % (total, n, int(out.shape[0])))
    if base is not None and tuple(base.shape) != (total // n, int(E.shape[1])):
        raise ValueError("gather_window: base must be [mb, d]")
    call("arx_gather_window_fwd", _p(E), _p(cat_map), _p(ids), n, total // n, int(E.shape[1]), float(scale),
         _p(base), _ld(base) if base is not None else 0, float(base_scale), _p(out), _ld(out), _stream())
    return out


def window_slots_fwd(R, slots, n, out, scale=1.0, base=None, base_scale=1.0):
    """out[b] = base_scale * base[b] + scale * sum_t R[slots[t * mb + b], :d] (arx_window_slots_fwd): the context
    window over the rows of a received block, named by slot; d = out's width, R / base / out may be wider views."""
    _chk(R, torch.float32, 'R'); _chk(slots, torch.int32, 'slots'); _chk(out, torch.float32, 'out')
    _chk(base, torch.float32, 'base')
    total, n, d = int(slots.shape[0]), int(n), int(out.shape[1])
    if n < 1 or total % n or int(out.shape[0]) != total // n:
        raise ValueError("window_slots_fwd: %d slots, n = %d, %d output rows" % (total, n, int(out.shape[0])))
    if int(R.shape[1]) != d or (base is not None and tuple(base.shape) != (total // n, d)):
        raise ValueError("window_slots_fwd: R must be [*, d] and base [mb, d]")
    call("arx_window_slots_fwd", _p(R), _ld(R), _p(slots), n, total // n, d, float(scale), _p(base),
         _ld(base) if base is not None else 0, float(base_scale), _p(out), _ld(out), _stream())
    return out


def window_slots_bwd(dX, slots, n, dbase, dR, scale=1.0, base_scale=1.0, acc_dbase=False):
    """dbase[b] (+)= base_scale * dX[b]; dR[slots[t * mb + b]] = scale * dX[b] for every t (arx_window_slots_bwd)."""
    for t, nm in ((dX, 'dX'), (dbase, 'dbase'), (dR, 'dR')):
        _chk(t, torch.float32, nm)
    _chk(slots, torch.int32, 'slots')
    total, n, mb, d = int(slots.shape[0]), int(n), int(dX.shape[0]), int(dX.shape[1])
    if n < 1 or total != n * mb:
        raise ValueError("window_slots_bwd: %d slots, n = %d, %d gradient rows" % (total, n, mb))
    if tuple(dbase.shape) != (mb, d) or int(dR.shape[1]) != d:
        raise ValueError("window_slots_bwd: dbase must be [mb, d] and dR [*, d]")
    call("arx_window_slots_bwd", _p(dX), _ld(dX), _p(slots), n, mb, d, float(scale), float(base_scale), _p(dbase),
         _ld(dbase), 1 if acc_dbase else 0, _p(dR), _ld(dR), _stream())


def shard_route(ids, world, rank, zero_row, rows_out, keys_out):
    call("arx_shard_route", _p(ids), int(ids.shape[0]), int(world), int(rank), int(zero_row),
         _p(rows_out), _p(keys_out), _stream())


def pool_blocks(ids, world, rank, zero_row, cap, counts, gidx=None, my_slots=None, pool_rows=None):
    """Block layout of a pool striped over `world` owners (arx.h); cap == 0: counts only."""
    call("arx_pool_blocks", _p(ids), int(ids.shape[0]), int(world), int(rank), int(zero_row), int(cap),
         _p(counts), _p(gidx), _p(my_slots), _p(pool_rows), _stream())


def copy_2d(src, dst):
    call("arx_copy_2d", _p(src), _ld(src), _p(dst), _ld(dst), int(src.shape[0]), int(src.shape[1]),
         _stream())


def copy_strided(src, dst):
    """dst[i] = src[i] for 1-D fp32 views of any (positive) element stride."""
    call("arx_copy_strided_f32", _p(src), int(src.stride(0)), _p(dst), int(dst.stride(0)),
         int(src.shape[0]), _stream())


def rows_fingerprint(x, row0, row_step, out):
    """out (one int64 device word, zeroed by the caller) += the striping-independent fingerprint of the rows of x
    (1-D of unit stride: rows of width 1; 2-D: any row stride), row j standing for global row row0 + row_step * j
    (arx_rows_fingerprint)."""
    _chk(x, torch.float32, 'x')
    if out.dtype != torch.int64 or out.numel() != 1 or not out.is_cuda:
        raise ValueError("out must be one int64 device word")
    if x.dim() == 1:
        if x.shape[0] > 1 and x.stride(0) != 1:
            raise ValueError("a 1-D x must have unit stride")
        rows, width, ld = int(x.shape[0]), 1, 1
    else:
        rows, width = int(x.shape[0]), int(x.shape[1])
        if rows and width > 1 and x.stride(1) != 1:
            raise ValueError("inner dimension must be contiguous")
        ld = max(width, int(x.stride(0)) if rows > 1 else width)
    call("arx_rows_fingerprint", _p(x), ld, rows, width, int(row0), int(row_step), _p(out), _stream())


# ---- a5 ---------------------------------------------------------------------
def transpose(src, dst):
    """dst[c, r] = src[r, c] for 2-D fp32 views with unit inner stride."""
    rows, cols = int(src.shape[0]), int(src.shape[1])
    call("arx_transpose_f32", _p(src), int(src.stride(0)), rows, cols, _p(dst), int(dst.stride(0)),
         _stream())


def gather_rows_wide(src, rows, dst):
    """dst[r, :] = src[rows[r], :] for 2-D fp32 views of any width (zeros for row indices out of range)."""
    call("arx_gather_rows_wide", _p(src), _ld(src), int(src.shape[0]), _p(rows), int(rows.shape[0]),
         int(dst.shape[1]), _p(dst), _ld(dst), _stream())


def gather_onehot(E, bias, cat_map, ids, out, scale=1.0, accumulate=False, bias_out=None):
    _chk(E, torch.float32, 'E'); _chk(ids, torch.int32, 'ids'); _chk(out, torch.float32, 'out')
    call("arx_gather_onehot_fwd", _p(E), _p(bias), _p(cat_map), _p(ids), int(ids.shape[0]),
         int(E.shape[1]), float(scale), int(bool(accumulate)), _p(out), _ld(out), _p(bias_out),
         _stream())
    return out


def gather_onehot_packed(E, bias, cat_map, ids, out, scale=1.0):
    """out[r] = [scale * E[row] | scale * bias[row] | pad]: packed rows of the sharded exchanges."""
    _chk(E, torch.float32, 'E'); _chk(ids, torch.int32, 'ids'); _chk(out, torch.float32, 'out')
    call("arx_gather_onehot_packed_fwd", _p(E), _p(bias), _p(cat_map), _p(ids), int(ids.shape[0]),
         int(E.shape[1]), float(scale), _p(out), _ld(out), _stream())
    return out


def gather_id_plus_bag(E_id, bias_id, cat_map, E_tok, bias_tok, vals, starts, lens, ids, out, scale=1.0,
                       accumulate=False, bias_out=None):
    """id row + bag mean of one entity in one launch (both scaled by `scale`)."""
    call("arx_gather_id_plus_bag", _p(E_id), _p(bias_id), _p(cat_map), _p(E_tok), _p(bias_tok), _p(vals),
         _p(starts), _p(lens), _p(ids), int(ids.shape[0]), int(E_id.shape[1]), float(scale),
         int(bool(accumulate)), _p(out), _ld(out), _p(bias_out), _stream())


def het_rows_range(E_id, bias_id, E_tok, bias_tok, vals, starts, lens, n_items, world, rank, c0, c1, out,
                   bias_out=None, all_owners=False, scale=0.5, block_rows=0):
    """HET rows (id row + bag mean, times scale) of the shard columns [c0, c1) of owner `rank` -- or, all_owners, of
    every owner, owner s's rows at out[s * block_rows ...) -- with no id array (arx_het_rows_range).  out: 2-D,
    at least d wide; bias_out: a 1-D view of any stride, or None: column d of the out rows (packed d+4 rows)."""
    d = int(E_id.shape[1])
    _chk(E_id, torch.float32, 'E_id'); _chk(E_tok, torch.float32, 'E_tok'); _chk(out, torch.float32, 'out')
    for t, n in ((vals, 'vals'), (starts, 'starts'), (lens, 'lens')):
        _chk(t, torch.int32, n)
    ldo = _ld(out)
    own_rows = (int(n_items) - int(rank) + int(world) - 1) // max(int(world), 1)
    if int(E_id.shape[0]) < own_rows or int(bias_id.shape[0]) < own_rows:
        raise ValueError("het_rows_range: the id shard holds %d rows, rank %d of %d owns %d"
                         % (int(E_id.shape[0]), int(rank), int(world), own_rows))
    if int(starts.shape[0]) < int(n_items) or int(lens.shape[0]) < int(n_items):
        raise ValueError("het_rows_range: the bag index is shorter than n_items")
    nown = int(world) if all_owners else 1
    rows = (nown - 1) * int(block_rows) + int(c1) - int(c0) if nown > 1 else int(c1) - int(c0)
    if int(out.shape[0]) < rows:
        raise ValueError("het_rows_range: out holds %d rows, the range writes %d" % (int(out.shape[0]), rows))
    if bias_out is None:
        if int(out.shape[1]) <= d:
            raise ValueError("het_rows_range: packed rows need a column d in out")
        pb, ldb = _p(out) + 4 * d, ldo
    else:
        if int(bias_out.shape[0]) < rows:
            raise ValueError("het_rows_range: bias_out holds %d cells, the range writes %d"
                             % (int(bias_out.shape[0]), rows))
        pb, ldb = _p(bias_out), int(bias_out.stride(0))
    call("arx_het_rows_range", _p(E_id), _p(bias_id), _p(E_tok), _p(bias_tok), _p(vals), _p(starts), _p(lens),
         int(n_items), int(world), int(rank), int(c0), int(c1), int(bool(all_owners)), d, float(scale), _p(out), ldo,
         pb, ldb, int(block_rows), _stream())


class GatherSet(object):
    """Descriptor arrays of arx_gather_onehot_multi, built once per plan.
    sites: [(E, bias|None, cat_map|None, ids, out, scale, bias_out|None)], equal width d.
    bias_out may be the string 'packed': the bias goes to column d of the site's out rows.
    bias may be an int c: column c of the (packed) table rows themselves."""

    def __init__(self, sites):
        import ctypes as C
        n = len(sites)
        self.n = n
        self.d = int(sites[0][0].shape[1])
        vp = lambda xs: (C.c_void_p * n)(*[(_p(x) or None) for x in xs])
        self.E = vp([s[0] for s in sites])
        colb = [isinstance(s[1], int) for s in sites]
        self.bias = (C.c_void_p * n)(*[(_p(s[0]) + 4 * s[1]) if cb else (_p(s[1]) or None)
                                       for s, cb in zip(sites, colb)])
        self.ldbi = (C.c_int64 * n)(*[self.d if cb else 1 for cb in colb])
        self.cat_map, self.ids = vp([s[2] for s in sites]), vp([s[3] for s in sites])
        packed = [isinstance(s[6], str) for s in sites]
        assert all(s[6] == 'packed' and _ld(s[4]) > self.d for s, pk in zip(sites, packed) if pk)
        self.out = vp([s[4] for s in sites])
        self.bias_out = (C.c_void_p * n)(*[(_p(s[4]) + 4 * self.d) if pk else (_p(s[6]) or None)
                                           for s, pk in zip(sites, packed)])
        self.cnt = (C.c_int64 * n)(*[int(s[3].shape[0]) for s in sites])
        self.ldo = (C.c_int64 * n)(*[_ld(s[4]) for s in sites])
        self.ldb = (C.c_int64 * n)(*[_ld(s[4]) if pk else 1 for s, pk in zip(sites, packed)])
        self.scale = (C.c_float * n)(*[float(s[5]) for s in sites])
        self._keep = sites


def gather_onehot_multi(gs):
    call("arx_gather_onehot_multi", gs.n, gs.E, gs.bias, gs.ldbi, gs.cat_map, gs.ids, gs.cnt, gs.d, gs.scale, gs.out,
         gs.ldo, gs.bias_out, gs.ldb, _stream())


class LookupSet(object):
    """Descriptor arrays of arx_lookup_multi, built once per plan.  sites: [(E_id|None, bias_id|None,
    cat_map|None, E_tok|None, bias_tok|None, vals|None, starts|None, lens|None, ids, out, scale,
    bias_out|None)], equal width d."""

    def __init__(self, sites):
        import ctypes as C
        n = len(sites)
        self.n = n
        self.d = int((sites[0][0] if sites[0][0] is not None else sites[0][3]).shape[1])
        vp = lambda xs: (C.c_void_p * n)(*[(_p(x) or None) for x in xs])
        col = lambda k: vp([s[k] for s in sites])
        self.E_id, self.bias_id, self.cat_map = col(0), col(1), col(2)
        self.E_tok, self.bias_tok, self.vals, self.starts, self.lens = col(3), col(4), col(5), col(6), col(7)
        self.ids, self.out, self.bias_out = col(8), col(9), col(11)
        self.cnt = (C.c_int64 * n)(*[int(s[8].shape[0]) for s in sites])
        self.ldo = (C.c_int64 * n)(*[_ld(s[9]) for s in sites])
        self.scale = (C.c_float * n)(*[float(s[10]) for s in sites])
        self._keep = sites


def lookup_multi(ls):
    call("arx_lookup_multi", ls.n, ls.E_id, ls.bias_id, ls.cat_map, ls.E_tok, ls.bias_tok, ls.vals, ls.starts,
         ls.lens, ls.ids, ls.cnt, ls.d, ls.scale, ls.out, ls.ldo, ls.bias_out, _stream())


def gather_mulhot_mean(E, bias, vals, starts, lens, ids, out, scale=1.0, accumulate=False,
                       bias_out=None):
    _chk(E, torch.float32, 'E'); _chk(ids, torch.int32, 'ids'); _chk(out, torch.float32, 'out')
    call("arx_gather_mulhot_mean_fwd", _p(E), _p(bias), _p(vals), _p(starts), _p(lens), _p(ids),
         int(ids.shape[0]), int(E.shape[1]), float(scale), int(bool(accumulate)), _p(out),
         _ld(out), _p(bias_out), _stream())
    return out


# ---- a9 -----------------------------------------------------------------------
def dot_score(U, T, tbias, score):
    call("arx_dot_score_fwd", _p(U), _ld(U), _p(T), _ld(T), _p(tbias), int(U.shape[0]),
         int(U.shape[1]), _p(score), _stream())
    return score


def dot_score_bwd(U, T, dscore, dU, acc_dU, dT):
    call("arx_dot_score_bwd", _p(U), _ld(U), _p(T), _ld(T), _p(dscore), int(U.shape[0]),
         int(U.shape[1]), _p(dU), _ld(dU), int(bool(acc_dU)), _p(dT),
         _ld(dT) if dT is not None else 0, _stream())


PAIR_KINDS = {'bpr': 0, 'bpr-hinge': 1}


def pair_loss(U, P, pbias, N, nbias, kind, gscale, pos_score, neg_score, batch_loss, neg_ids=None, row_w=None,
              dU=None, acc_dU=False, dP=None, dpbias=None, dN=None, dnbias=None):
    """'bpr' / 'bpr-hinge' over the rows of (U, P, N): scores, loss and -- unless all five gradient tensors are
    None -- the gradients, in one launch (arx.h arx_pair_loss_fwdbwd).  neg_ids: rows with a negative id are void."""
    call("arx_pair_loss_fwdbwd", _p(U), _ld(U), _p(P), _ld(P), _p(pbias), _p(N), _ld(N), _p(nbias), _p(neg_ids),
         _p(row_w), int(U.shape[0]), int(U.shape[1]), PAIR_KINDS[kind], float(gscale), _p(pos_score),
         _p(neg_score), _p(batch_loss), _p(dU), _ld(dU) if dU is not None else 0, int(bool(acc_dU)), _p(dP),
         _ld(dP) if dP is not None else 0, _p(dpbias), _p(dN), _ld(dN) if dN is not None else 0, _p(dnbias),
         _stream())


def pair_loss_slots(U, R, pos_slot, neg_slot, kind, gscale, pos_score, neg_score, batch_loss, row_w=None, dU=None,
                    acc_dU=False, dR=None, auc_counts=None):
    """'bpr' / 'bpr-hinge' over packed rows named by slot (arx.h arx_pair_loss_slots): row r scores U[r] against
    R[pos_slot[r]] and R[neg_slot[r]] (bias in column d) and writes their gradient rows to the same rows of dR.
    neg_slot < 0: a void row.  No slot may be named twice.  auc_counts: int32 [2], (sign sum, live rows)."""
    _chk(pos_slot, torch.int32, "pos_slot")
    _chk(neg_slot, torch.int32, "neg_slot")
    if pos_slot.shape[0] != U.shape[0] or neg_slot.shape[0] != U.shape[0]:
        raise ValueError("pair_loss_slots: one positive and one negative slot per row of U")
    call("arx_pair_loss_slots", _p(U), _ld(U), _p(R), _ld(R), int(R.shape[0]), _p(pos_slot), _p(neg_slot), _p(row_w),
         int(U.shape[0]), int(U.shape[1]), PAIR_KINDS[kind], float(gscale), _p(pos_score), _p(neg_score),
         _p(batch_loss), _p(dU), _ld(dU) if dU is not None else 0, int(bool(acc_dU)), _p(dR),
         _ld(dR) if dR is not None else 0, _p(auc_counts), _stream())


def pair_auc(pos_score, neg_score, neg_ids, out):
    """out[0] = 0.5 - 0.5 * mean sign(neg_score - pos_score) over the rows that are not void (arx.h)."""
    call("arx_pair_auc", _p(pos_score), _p(neg_score), _p(neg_ids), int(pos_score.shape[0]), _p(out), _stream())
    return out


def neg_draw_uniform(users, ex_ptr, ex_cols, V, col2item, seed, step_dev, counter, neg_items, lookup_items=None,
                     out_rank=None):
    """One negative per row, uniform over the logit columns outside the user's sorted list (arx.h
    arx_neg_draw_uniform); -1 for a user without an eligible column."""
    _chk(users, torch.int32, "users")
    _chk(neg_items, torch.int32, "neg_items")
    call("arx_neg_draw_uniform", _p(users), int(users.shape[0]), int(ex_ptr.shape[0]) - 1, _p(ex_ptr), _p(ex_cols),
         int(V), _p(col2item), int(seed) & (2 ** 64 - 1), _p(step_dev), int(counter) & (2 ** 64 - 1),
         _p(neg_items), _p(lookup_items), _p(out_rank), _stream())
    return neg_items


def neg_draw_weighted(users, ex_ptr, ex_cols, ex_cum, cum, V, col2item, seed, step_dev, counter, neg_items,
                      lookup_items=None, out_mass=None):
    """One negative per row, drawn in proportion to integer column weights over the logit columns outside the user's
    sorted list (arx.h arx_neg_draw_weighted); -1 for a user without eligible weight.  cum int64 [V + 1]: the
    exclusive prefix sum of the weights; ex_cum int64, aligned with ex_cols: the prefix sums along each list
    (arx.utils.prepare_train.pair_draw_tables).  out_mass int64 [B]: the drawn point of the eligible mass."""
    _chk(users, torch.int32, "users")
    _chk(neg_items, torch.int32, "neg_items")
    _chk(ex_cols, torch.int32, "ex_cols")
    _chk(ex_cum, torch.int64, "ex_cum")
    _chk(cum, torch.int64, "cum")
    if int(cum.shape[0]) != int(V) + 1 or int(ex_cum.shape[0]) != int(ex_cols.shape[0]):
        raise ValueError("neg_draw_weighted: cum holds V + 1 entries and ex_cum one per entry of ex_cols")
    if out_mass is not None:
        _chk(out_mass, torch.int64, "out_mass")
    call("arx_neg_draw_weighted", _p(users), int(users.shape[0]), int(ex_ptr.shape[0]) - 1, _p(ex_ptr), _p(ex_cols),
         _p(ex_cum), _p(cum), int(V), _p(col2item), int(seed) & (2 ** 64 - 1), _p(step_dev),
         int(counter) & (2 ** 64 - 1), _p(neg_items), _p(lookup_items), _p(out_mass), _stream())
    return neg_items


def neg_draw_hard(users, ex_ptr, ex_cols, ex_cum, cum, V, col2item, seed, step_dev, counter, C, U, umap, P, pbias,
                  col2row, neg_items, lookup_items=None, out_pick=None, out_cand=None, out_score=None):
    """The hardest of C drawn negatives per row, one launch (arx_neg_hard.h arx_neg_draw_hardest): candidate j is the
    column neg_draw_uniform (ex_cum and cum None) / neg_draw_weighted gives at counter + j; it scores
    U[umap[user]] . P[col2row[col]] + pbias[col2row[col]] in slate_scores' arithmetic; the first arg-max wins (a NaN
    counts as -inf).  -1 for a row the plain draw leaves void and for a user without a row of U.  umap, col2row (one
    entry per column), col2item, pbias may be None.  out_pick int32 [B], out_cand int32 [B, >= C], out_score float32
    [B, >= C]: the pick, the columns and the score bits."""
    _chk(users, torch.int32, "users")
    _chk(neg_items, torch.int32, "neg_items")
    _chk(ex_cols, torch.int32, "ex_cols")
    _chk(ex_cum, torch.int64, "ex_cum")
    _chk(cum, torch.int64, "cum")
    if (cum is None) != (ex_cum is None):
        raise ValueError("neg_draw_hard: cum and ex_cum come together (weighted) or not at all (uniform)")
    if cum is not None and (int(cum.shape[0]) != int(V) + 1 or int(ex_cum.shape[0]) != int(ex_cols.shape[0])):
        raise ValueError("neg_draw_hard: cum holds V + 1 entries and ex_cum one per entry of ex_cols")
    _chk(U, torch.float32, "U"); _chk(P, torch.float32, "P"); _chk(pbias, torch.float32, "pbias")
    _chk(umap, torch.int32, "umap"); _chk(col2row, torch.int32, "col2row")
    _chk(out_pick, torch.int32, "out_pick"); _chk(out_cand, torch.int32, "out_cand")
    _chk(out_score, torch.float32, "out_score")
    if U.dim() != 2 or P.dim() != 2 or U.shape[1] != P.shape[1]:
        raise ValueError("neg_draw_hard: U [n_urows, d] and P [n_prows, d]")
    if pbias is not None and (pbias.dim() != 1 or int(pbias.shape[0]) < int(P.shape[0])):
        raise ValueError("neg_draw_hard: pbias needs one entry per row of P")
    if col2row is not None and int(col2row.shape[0]) < int(V):
        raise ValueError("neg_draw_hard: col2row needs one entry per column")
    B = int(users.shape[0])
    for t, name in ((out_cand, "out_cand"), (out_score, "out_score")):
        if t is not None and (t.dim() != 2 or int(t.shape[0]) != B or int(t.shape[1]) < int(C)):
            raise ValueError("neg_draw_hard: %s is [B, >= C]" % name)
    call("arx_neg_draw_hardest", _p(users), B, int(ex_ptr.shape[0]) - 1, _p(ex_ptr), _p(ex_cols), _p(ex_cum), _p(cum),
         int(V), _p(col2item), int(seed) & (2 ** 64 - 1), _p(step_dev), int(counter) & (2 ** 64 - 1), int(C),
         _p(U), _ld(U), int(U.shape[0]), _p(umap), int(umap.shape[0]) if umap is not None else 0,
         _p(P), _ld(P), int(P.shape[0]), _p(pbias), _p(col2row), int(U.shape[1]),
         _p(neg_items), _p(lookup_items), _p(out_pick), _p(out_cand), _ld(out_cand) if out_cand is not None else 0,
         _p(out_score), _ld(out_score) if out_score is not None else 0, _stream())
    return neg_items


# ---- a8 -----------------------------------------------------------------------
# The scorer products run on the bf16 matrix pipe, f32-exact (three exact bf16 pieces per operand, six MFMA terms,
# f32 accumulation: csrc/gemm_bx6.hip) -- the default since round 4; ARX_SCORER_F32=1 selects the f32-input MFMA
# kernels (the A/B reference, bench.py's *_f32mfma sub-results).  Read once per process.
SCORER_F32 = bool(os.environ.get("ARX_SCORER_F32"))
_BX6 = not SCORER_F32
_bx6_ws = {}


def gemm_nt_bx6(A, B, C, col_bias=None):
    """C[M, N] = A[M, K] . B[N, K]^T + col_bias by six bf16 MFMAs per f32 product term (csrc/gemm_bx6.hip):
    every bit of an f32 multiply-add chain at 16/6 of the f32 MFMA peak.  K in {64, 128}, N % 128 == 0."""
    M, K = int(A.shape[0]), int(A.shape[1])
    N = int(B.shape[0])
    ws = _bx6_ws.setdefault(A.device, Workspace(A.device))
    wsp, wsn = ws.get(_lib.lib.arx_gemm_nt_bx6_workspace_bytes(N, K))
    call("arx_gemm_nt_bx6", M, N, K, _p(A), _ld(A), _p(B), _ld(B), _p(col_bias), _p(C), _ld(C), wsp, wsn,
         _stream())
    return C


def gemm(A, B, C, ws, transA=False, transB=False, alpha=1.0, beta=0.0, col_bias=None,
         a_rowsum=None):
    """C[M,N] = alpha * op(A) . op(B) + beta * C + col_bias  (fp32 MFMA);
    a_rowsum[m] = sum_k op(A)[m,k] when given."""
    M, N = int(C.shape[0]), int(C.shape[1])
    K = int(A.shape[0] if transA else A.shape[1])
    kb = int(B.shape[1] if transB else B.shape[0])
    if K != kb:
        raise ValueError("gemm: inner dimensions differ (%d vs %d)" % (K, kb))
    if (_BX6 and transB and not transA and K in (64, 128) and N % 128 == 0 and alpha == 1.0 and beta == 0.0
            and a_rowsum is None and M >= 4096):
        return gemm_nt_bx6(A, B, C, col_bias)
    wsp, wsn = ws.get(_lib.lib.arx_gemm_f32_workspace_bytes(M, N, K))
    call("arx_gemm_f32", int(bool(transA)), int(bool(transB)), M, N, K, float(alpha), _p(A),
         _ld(A), _p(B), _ld(B), float(beta), _p(C), _ld(C), _p(col_bias), _p(a_rowsum), wsp, wsn,
         _stream())
    return C


def gemm_tn_pair_supported(M, N1, N2, K):
    """The shape class of gemm_tn_pair (include/arx.h: arx_gemm_f32_tn_pair)."""
    return (N1 % 4 == 0 and N2 % 4 == 0 and 32 < N1 + N2 <= 128 and M >= 64 and M % 4 == 0 and
            K >= 64 and K % 32 == 0)


def gemm_tn_pair(A, B1, B2, shift, Ct, ws, a_rowsum=None):
    """Ct [N1 + N2, M] = (A^T . [B1 | B2 shifted down by `shift` rows])^T in one pass over A [K, M]
    (the LSTM cell's dW with A = dz, B1 = x, B2 = the cell outputs, shift = B), a_rowsum = A's column sums."""
    K, M = int(A.shape[0]), int(A.shape[1])
    N1, N2 = int(B1.shape[1]), int(B2.shape[1])
    wsp, wsn = ws.get(_lib.lib.arx_gemm_f32_tn_pair_workspace_bytes(M, N1 + N2, K))
    call("arx_gemm_f32_tn_pair", M, N1, N2, K, _p(A), _ld(A), _p(B1), _ld(B1), _p(B2), _ld(B2), int(shift),
         _p(Ct), _ld(Ct), _p(a_rowsum), wsp, wsn, _stream())
    return Ct


def gemm_steps_tn(A, B, C_steps, rowsum_steps, steps, Kb, C_sum=None, beta=0.0, rowsum_sum=None):
    """C_steps[t] = A_t^T . B_t for every time step t (rows t*Kb..), plus the sums."""
    M, N = int(C_steps.shape[1]), int(C_steps.shape[2])
    call("arx_gemm_f32_steps_tn", int(steps), M, N, int(Kb), _p(A), _ld(A), _p(B), _ld(B),
         _p(C_steps), _p(rowsum_steps), float(beta), _p(C_sum),
         _ld(C_sum) if C_sum is not None else 0, _p(rowsum_sum), _stream())


def dot_scaled(x, y, scale, out, n=None):
    call("arx_dot_scaled", _p(x), _p(y), int(x.numel() if n is None else n), float(scale), _p(out),
         _stream())


def inv_len_scale(lens, ids, c, out):
    call("arx_inv_len_scale", _p(lens), _p(ids), int(out.numel()), float(c), _p(out), _stream())


# ---- a14 ------------------------------------------------------------------------
def pos_mask_scatter(user_ids, pos_ptr, pos_items, item2slot, mask, value):
    call("arx_pos_mask_scatter", _p(user_ids), int(user_ids.shape[0]), _p(pos_ptr), _p(pos_items),
         _p(item2slot), _p(mask), _ld(mask), int(value), _stream())


def _slot_map_detach(ptr, _bits_keepalive):
    import ctypes as C
    try:
        _lib.lib.arx_slot_map_attach_bitmap(C.c_void_p(ptr), None)
    except Exception:
        pass


def slot_map_attach_bitmap(item2slot, bits):
    """Register the "in the pool?" bitmap (int32 zeros [(items + 32) // 32]) of an item2slot map.
    The registration is keyed by the map's device address: it is dropped when the map TENSOR is
    collected (weakref finaliser, which also keeps `bits` alive until then), so a stale entry can
    never meet a new allocation at the same address.  Best effort: with 16 maps registered the call
    is a no-op and the losses probe the map directly."""
    import weakref
    call("arx_slot_map_attach_bitmap", _p(item2slot), _p(bits))       # (bits None: detach)
    if bits is not None:
        weakref.finalize(item2slot, _slot_map_detach, item2slot.data_ptr(), bits)


def slot_map_set(item2slot, ids, clear=False):
    call("arx_slot_map_set", _p(item2slot), _p(ids), int(ids.shape[0]), int(bool(clear)), _stream())


# ---- a10-a12 -----------------------------------------------------------------------
def loss_mw(logits, tscore, mask, batch_loss, dlogits, dtscore, gscale, row_w=None,
            mask_rows=0, kind='mw'):
    """kind 'mw' (WMRB hinge, embed_attribute.py:641-649) or 'mce' (build-defined sampled softmax)."""
    B, S = int(logits.shape[0]), int(logits.shape[1])
    call("arx_loss_%s_fwdbwd" % kind, _p(logits), _ld(logits), _p(tscore), _p(mask),
         _ld(mask) if mask is not None else 0, int(mask_rows), float(gscale), _p(row_w), B, S,
         _p(batch_loss), _p(dlogits), _ld(dlogits) if dlogits is not None else 0, _p(dtscore),
         _stream())


def loss_warp(logits, target, mask, batch_loss, dlogits, gscale, row_w=None, mask_rows=0):
    B, V = int(logits.shape[0]), int(logits.shape[1])
    call("arx_loss_warp_fwdbwd", _p(logits), _ld(logits), _p(target), _p(mask),
         _ld(mask) if mask is not None else 0, int(mask_rows), float(gscale), _p(row_w), B, V,
         _p(batch_loss), _p(dlogits), _ld(dlogits) if dlogits is not None else 0, _stream())


POS_MASK_MAX_COLS = 1 << 20


def loss_mw_pos(logits, tscore, user_ids, pos_ptr, pos_items, item2slot, batch_loss, dlogits,
                dtscore, gscale, row_w=None, mask_rows=0, kind='mw'):
    B, S = int(logits.shape[0]), int(logits.shape[1])
    call("arx_loss_%s_fwdbwd_pos" % kind, _p(logits), _ld(logits), _p(tscore), _p(user_ids), _p(pos_ptr),
         _p(pos_items), _p(item2slot), int(mask_rows), float(gscale), _p(row_w), B, S,
         _p(batch_loss), _p(dlogits), _ld(dlogits) if dlogits is not None else 0, _p(dtscore),
         _stream())


def loss_mw_fused_pos(logits, U, T, tbias, user_ids, pos_ptr, pos_items, item2slot, batch_loss, dlogits,
                      tscore_out, dtscore, dU, dT, gscale, row_w=None, mask_rows=0, kind='mw'):
    """'mw' (or 'mce') loss with the target score t = U.T + tbias, dT = dt*U and dU = dt*T formed by the
    same kernel (dU is WRITTEN: accumulate the scorer's dU onto it afterwards)."""
    B, S = int(logits.shape[0]), int(logits.shape[1])
    call("arx_loss_%s_fused_pos" % kind, _p(logits), _ld(logits), _p(U), _ld(U), _p(T), _ld(T), _p(tbias),
         int(tbias.stride(0)) if tbias is not None else 1, int(U.shape[1]), _p(user_ids), _p(pos_ptr),
         _p(pos_items), _p(item2slot), int(mask_rows), float(gscale), _p(row_w), B, S, _p(batch_loss),
         _p(dlogits), _ld(dlogits) if dlogits is not None else 0, _p(tscore_out), _p(dtscore),
         int(dtscore.stride(0)) if dtscore is not None else 1, _p(dU),
         _ld(dU) if dU is not None else 0, _p(dT), _ld(dT) if dT is not None else 0, _stream())


def eval_chunk_accum(logits, tscore, mode, first, acc0, acc1):
    call("arx_eval_chunk_accum", _p(logits), _ld(logits), int(logits.shape[0]), int(logits.shape[1]), _p(tscore),
         int(mode), int(bool(first)), _p(acc0), _p(acc1), _stream())


def eval_warp_unmask(U, P, pbias, tscore, user_ids, pos_ptr, pos_items, item2col, s_acc, mask_rows=0):
    call("arx_eval_warp_unmask", _p(U), _ld(U), _p(P), _ld(P), _p(pbias), int(U.shape[1]), _p(tscore), _p(user_ids),
         _p(pos_ptr), _p(pos_items), _p(item2col), int(mask_rows), int(U.shape[0]), int(P.shape[0]), _p(s_acc),
         _stream())


def eval_finish(mode, acc0, acc1, tscore, out):
    call("arx_eval_finish", int(mode), _p(acc0), _p(acc1), _p(tscore), int(out.shape[0]), _p(out), _stream())


def mw_scorer_supported(B, S, d):
    """True when the fused 'mw' scorer (csrc/scorer.hip) takes this shape: d in {64, 128}, S % 128 == 0,
    128 <= S <= 2048 -- and the process has not asked for the f32-MFMA reference (ARX_SCORER_F32)."""
    return (not SCORER_F32) and bool(_lib.lib.arx_mw_scorer_supported(int(B), int(S), int(d)))


class MwScorer(object):
    """The 'mw' scorer of a training step on the bf16 matrix pipe, f32-exact (include/arx.h, "a8-a11 fused"):
    fwd() forms target score, act bits, loss and row factors without [B, S] logits; bwd_dU() / bwd_dI() are the two
    backward products out of the bits.  Owns the caller-side state buffer (one per model and stream)."""

    def __init__(self, B, S, d, device):
        import ctypes as C
        self.B, self.S, self.d = int(B), int(S), int(d)
        n = int(_lib.lib.arx_mw_scorer_state_bytes(self.B, self.S, self.d))
        if n == 0:
            raise ValueError("MwScorer: shape not supported (B=%d, S=%d, d=%d)" % (B, S, d))
        self.state = torch.zeros(n, dtype=torch.uint8, device=device)
        lay = (C.c_int64 * 6)()
        call("arx_mw_scorer_state_layout", self.B, self.S, self.d, lay)
        self.Bp = int(lay[4])
        ld, ldt = int(lay[1]), int(lay[5])
        i32 = self.state.view(torch.int32)
        self.act_bits = i32[lay[0] // 4: lay[0] // 4 + (self.S // 32) * ld].view(self.S // 32, ld)     # word-major
        self.act_bits_t = i32[lay[2] // 4: lay[2] // 4 + (self.Bp // 32) * ldt].view(self.Bp // 32, ldt)[:, :self.S]
        self.g = self.state.view(torch.float32)[lay[3] // 4: lay[3] // 4 + self.Bp]
        self.ws = Workspace(device)

    def fwd(self, U, P, pbias, T, tbias, user_ids, pos_ptr, pos_items, item2slot, batch_loss, tscore_out, dtscore,
            dU, dT, gscale, row_w=None, mask_rows=0, phases=7, seq_w=None, seq_rows=0):
        """phases: 1 pool planes + hit lists, 2 hinge GEMM, 4 row kernel (arx_mw_scorer_fwd).  seq_w (the
        sequence model's raw example weights, [L * seq_rows]): row_w is WRITTEN by phase 1 (normalised over time)."""
        call("arx_mw_scorer_fwd", _p(U), _ld(U), _p(P), _ld(P), _p(pbias), _p(T), _ld(T), _p(tbias),
             int(tbias.stride(0)) if tbias is not None else 1, self.d, _p(user_ids), _p(pos_ptr), _p(pos_items),
             _p(item2slot), int(mask_rows), float(gscale), _p(row_w), _p(seq_w), int(seq_rows), self.B, self.S,
             _p(batch_loss), _p(tscore_out), _p(dtscore), int(dtscore.stride(0)) if dtscore is not None else 1,
             _p(dU), _ld(dU) if dU is not None else 0, _p(dT), _ld(dT) if dT is not None else 0, _p(self.state),
             int(self.state.numel()), int(phases), _stream())

    def bwd_dU(self, dU, beta=1.0):
        """dU = beta dU + g * (act . P)"""
        call("arx_mw_scorer_bwd_du", self.B, self.S, self.d, _p(self.state), float(beta), _p(dU), _ld(dU), _stream())

    def bwd_dI(self, dI, db=None, beta=0.0, step_rows=0, dI_steps=None, db_steps=None, loss=None):
        """dI = beta dI + act^T . (g U), db = act^T . g; step_rows > 0: the per-time-step products too; loss =
        (batch_loss [B], gscale, row_w [B] or None, out [1]): out = gscale * sum_r row_w_r * batch_loss_r, the step's
        scalar, out of the same reduce launch."""
        wsp, wsn = (None, 0)
        if dI_steps is None:
            wsp, wsn = self.ws.get(_lib.lib.arx_mw_scorer_bwd_di_workspace_bytes(self.B, self.S, self.d,
                                                                                 int(step_rows)))
        bl, gs, rw, out = loss if loss is not None else (None, 0.0, None, None)
        call("arx_mw_scorer_bwd_di", self.B, self.S, self.d, _p(self.state), int(step_rows), float(beta), _p(dI),
             _ld(dI), _p(db), _p(dI_steps), _p(db_steps), _p(bl), float(gs), _p(rw), _p(out), wsp, wsn, _stream())


def gemm_bt_bx6_supported(M, N, K):
    """arx_gemm_bt_bx6 takes this shape (N % 32 == 0, N <= 128, K in {64, 128, 256}) and the six-term family is on."""
    return (not SCORER_F32) and bool(_lib.lib.arx_gemm_bt_bx6_supported(int(M), int(N), int(K)))


def gemm_bt_bx6(A, Bt, C, beta=0.0):
    """C = beta C + A . Bt^T, six-term f32-exact, Bt [N, K] k-contiguous (the LSTM's dx = dz . W_x^T with Bt = W_x)."""
    M, K = int(A.shape[0]), int(A.shape[1])
    N = int(Bt.shape[0])
    call("arx_gemm_bt_bx6", M, N, K, _p(A), _ld(A), _p(Bt), _ld(Bt), float(beta), _p(C), _ld(C), _stream())


def mce_scorer_supported(B, S, d):
    """True when the fused 'mce' family (csrc/scorer.hip, k_mc_flow) takes this shape: d in {64, 128}, S % 128 == 0,
    128 <= S <= 2048 -- and the process has not asked for the materialising reference (ARX_SCORER_F32 /
    ARX_MCE_FUSED=0)."""
    if SCORER_F32 or os.environ.get('ARX_MCE_FUSED', '1') == '0':
        return False
    return bool(_lib.lib.arx_mce_scorer_supported(int(B), int(S), int(d)))


class MceScorer(object):
    """The build-defined sampled softmax 'mce' without [B, S] logits or weights in HBM (include/arx.h, "'mce' on the
    fused family"): fwd() leaves loss, target-score terms and the COMPLETE latent gradient (one pass forms s_r and
    O_r = sum_s e_rs P_s); bwd_dI() recomputes the weight tiles for the pool-side product.  Same surface as MwScorer
    (bwd_dU is a no-op kept for the graph nodes that drive both)."""

    def __init__(self, B, S, d, device):
        self.B, self.S, self.d = int(B), int(S), int(d)
        n = int(_lib.lib.arx_mce_scorer_state_bytes(self.B, self.S, self.d))
        if n == 0:
            raise ValueError("MceScorer: shape not supported (B=%d, S=%d, d=%d)" % (B, S, d))
        self.state = torch.zeros(n, dtype=torch.uint8, device=device)
        self.ws = Workspace(device)
        self._pbias, self._mask_rows = None, 0

    def fwd(self, U, P, pbias, T, tbias, user_ids, pos_ptr, pos_items, item2slot, batch_loss, tscore_out, dtscore,
            dU, dT, gscale, row_w=None, mask_rows=0, phases=7, seq_w=None, seq_rows=0):
        self._pbias, self._mask_rows = pbias, int(mask_rows)
        call("arx_mce_scorer_fwd", _p(U), _ld(U), _p(P), _ld(P), _p(pbias), _p(T), _ld(T), _p(tbias),
             int(tbias.stride(0)) if tbias is not None else 1, self.d, _p(user_ids), _p(pos_ptr), _p(pos_items),
             _p(item2slot), int(mask_rows), float(gscale), _p(row_w), _p(seq_w), int(seq_rows), self.B, self.S,
             _p(batch_loss), _p(tscore_out), _p(dtscore), int(dtscore.stride(0)) if dtscore is not None else 1,
             _p(dU), _ld(dU) if dU is not None else 0, _p(dT), _ld(dT) if dT is not None else 0, _p(self.state),
             int(self.state.numel()), int(phases), _stream())

    def bwd_dU(self, dU, beta=1.0):
        """(the forward wrote dU = coef O + dt T: nothing left to add)"""
        if beta != 1.0:
            raise RuntimeError("MceScorer: the latent gradient is written by fwd(); bwd_dU(beta != 1) would drop it")

    def bwd_dI(self, dI, db=None, beta=0.0, step_rows=0, dI_steps=None, db_steps=None, loss=None):
        wsp, wsn = self.ws.get(_lib.lib.arx_mce_scorer_bwd_di_workspace_bytes(self.B, self.S, self.d, int(step_rows)))
        bl, gs, rw, out = loss if loss is not None else (None, 0.0, None, None)
        call("arx_mce_scorer_bwd_di", self.B, self.S, self.d, _p(self.state), _p(self._pbias), self._mask_rows,
             int(step_rows),
             float(beta), _p(dI), _ld(dI), _p(db), _p(dI_steps), _p(db_steps), _p(bl), float(gs), _p(rw), _p(out),
             wsp, wsn, _stream())


def loss_warp_pos(logits, target, user_ids, pos_ptr, pos_items, item2slot, batch_loss, dlogits,
                  gscale, row_w=None, mask_rows=0):
    B, V = int(logits.shape[0]), int(logits.shape[1])
    call("arx_loss_warp_fwdbwd_pos", _p(logits), _ld(logits), _p(target), _p(user_ids), _p(pos_ptr),
         _p(pos_items), _p(item2slot), int(mask_rows), float(gscale), _p(row_w), B, V,
         _p(batch_loss), _p(dlogits), _ld(dlogits) if dlogits is not None else 0, _stream())


def item_frequency(item_ids, n_items, counts, weights=None, total=0, power=0.5):
    """counts[v] += #(item_ids == v); weights (optional) = (counts / total)^power, 0 where unseen."""
    n = 0 if item_ids is None else int(item_ids.shape[0])
    call("arx_item_frequency", _p(item_ids), n, int(n_items), int(total), float(power), _p(counts),
         _p(weights), _stream())


def sample_wor(weights, S, seed, counter, out, ws, key_cap=0.0, out_keys=None):
    """Weighted sampling without replacement on device (exponential race); out: int32 [S].
    key_cap > 0: pre-filter for very large item sets.  out_keys (float32 [S]): the race keys of
    the drawn items, ascending (arx_sample_wor)."""
    n = int(weights.shape[0])
    wsp, wsn = ws.get(_lib.lib.arx_sample_wor_workspace_bytes(n, int(S), float(key_cap)))
    call("arx_sample_wor", _p(weights), n, int(S), int(seed) & (2 ** 64 - 1),
         int(counter) & (2 ** 64 - 1), float(key_cap), _p(out), _p(out_keys), wsp, wsn, _stream())
    return out


RS_KINDS = {'rs': 0, 'rs-sig': 1, 'rs-sig2': 2, 'bbpr': 3}
RS_FUNCS = {'log': 0, 'exp': 1, 'poly': 2, 'poly2': 3, 'linear': 4, 'square': 5}


def loss_rs(logits, target, kind, loss_func, exp_p, batch_loss, dlogits, gscale, mask=None,
            pos=None, row_w=None, mask_rows=0):
    """rs / rs-sig / rs-sig2 / bbpr over full logits.  pos = (user_ids, pos_ptr, pos_items,
    item2slot) builds the mask on the fly; else `mask` (uint8 [rows, V]) or no mask."""
    B, V = int(logits.shape[0]), int(logits.shape[1])
    uid, ptr, items, i2s = pos if pos is not None else (None, None, None, None)
    call("arx_loss_rs_fwdbwd", _p(logits), _ld(logits), _p(target), _p(mask),
         _ld(mask) if mask is not None else 0, _p(uid), _p(ptr), _p(items), _p(i2s), int(mask_rows),
         RS_KINDS[kind], RS_FUNCS[loss_func], float(exp_p), float(gscale), _p(row_w), B, V,
         _p(batch_loss), _p(dlogits), _ld(dlogits) if dlogits is not None else 0, _stream())


def row_logsumexp(logits, out):
    call("arx_row_logsumexp", _p(logits), _ld(logits), int(logits.shape[0]), int(logits.shape[1]),
         _p(out), _stream())
    return out


def loss_ce(logits, target, batch_loss, dlogits, gscale, row_w=None):
    B, V = int(logits.shape[0]), int(logits.shape[1])
    call("arx_loss_ce_fwdbwd", _p(logits), _ld(logits), _p(target), float(gscale), _p(row_w), B, V,
         _p(batch_loss), _p(dlogits), _ld(dlogits) if dlogits is not None else 0, _stream())


def loss_warp_eval(logits, target, mask, margin_rank, true_rank, mask_rows=0):
    B, V = int(logits.shape[0]), int(logits.shape[1])
    call("arx_loss_warp_eval", _p(logits), _ld(logits), _p(target), _p(mask),
         _ld(mask) if mask is not None else 0, int(mask_rows), B, V, _p(margin_rank),
         _p(true_rank), _stream())


# ---- a17 ---------------------------------------------------------------------------
def key_bits_for(nrows):
    return max(1, int(math.ceil(math.log2(max(2, int(nrows))))))


def sparse_adagrad(E, acc, bias, bias_acc, keys, src, coef, G, Gb, lr_dev, ws, gscale_dev=None,
                   n=None, aux_cnt=None):
    """aux_cnt (int32[table rows], zeros): enables the one-launch apply (ticket)."""
    n = int(keys.shape[0]) if n is None else int(n)
    wsp, wsn = ws.get(_lib.lib.arx_sparse_adagrad_workspace_bytes(n))
    call("arx_sparse_adagrad", _p(E), _p(acc), _p(bias), _p(bias_acc), int(E.shape[1]),
         _p(keys), _p(src), _p(coef), n, _p(G), _ld(G), _p(Gb), _p(lr_dev), _p(gscale_dev),
         key_bits_for(E.shape[0]), _p(aux_cnt), wsp, wsn, _stream())


class CatSiteArgs(object):
    """Host-side descriptor arrays of arx_sparse_adagrad_cat, built once per plan."""

    def __init__(self, sites):
        import ctypes as C
        n = len(sites)
        self.n = n
        self.total = sum(int(s[2].shape[0]) for s in sites)
        self.cat_map = (C.c_void_p * n)(*[_p(s[0]) or None for s in sites])
        self.ids = (C.c_void_p * n)(*[_p(s[2]) for s in sites])
        self.count = (C.c_int64 * n)(*[int(s[2].shape[0]) for s in sites])
        self.row_base = (C.c_int32 * n)(*[int(s[3]) for s in sites])
        self.coef = (C.c_float * n)(*[float(s[4]) for s in sites])
        self._keep = sites


# The halves of a K7 pass (include/arx.h: arx_sparse_adagrad_cat_multi, _cat_multi_bags, _bags).  The
# two halves of a pass take the same arguments and the same, otherwise untouched, workspace.
K7_SORT = 1              # key generation + sort(s): needs the lookup ids only (side stream, under the GEMMs)
K7_APPLY = 2             # apply: needs the gradient arena
K7_BOTH = 3              # both halves in one call
# ... each half split again for a pass with a riding bag table, so the token chain can run under the one-hot apply:
K7_SORT_HOT = 5          # the one-hot keys + sort (+ the bag offsets; static token order: marks the live pairs)
K7_SORT_TOKENS = 6       # the token chain (needs 5; static token order: sweeps the marks out)
K7_APPLY_HOT = 7         # the one-hot apply, merged entity rows as its side output (needs 5 and the arena)
K7_APPLY_TOKENS = 8      # the token apply (needs 6 and 7)
# the rider's apply form, OR-ed into every phase of a pass (0: the process default ARX_K7_RIDER):
K7_FORM_SPLIT = 0x100    # `split`: table 0's runs alone, then ONE launch with the token runs and the other tables' runs
K7_FORM_WIN = 0x200      # `win`: window + finish launches, then the token apply
# the halves of the lone one-hot pass (arx_sparse_adagrad_cat's `mode`):
K7_CAT_BOTH = 0          # the whole sorted pass
K7_CAT_SORT = 0x10       # its first half: contributions + sort (ids only)
K7_CAT_APPLY = 0x20      # its second half: apply
K7_CAT_MODE = {K7_BOTH: K7_CAT_BOTH, K7_SORT: K7_CAT_SORT, K7_APPLY: K7_CAT_APPLY}     # pass phase -> `mode`


def k7_is_sort(phase):
    """phase is a sort half (or a part of one): it reads the lookup ids only."""
    return phase in (K7_SORT, K7_SORT_HOT, K7_SORT_TOKENS)


def k7_is_apply(phase):
    """phase is an apply half (or a part of one): it reads the gradient arena and the sort half's lists."""
    return phase in (K7_APPLY, K7_APPLY_HOT, K7_APPLY_TOKENS)


def sparse_adagrad_cat(E, acc, bias, bias_acc, site_args, G, Gb, lr_dev, aux_first, aux_cnt,
                       aux_hot, keys_buf, src_buf, coef_buf, ws, gscale_dev=None, mode=K7_CAT_BOTH):
    """sites: list of (cat_map|None, _, ids, row_base, coef) packed in CatSiteArgs.
    mode K7_CAT_BOTH: fused keygen + LDS sort + Adagrad passes (n <= 16384) else atomic election; K7_CAT_SORT /
    K7_CAT_APPLY: its halves."""
    wsp, wsn = ws.get(_lib.lib.arx_sparse_adagrad_workspace_bytes(site_args.total))
    call("arx_sparse_adagrad_cat", _p(E), _p(acc), _p(bias), _p(bias_acc), int(E.shape[0]),
         int(E.shape[1]), site_args.n, site_args.cat_map, site_args.ids, site_args.count,
         site_args.row_base, site_args.coef, _p(G), _ld(G), _p(Gb), _p(lr_dev), _p(gscale_dev),
         _p(aux_first), _p(aux_cnt), _p(aux_hot), int(aux_hot.numel()), _p(keys_buf), _p(src_buf),
         _p(coef_buf), int(mode), wsp, wsn, _stream())


class MultiCatArgs(object):
    """Host-side descriptor arrays of arx_sparse_adagrad_cat_multi, built once per plan.
    tables: list of (E, acc, bias|None, bias_acc|None, aux_cnt|None);
    sites: list of (table_index, cat_map|None, ids, row_base, coef)."""

    def __init__(self, tables, sites, extra=()):
        """extra: [(table_index, n)] pre-expanded segments (arx_csr_expand output) that follow
        the one-hot contributions in keys_buf / src_buf / coef_buf."""
        import ctypes as C
        nt, ns = len(tables), len(sites)
        self.nt, self.ns = nt, ns
        # a table may be VIRTUAL -- (None, None, None, None, None, rows): entity ids of a bag table
        # riding on the pass (arx_sparse_adagrad_cat_multi_bags), no rows of its own
        self.d = int(next(t[0] for t in tables if t[0] is not None).shape[1])
        self.n_cat = sum(int(s[2].shape[0]) for s in sites)
        self.nx = len(extra)
        self.extra_n = (C.c_int64 * max(self.nx, 1))(*[int(e[1]) for e in extra])
        self.extra_table = (C.c_int32 * max(self.nx, 1))(*[int(e[0]) for e in extra])
        self.extra_off = []
        off = self.n_cat
        for e in extra:
            self.extra_off.append(off)
            off += int(e[1])
        self.total = off
        self.E = (C.c_void_p * nt)(*[_p(t[0]) for t in tables])
        self.acc = (C.c_void_p * nt)(*[_p(t[1]) for t in tables])
        self.bias = (C.c_void_p * nt)(*[_p(t[2]) or None for t in tables])
        self.bias_acc = (C.c_void_p * nt)(*[_p(t[3]) or None for t in tables])
        self.rows = (C.c_int64 * nt)(*[int(t[0].shape[0]) if t[0] is not None else int(t[5]) for t in tables])
        self.cnt = (C.c_void_p * nt)(*[_p(t[4]) or None for t in tables])
        m = max(ns, 1)
        self.site_table = (C.c_int32 * m)(*[int(s[0]) for s in sites])
        self.cat_map = (C.c_void_p * m)(*[_p(s[1]) or None for s in sites])
        self.ids = (C.c_void_p * m)(*[_p(s[2]) for s in sites])
        self.count = (C.c_int64 * m)(*[int(s[2].shape[0]) for s in sites])
        self.row_base = (C.c_int32 * m)(*[int(s[3]) for s in sites])
        self.coef = (C.c_float * m)(*[float(s[4]) for s in sites])
        self._keep = (tables, sites)


def sparse_adagrad_cat_multi(args, G, Gb, lr_dev, keys_buf, src_buf, coef_buf, ws, gscale_dev=None, phase=K7_BOTH):
    """phase K7_SORT: key generation + sort (needs the ids only), K7_APPLY: apply, K7_BOTH: both.  The two
    halves must use the same workspace object, untouched in between."""
    wsp, wsn = ws.get(_lib.lib.arx_sparse_adagrad_workspace_bytes(args.total))
    call("arx_sparse_adagrad_cat_multi", int(phase), args.nt, args.E, args.acc, args.bias,
         args.bias_acc, args.rows, args.cnt, args.d, args.ns, args.site_table, args.cat_map, args.ids,
         args.count, args.row_base, args.coef, _p(G), _ld(G), _p(Gb), _p(lr_dev), _p(gscale_dev),
         _p(keys_buf), _p(src_buf), _p(coef_buf), args.nx, args.extra_n, args.extra_table, wsp, wsn,
         _stream())


def sparse_adagrad_cat_multi_bags(args, G, Gb, lr_dev, keys_buf, src_buf, coef_buf, ws, bag_E, bag_acc,
                                  bag_bias, bag_bias_acc, vals, starts, lens, max_len, bag_ws,
                                  gscale_dev=None, phase=K7_BOTH, bag_aux_cnt=None, csc=None, split=None):
    """arx_sparse_adagrad_cat_multi with a multi-hot table riding on it: the lookups of one-hot
    table 0 are also the lookups of the bags of table bag_E -- an item's id row and its multi-hot
    attribute (HET layout); starts / lens are indexed by the ROW of table 0 (arx.h).  Same phases as
    sparse_adagrad_cat_multi, or the quarters K7_SORT_HOT .. K7_APPLY_TOKENS; `ws` and `bag_ws` must be the same
    objects for all of them."""
    assert args.nx == 0
    n0 = sum(int(args.count[q]) for q in range(args.ns) if int(args.site_table[q]) == 0)
    wsp, wsn = ws.get(_lib.lib.arx_sparse_adagrad_workspace_bytes(args.total))
    bwp, bwn = bag_ws.get(_lib.lib.arx_sparse_adagrad_bags_workspace_bytes(max(n0, 1), int(max_len), args.d))
    # csc: (BagCSC, flags, slot_of) -- the table's static token order (no expansion, no token sort in the step)
    cs, flags, slot_of = csc if csc is not None else (None, None, None)
    # split: this pass's apply form (True `split`, False `win`, None: the process default ARX_K7_RIDER) -- arx.h
    form = 0 if split is None else (K7_FORM_SPLIT if split else K7_FORM_WIN)
    call("arx_sparse_adagrad_cat_multi_bags", int(phase) | form, args.nt, args.E, args.acc, args.bias,
         args.bias_acc, args.rows, args.cnt, args.d, args.ns, args.site_table, args.cat_map, args.ids,
         args.count, args.row_base, args.coef, _p(G), _ld(G), _p(Gb), _p(lr_dev), _p(gscale_dev),
         _p(keys_buf), _p(src_buf), _p(coef_buf), wsp, wsn, _p(bag_E), _p(bag_acc), _p(bag_bias),
         _p(bag_bias_acc), int(bag_E.shape[0]), _p(vals), _p(starts), _p(lens), int(max_len),
         _p(bag_aux_cnt), bwp, bwn, _p(cs.qpos) if cs is not None else None,
         _p(cs.qte) if cs is not None else None, _p(flags), _p(slot_of), cs.nq if cs is not None else 0,
         _stream())


class BagCSC(object):
    """The STATIC token-major order of a multi-hot table's bags (csrc/csc.hip; arx.h,
    arx_sparse_adagrad_cat_multi_bags): built once per (bag index, max_len) on the host from the
    feature CSR of attributes/attribute.py (embed_attribute.py:265-318 uploads it once and never
    changes it).  Pairs are enumerated by (entity, position in bag) and ordered by token with a stable
    sort -- the order the per-step stable radix sort of the expanded bags produced, so the token
    sums keep their bits.  ok == False: a CSR position belongs to two bags (no place of its own)."""

    def __init__(self, vals, starts, lens, max_len, table_rows):
        import numpy as np
        dev = vals.device
        v = vals.detach().cpu().numpy()
        ln = np.clip(lens.detach().cpu().numpy().astype(np.int64), 0, int(max_len))
        n_ent, nv = int(ln.shape[0]), int(v.shape[0])
        st = starts.detach().cpu().numpy().astype(np.int64)[:n_ent]
        tot = int(ln.sum())
        assert nv < (1 << 31) and tot < (1 << 31)
        # every CSR position may belong to ONE bag only (it gets one place): ranges of non-empty bags, in start order,
        # must not overlap and must lie inside vals
        live = np.nonzero(ln > 0)[0]
        o_ = live[np.argsort(st[live], kind='stable')]
        inside = bool(live.size == 0 or (st[o_[0]] >= 0 and st[o_[-1]] + ln[o_[-1]] <= nv))
        self.ok = inside and bool(np.all(st[o_[:-1]] + ln[o_[:-1]] <= st[o_[1:]]))
        self.nq, self.n_ent = 0, n_ent
        if not self.ok:
            self.qpos = self.qte = None
            return
        ent = np.repeat(np.arange(n_ent, dtype=np.int32), ln)
        pos = np.repeat((st - (np.cumsum(ln) - ln)).astype(np.int32), ln) + np.arange(tot, dtype=np.int32)
        tok = v[pos]                                   # CSR position and token of every pair, (entity, position) order
        bad = (tok < 0) | (tok >= int(table_rows))
        if bad.any():                                  # tokens outside the table are dropped (as the step's sort does)
            keep = ~bad
            pos, ent, tok = pos[keep], ent[keep], tok[keep]
        # stable order by token: LSD passes over 16-bit digits (numpy's stable sort is a radix sort for those)
        order = np.argsort((tok & 0xffff).astype(np.uint16), kind='stable')
        if int(table_rows) > (1 << 16):
            order = order[np.argsort((tok[order] >> 16).astype(np.uint16), kind='stable')]
        nq = int(order.shape[0])
        qpos = np.full(max(nv, 1), -1, dtype=np.int32)
        qpos[pos[order]] = np.arange(nq, dtype=np.int32)
        self.nq = nq
        qte = np.empty((max(nq, 1), 2), dtype=np.int32)
        qte[:nq, 0] = tok[order]
        qte[:nq, 1] = ent[order]
        self.qpos = torch.from_numpy(qpos).to(dev)
        self.qte = torch.from_numpy(qte).to(dev)

    def scratch(self):
        """Per-pass device state: the flag bytes (zero between steps) and the entity -> merged-row map."""
        dev = self.qpos.device
        fb = (self.nq + 255) // 256 * 256          # flag bytes + one coarse byte per 16 of them (arx.h)
        return (torch.zeros(fb + fb // 16, dtype=torch.uint8, device=dev),
                torch.zeros(max(self.n_ent, 1), dtype=torch.int32, device=dev))


class BagSiteArgs(object):
    """Host-side descriptor arrays of arx_sparse_adagrad_bags, built once per plan.
    sites: list of (ids, row_base, coef) -- the lookups of one multi-hot table."""

    def __init__(self, sites, max_len):
        import ctypes as C
        n = len(sites)
        self.n = n
        self.total = sum(int(s[0].shape[0]) for s in sites)
        self.max_len = int(max_len)
        self.ids = (C.c_void_p * n)(*[_p(s[0]) for s in sites])
        self.count = (C.c_int64 * n)(*[int(s[0].shape[0]) for s in sites])
        self.row_base = (C.c_int32 * n)(*[int(s[1]) for s in sites])
        self.coef = (C.c_float * n)(*[float(s[2]) for s in sites])
        self._keep = sites


def sparse_adagrad_bags(E, acc, bias, bias_acc, vals, starts, lens, site_args, G, Gb, lr_dev, ws,
                        gscale_dev=None, phase=K7_BOTH, aux_cnt=None):
    """Multi-hot lookups of one table: merge per entity, then per token (arx.h).  phase K7_SORT: both
    sorts (ids only), K7_APPLY: merge + apply, K7_BOTH: both; same `ws` for both halves."""
    d = int(E.shape[1])
    wsp, wsn = ws.get(_lib.lib.arx_sparse_adagrad_bags_workspace_bytes(site_args.total, site_args.max_len, d))
    call("arx_sparse_adagrad_bags", int(phase), _p(E), _p(acc), _p(bias), _p(bias_acc), int(E.shape[0]), d,
         _p(vals), _p(starts), _p(lens), int(lens.shape[0]), site_args.max_len, site_args.n, site_args.ids,
         site_args.count, site_args.row_base, site_args.coef, _p(G), _ld(G), _p(Gb), _p(lr_dev),
         _p(gscale_dev), _p(aux_cnt), wsp, wsn, _stream())


def segment_pool_fwd(scores, offs, W, mode, out, gmax=None):
    call("arx_segment_pool_fwd", _p(scores), _ld(scores), _p(offs), int(scores.shape[0]), int(W), int(mode),
         _p(gmax), _p(out), _ld(out), _stream())


def segment_pool_bwd(scores, offs, W, mode, out, dout, dscores, gmax=None, resid_rows=None):
    call("arx_segment_pool_bwd", _p(scores), _ld(scores), _p(offs), int(scores.shape[0]), int(W),
         int(dscores.shape[1]), int(mode), _p(gmax), _p(out), _ld(out), _p(dout), _ld(dout), _p(dscores),
         _ld(dscores), _p(resid_rows), _stream())


_reduce_scratch = {}


def new_reduce_scratch(device):
    """A zeroed arx_reduce_scratch_bytes() buffer: the caller-owned block partials + arrival ticket of the
    deterministic one-launch reductions (norms, running arg-max).  Launches that may overlap on the GPU need
    different buffers (a Runtime owns one); every call leaves it zeroed."""
    return torch.zeros(int(_lib.lib.arx_reduce_scratch_bytes()), dtype=torch.uint8, device=device)


def _rscratch(x, scratch):
    """scratch given by the caller, else ONE buffer per device (fine for launches on one stream only)."""
    if scratch is not None:
        return _p(scratch)
    s = _reduce_scratch.get(x.device)
    if s is None:
        s = _reduce_scratch[x.device] = new_reduce_scratch(x.device)
    return _p(s)


def max_argmax(x, col_base, first, best, best_idx, scratch=None):
    call("arx_max_argmax", _p(x), int(x.shape[0]), int(x.shape[1]), _ld(x), int(col_base), int(bool(first)),
         _p(best), _p(best_idx), _rscratch(x, scratch), _stream())


def gmax_residual_bwd(resid, idx, U, E_row, row_grad, bias_grad, dU):
    call("arx_gmax_residual_bwd", _p(resid), _p(idx), _p(U), _ld(U), _p(E_row), int(U.shape[1]), _p(row_grad),
         _p(bias_grad), _p(dU), _ld(dU) if dU is not None else 0, _stream())


def gmax_norm_corr(keys, src, coef, n, X, d, per_step, step_stride, Xb, per_step_b, stepb_stride, vrows, RG, RGb, corr):
    """corr[t] = change of a merged table gradient's squared norm from the arg-max residual rows (arx.h)."""
    call("arx_gmax_norm_corr", _p(keys), _p(src), _p(coef), int(n), _p(X), int(X.stride(-2)) if X is not None else 0,
         int(d), int(bool(per_step)), int(step_stride), _p(Xb), int(bool(per_step_b)), int(stepb_stride), _p(vrows),
         _p(RG), int(RG.stride(-2)) if RG is not None else 0, _p(RGb), int(vrows.shape[0]), _p(corr), _stream())


def adagrad_dense(w, acc, g, lr_dev, gscale_dev=None):
    call("arx_adagrad_dense", _p(w), _p(acc), _p(g), int(w.numel()), _p(lr_dev), _p(gscale_dev),
         _stream())


def adagrad_rows_nonzero(W, acc, bias, bias_acc, G, Gb, lr_dev):
    """Adagrad over the rows of W whose dense gradient row in G is not all zero; consumed rows of G / cells of Gb are
    zeroed (arx.h)."""
    call("arx_adagrad_rows_nonzero", _p(W), _p(acc), _p(bias), _p(bias_acc), _p(G), _p(Gb), int(W.shape[0]),
         int(W.shape[1]), _p(lr_dev), _stream())


def adagrad_dense_multi(params, lr_dev, gscale_dev=None):
    """params: [(w, acc|None, g)]: one launch per 8 parameters (arx_adagrad_dense_multi)."""
    import ctypes as C
    for k in range(0, len(params), 8):
        grp = params[k:k + 8]
        m = len(grp)
        ws_ = (C.c_void_p * m)(*[_p(p[0]) for p in grp])
        accs = (C.c_void_p * m)(*[(_p(p[1]) or None) for p in grp])
        gs = (C.c_void_p * m)(*[_p(p[2]) for p in grp])
        ns = (C.c_int64 * m)(*[int(p[0].numel()) for p in grp])
        call("arx_adagrad_dense_multi", m, ws_, accs, gs, ns, _p(lr_dev), _p(gscale_dev), _stream())


def sq_norm_accum(x, out_accum, d=1, row_scale=None, n=None, scratch=None):
    call("arx_sq_norm_accum", _p(x), int(x.numel() if n is None else n), int(d), _p(row_scale),
         _p(out_accum), _rscratch(x, scratch), _stream())


def sq_norm_accum_multi(items, out_accum, scratch=None):
    """items: [(x, d, row_scale|None, n|None)]: out += sum over all of them, <= 8 per launch."""
    import ctypes as C
    for k in range(0, len(items), 8):
        grp = items[k:k + 8]
        m = len(grp)
        xs = (C.c_void_p * m)(*[_p(g[0]) for g in grp])
        ns = (C.c_int64 * m)(*[int(g[0].numel() if g[3] is None else g[3]) for g in grp])
        ds = (C.c_int * m)(*[int(g[1]) for g in grp])
        rs = (C.c_void_p * m)(*[(_p(g[2]) or None) for g in grp])
        call("arx_sq_norm_accum_multi", m, xs, ns, ds, rs, _p(out_accum), _rscratch(out_accum, scratch), _stream())


def sq_norm_clip_multi(items, sqnorm, max_norm, coef_out, gnorm_out=None, init=True, scratch=None):
    """sq_norm_accum_multi + clip_coef in as few launches as tensors / 8: the LAST launch also forms
    coef = max_norm / max(||g||, max_norm) (arx_sq_norm_clip_multi); init: sqnorm is overwritten by the
    first launch instead of accumulated onto (no fill launch)."""
    import ctypes as C
    groups = [items[k:k + 8] for k in range(0, len(items), 8)]
    if not groups:
        if init:
            fill_f32(sqnorm, 0.0)
        clip_coef(sqnorm, max_norm, coef_out, gnorm_out)
        return
    for gi, grp in enumerate(groups):
        m = len(grp)
        xs = (C.c_void_p * m)(*[_p(g[0]) for g in grp])
        ns = (C.c_int64 * m)(*[int(g[0].numel() if g[3] is None else g[3]) for g in grp])
        ds = (C.c_int * m)(*[int(g[1]) for g in grp])
        rs = (C.c_void_p * m)(*[(_p(g[2]) or None) for g in grp])
        first, last = gi == 0, gi == len(groups) - 1
        if last:
            call("arx_sq_norm_clip_multi", m, xs, ns, ds, rs, int(bool(init and first)), _p(sqnorm), float(max_norm),
                 _p(coef_out), _p(gnorm_out), _rscratch(sqnorm, scratch), _stream())
        elif init and first:
            fill_f32(sqnorm, 0.0)
            call("arx_sq_norm_accum_multi", m, xs, ns, ds, rs, _p(sqnorm), _rscratch(sqnorm, scratch), _stream())
        else:
            call("arx_sq_norm_accum_multi", m, xs, ns, ds, rs, _p(sqnorm), _rscratch(sqnorm, scratch), _stream())


def merged_sq_norm(keys, src, coef, table_rows, out_accum, ws, X=None, d=0, L=1, step_stride=0,
                   Xb=None, Lb=1, stepb_stride=0, n=None, scratch=None):
    """out += sum_t sum_rows ||sum_{c -> row} coef_c X_t[src_c]||^2 (+ the d = 1 analogue on Xb):
    the norm of a table gradient after merging contributions per table row."""
    n = int(keys.shape[0]) if n is None else int(n)
    wsp, wsn = ws.get(_lib.lib.arx_sparse_adagrad_workspace_bytes(n))
    call("arx_merged_sq_norm", _p(keys), _p(src), _p(coef), n, key_bits_for(table_rows),
         _p(X), int(X.stride(-2)) if X is not None else 0, int(d), int(L), int(step_stride),
         _p(Xb), int(Lb), int(stepb_stride), _p(out_accum), wsp, wsn, _rscratch(out_accum, scratch), _stream())


def clip_coef(sqnorm, max_norm, coef_out, gnorm_out=None):
    call("arx_clip_coef", _p(sqnorm), float(max_norm), _p(coef_out), _p(gnorm_out), _stream())


# ---- utilities -------------------------------------------------------------------------
def fill_f32(t, v):
    call("arx_fill_f32", _p(t), int(t.numel()), float(v), _stream())


def fill_i32(t, v):
    call("arx_fill_i32", _p(t), int(t.numel()), int(v), _stream())


def fill_u8(t, v):
    call("arx_fill_u8", _p(t), int(t.numel()), int(v), _stream())


def axpby(a, x, b, y, n=None):
    call("arx_axpby", float(a), _p(x), float(b), _p(y), int(y.numel() if n is None else n), _stream())


def add_rows_bcast(a, x, b, y):
    call("arx_add_rows_bcast", float(a), _p(x), _ld(x), int(x.shape[0]), float(b), _p(y), _ld(y),
         int(y.shape[0]), int(y.shape[1]), _stream())


def row_sum(x, out, accumulate=False):
    call("arx_row_sum", _p(x), _ld(x), int(x.shape[0]), int(x.shape[1]), _p(out),
         int(bool(accumulate)), _stream())


def col_sum(x, out, ws):
    rows, cols = int(x.shape[0]), int(x.shape[1])
    wsp, wsn = ws.get(_lib.lib.arx_col_sum_workspace_bytes(rows, cols))
    call("arx_col_sum", _p(x), _ld(x), rows, cols, _p(out), wsp, wsn, _stream())


def sum_scaled(x, scale, out, n=None):
    call("arx_sum_scaled", _p(x), int(x.numel() if n is None else n), float(scale), _p(out), _stream())


def dropout_fwd(x, keep_prob, seed, y, keep_mask):
    call("arx_dropout_fwd", _p(x), int(x.numel()), float(keep_prob), int(seed), _p(y),
         _p(keep_mask), _stream())


def dropout_fwd_step(x, keep_prob, seed, step_dev, y, keep_mask):
    """dropout whose seed also takes a device-side step counter (int64 tensor [1])."""
    call("arx_dropout_fwd_step", _p(x), int(x.numel()), float(keep_prob), int(seed) & (2 ** 64 - 1),
         _p(step_dev), _p(y), _p(keep_mask), _stream())


def merge_keyed_take(keys, ids, S, out):
    """out[r] = id of the r-th smallest (key, position) pair, r < S (arx.h): the merge of sorted race lists.
    keys: float32 >= 0 (race keys: the kernel orders their bit patterns), ids / out: int32."""
    if keys.dtype != torch.float32 or ids.dtype != torch.int32 or out.dtype != torch.int32:
        raise TypeError("merge_keyed_take: keys float32, ids / out int32 expected (got %s, %s, %s)"
                        % (keys.dtype, ids.dtype, out.dtype))
    if ids.shape[0] != keys.shape[0] or out.shape[0] < int(S):
        raise ValueError("merge_keyed_take: ids must match keys, out must hold S entries")
    call("arx_merge_keyed_take", _p(keys), _p(ids), int(keys.shape[0]), int(S), _p(out), _stream())


def take_i32(table, idx, out, fill=-1):
    call("arx_take_i32", _p(table), _p(idx), int(idx.shape[0]), int(fill), _p(out), _stream())


def copy_words(pairs):
    """[(src, dst), ...] device tensors of 4-byte elements, equal sizes per pair; <= 8 per launch."""
    import ctypes as C
    for k in range(0, len(pairs), 8):
        grp = pairs[k:k + 8]
        n = len(grp)
        src, dst, cnt = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int64 * n)()
        for a, (s_, d_) in enumerate(grp):
            if s_.element_size() != 4 or d_.element_size() != 4 or s_.numel() != d_.numel():
                raise ValueError("copy_words: 4-byte tensors of equal size expected")
            src[a], dst[a], cnt[a] = s_.data_ptr(), d_.data_ptr(), s_.numel()
        call("arx_copy_words", n, src, dst, cnt, _stream())


def counter_add(counter_dev, v=1):
    call("arx_counter_add", _p(counter_dev), int(v), _stream())


def dropout_bwd(dy, keep_mask, keep_prob, dx):
    call("arx_dropout_bwd", _p(dy), _p(keep_mask), int(dy.numel()), float(keep_prob), _p(dx), _stream())


def act_fwd(x, kind, y):
    call("arx_act_fwd", _p(x), int(x.numel()), int(kind), _p(y), _stream())


def act_bwd(y, dy, kind, dx):
    call("arx_act_bwd", _p(y), _p(dy), int(y.numel()), int(kind), _p(dx), _stream())


def topk_chunk(logits, k, idx_base, values, indices):
    call("arx_topk_chunk", _p(logits), _ld(logits), int(logits.shape[0]), int(logits.shape[1]), int(k),
         int(idx_base), _p(values), _p(indices), _stream())


def topk_merge(va, ia, vb, ib, k, vo, io):
    call("arx_topk_merge", _p(va), _p(ia), _p(vb), _p(ib), int(va.shape[0]), int(va.shape[1]),
         int(vb.shape[1]), int(k), _p(vo), _p(io), _stream())


def gemm_nt_topk_parts(M, N):
    """Column ranges arx_gemm_nt_topk_filter splits N columns into for M rows (sizes the candidate rows)."""
    import ctypes as C
    n = C.c_int(0)
    call("arx_gemm_nt_topk_parts", int(M), int(N), C.byref(n))
    return int(n.value)


def gemm_nt_topk_filter(A, Bm, col_bias, thr, col_base, cand_v, cand_i, capp, overflow, lse_part=None):
    """Scorer GEMM A . Bm^T + col_bias that keeps only the logits above thr[row]; lse_part [M, >= parts]: also the
    per-column-range log-sum-exp of every row (arx.h)."""
    call("arx_gemm_nt_topk_filter", _p(A), _ld(A), int(A.shape[0]), _p(Bm), _ld(Bm), int(Bm.shape[0]), int(A.shape[1]),
         _p(col_bias), _p(thr), int(thr.stride(0)), int(col_base), _p(cand_v), _p(cand_i), int(cand_v.stride(0)),
         int(capp), _p(overflow), _p(lse_part), int(lse_part.stride(0)) if lse_part is not None else 0, _stream())


def gemm_nt_topk_filter_excl(A, Bm, col_bias, thr, col_base, cand_v, cand_i, capp, overflow, ex, lse_part=None):
    """gemm_nt_topk_filter whose candidates skip each row's excluded columns (arx.h).  ex: (row_keys, key_rows,
    ex_ptr, ex_cols) -- row r's list is ex_cols[ex_ptr[key] .. ex_ptr[key + 1]), key = row_keys[r % key_rows]."""
    keys, key_rows, ptr, cols = ex
    call("arx_gemm_nt_topk_filter_excl", _p(A), _ld(A), int(A.shape[0]), _p(Bm), _ld(Bm), int(Bm.shape[0]),
         int(A.shape[1]), _p(col_bias), _p(thr), int(thr.stride(0)), int(col_base), _p(cand_v), _p(cand_i),
         int(cand_v.stride(0)), int(capp), _p(overflow), _p(lse_part),
         int(lse_part.stride(0)) if lse_part is not None else 0, _p(keys), int(key_rows), _p(ptr), _p(cols), _stream())


def topk_exclude_fill(logits, col0, ex):
    """logits[r, c - col0] = -inf for row r's excluded columns c in [col0, col0 + logits.shape[1]) (arx.h)."""
    if logits.numel() == 0:
        return
    keys, key_rows, ptr, cols = ex
    call("arx_topk_exclude_fill", _p(logits), _ld(logits), int(logits.shape[0]), int(col0), int(logits.shape[1]),
         _p(keys), int(key_rows), _p(ptr), _p(cols), _stream())


def topk_tags_fill(logits, col0, tags):
    """logits[r, c - col0] = -inf where column c in [col0, col0 + logits.shape[1]) is ineligible for row r (arx_tags.h).
    tags: (col_tags [V] int32 bit patterns by ABSOLUTE column, want_any, want_all, want_rows) -- row r's two words
    are want_*[r % want_rows]."""
    if logits.numel() == 0:
        return
    col_tags, want_any, want_all, want_rows = tags
    if int(col0) + int(logits.shape[1]) > int(col_tags.shape[0]):
        raise ValueError("topk_tags_fill: columns [%d, %d) past the %d tag words"
                         % (col0, int(col0) + int(logits.shape[1]), int(col_tags.shape[0])))
    call("arx_topk_tags_fill", _p(logits), _ld(logits), int(logits.shape[0]), int(col0), int(logits.shape[1]),
         _p(col_tags), _p(want_any), _p(want_all), int(want_rows), _stream())


def gemm_nt_topk_filter_tags(A, Bm, col_bias, thr, col_base, cand_v, cand_i, capp, overflow, tags, ex=None,
                             lse_part=None):
    """gemm_nt_topk_filter_excl whose candidates also skip the columns ineligible by their tag words (arx_tags.h).  tags:
    (col_tags, want_any, want_all, want_rows) with col_tags ALREADY sliced to this launch's columns (like col_bias);
    ex: exclusion lists or None."""
    col_tags, want_any, want_all, want_rows = tags
    if int(col_tags.shape[0]) < int(Bm.shape[0]):
        raise ValueError("gemm_nt_topk_filter_tags: %d tag words for %d columns"
                         % (int(col_tags.shape[0]), int(Bm.shape[0])))
    keys, key_rows, ptr, cols = ex if ex is not None else (None, 0, None, None)
    call("arx_gemm_nt_topk_filter_tags", _p(A), _ld(A), int(A.shape[0]), _p(Bm), _ld(Bm), int(Bm.shape[0]),
         int(A.shape[1]), _p(col_bias), _p(thr), int(thr.stride(0)), int(col_base), _p(cand_v), _p(cand_i),
         int(cand_v.stride(0)), int(capp), _p(overflow), _p(lse_part),
         int(lse_part.stride(0)) if lse_part is not None else 0, _p(keys), int(key_rows), _p(ptr), _p(cols),
         _p(col_tags), _p(want_any), _p(want_all), int(want_rows), _stream())


def rows_bf16_norm(P, img, norms):
    """img [N, K] bfloat16 = the round-to-nearest-even bf16 of P [N, K] float32, norms [N] = each row's 2-norm rounded
    UP (arx_topk_bf16.h) -- the image and the column norms gemm_nt_topk_filter_bf16 scans."""
    _chk(P, torch.float32, 'P')
    _chk(img, torch.bfloat16, 'img')
    _chk(norms, torch.float32, 'norms')
    if P.dim() != 2 or tuple(img.shape) != tuple(P.shape) or norms.dim() != 1 or int(norms.shape[0]) != int(P.shape[0]) \
            or not norms.is_contiguous():
        raise ValueError("rows_bf16_norm: P [N, K], img [N, K] and a contiguous norms [N], got %s, %s, %s"
                         % (tuple(P.shape), tuple(img.shape), tuple(norms.shape)))
    call("arx_rows_bf16_norm", _p(P), _ld(P), int(P.shape[0]), int(P.shape[1]), _p(img), _ld(img), _p(norms), _stream())


def gemm_nt_topk_filter_bf16(A, Bimg, coln, col_bias, thr, col_base, cand_v, cand_i, capp, overflow, coeff, tags=None,
                             ex=None):
    """gemm_nt_topk_filter_tags on the bf16 matrix pipe (arx_topk_bf16.h): Bimg [N, K] bfloat16 and coln [N] come from
    rows_bf16_norm, a logit passes when fmaf(coeff * |A[r]|, coln[c], v~) > thr[r]; cand_v receives the APPROXIMATE v~
    (cand_rescore overwrites it).  coeff: a float32 >= topk.bf16_margin_coeff(K).  tags: (col_tags, want_any, want_all,
    want_rows) with col_tags ALREADY sliced to this launch's columns, or None; ex: exclusion lists or None."""
    _chk(Bimg, torch.bfloat16, 'Bimg')
    _chk(coln, torch.float32, 'coln')
    if int(coln.shape[0]) < int(Bimg.shape[0]):
        raise ValueError("gemm_nt_topk_filter_bf16: %d column norms for %d columns"
                         % (int(coln.shape[0]), int(Bimg.shape[0])))
    col_tags, want_any, want_all, want_rows = tags if tags is not None else (None, None, None, 0)
    if col_tags is not None and int(col_tags.shape[0]) < int(Bimg.shape[0]):
        raise ValueError("gemm_nt_topk_filter_bf16: %d tag words for %d columns"
                         % (int(col_tags.shape[0]), int(Bimg.shape[0])))
    keys, key_rows, ptr, cols = ex if ex is not None else (None, 0, None, None)
    call("arx_gemm_nt_topk_filter_bf16", _p(A), _ld(A), int(A.shape[0]), _p(Bimg), _ld(Bimg), _p(coln),
         int(Bimg.shape[0]), int(A.shape[1]), float(coeff), _p(col_bias), _p(thr), int(thr.stride(0)), int(col_base),
         _p(cand_v), _p(cand_i), int(cand_v.stride(0)), int(capp), _p(overflow), _p(keys), int(key_rows), _p(ptr),
         _p(cols), _p(col_tags), _p(want_any), _p(want_all), int(want_rows), _stream())


def cand_rescore(U, P, pbias, cand_v, cand_i):
    """cand_v[r, j] = U[r] . P[cand_i[r, j]] + pbias[cand_i[r, j]] in slate_scores' arithmetic for every occupied slot
    (cand_v != -inf) of the candidate rows, in place (arx_topk_bf16.h); P: the WHOLE pool."""
    _chk(cand_v, torch.float32, 'cand_v')
    _chk(cand_i, torch.int32, 'cand_i')
    if cand_v.dim() != 2 or tuple(cand_i.shape) != tuple(cand_v.shape) or cand_i.stride(0) != cand_v.stride(0):
        raise ValueError("cand_rescore: cand_v and cand_i are [B, ncand] of one row stride")
    call("arx_cand_rescore", _p(U), _ld(U), int(U.shape[0]), _p(P), _ld(P), _p(pbias), int(P.shape[0]),
         int(U.shape[1]), _p(cand_v), _p(cand_i), int(cand_v.stride(0)), int(cand_v.shape[1]), _stream())


def sample_keyed(sample):
    """A sample tuple's noise key: (tau, tau_rows, seed_words) is the plain convention of arx_sample.h -- None; three
    more entries (col_mul, col_add, noise_rows int32 [tau_rows] or None) are the keyed one of arx_sample_shard.h --
    noise column = column * col_mul + col_add, noise row = noise_rows[r % tau_rows]."""
    if len(sample) == 3:
        return None
    col_mul, col_add, noise_rows = sample[3:]
    _chk(noise_rows, torch.int32, 'noise_rows')
    if noise_rows is not None and (noise_rows.dim() != 1 or not noise_rows.is_contiguous()
                                   or int(noise_rows.shape[0]) < int(sample[1])):
        raise ValueError("sample: noise_rows is a contiguous int32 [tau_rows]")
    return int(col_mul), int(col_add), noise_rows


def sample_rekeyed(sample, col_mul, col_add):
    """The sample tuple with another column map and the same noise rows (None where the tuple has none)."""
    return tuple(sample[:3]) + (int(col_mul), int(col_add), sample[5] if len(sample) > 3 else None)


def topk_gumbel_add(logits, col0, sample):
    """logits[r, c] = fmaf(tau[r % tau_rows], g(noise row, noise column of col0 + c), logits[r, c]) in place: the
    logits become the keys of the sampled recommend (arx_sample.h).  sample: (tau float32 [tau_rows], tau_rows,
    seed_words int32 [2]) -- noise row r % tau_rows, noise column col0 + c -- or the keyed six (sample_keyed)."""
    if logits.numel() == 0:
        return
    tau, tau_rows, seed_words = sample[:3]
    key = sample_keyed(sample)
    if key is None:
        call("arx_topk_gumbel_add", _p(logits), _ld(logits), int(logits.shape[0]), int(col0), int(logits.shape[1]),
             _p(tau), int(tau_rows), _p(seed_words), _stream())
        return
    call("arx_topk_gumbel_add_keyed", _p(logits), _ld(logits), int(logits.shape[0]), int(col0), int(logits.shape[1]),
         _p(tau), int(tau_rows), _p(seed_words), key[0], key[1], _p(key[2]), _stream())


def topk_gumbel_strip(values, indices, sample):
    """values = fmaf(-tau, g(r % tau_rows, index), key): the winners' keys back into scores; -inf at index -1
    (arx_sample.h)."""
    tau, tau_rows, seed_words = sample[:3]
    key = sample_keyed(sample)
    if key is None:
        call("arx_topk_gumbel_strip", _p(values), _ld(values), _p(indices), _ld(indices), int(values.shape[0]),
             int(values.shape[1]), _p(tau), int(tau_rows), _p(seed_words), _stream())
        return
    call("arx_topk_gumbel_strip_keyed", _p(values), _ld(values), _p(indices), _ld(indices), int(values.shape[0]),
         int(values.shape[1]), _p(tau), int(tau_rows), _p(seed_words), key[0], key[1], _p(key[2]), _stream())


def gemm_nt_topk_filter_sample(A, Bm, col_bias, thr, col_base, cand_v, cand_i, capp, overflow, sample, tags=None,
                               ex=None, lse_part=None):
    """gemm_nt_topk_filter_tags on the KEYS fmaf(tau, g, logit): thr and cand_v are keys, lse_part stays over the
    logits (arx_sample.h).  sample: (tau, tau_rows, seed_words); tags: (col_tags ALREADY sliced to this launch's
    columns, want_any, want_all, want_rows) or None; ex: exclusion lists or None."""
    tau, tau_rows, seed_words = sample[:3]
    key = sample_keyed(sample)
    col_tags, want_any, want_all, want_rows = tags if tags is not None else (None, None, None, 0)
    if tags is not None and int(col_tags.shape[0]) < int(Bm.shape[0]):
        raise ValueError("gemm_nt_topk_filter_sample: %d tag words for %d columns"
                         % (int(col_tags.shape[0]), int(Bm.shape[0])))
    keys, key_rows, ptr, cols = ex if ex is not None else (None, 0, None, None)
    args = (_p(A), _ld(A), int(A.shape[0]), _p(Bm), _ld(Bm), int(Bm.shape[0]),
            int(A.shape[1]), _p(col_bias), _p(thr), int(thr.stride(0)), int(col_base), _p(cand_v), _p(cand_i),
            int(cand_v.stride(0)), int(capp), _p(overflow), _p(lse_part),
            int(lse_part.stride(0)) if lse_part is not None else 0, _p(keys), int(key_rows), _p(ptr), _p(cols),
            _p(col_tags), _p(want_any), _p(want_all), int(want_rows), _p(tau), int(tau_rows), _p(seed_words))
    if key is None:
        call("arx_gemm_nt_topk_filter_sample", *(args + (_stream(),)))
    else:
        call("arx_gemm_nt_topk_filter_sample_keyed", *(args + (key[0], key[1], _p(key[2]), _stream())))


def topk_mark_empty(values, indices):
    """indices = -1 where values == -inf (a row with fewer eligible columns than k)."""
    call("arx_topk_mark_empty", _p(values), _ld(values), _p(indices), _ld(indices), int(values.shape[0]),
         int(values.shape[1]), _stream())


def rows_inv_norm(E, out):
    """out[i] = 1 / |E[i]| (0 for a zero row) of the rows of a 2-D fp32 view (arx.h)."""
    _chk(E, torch.float32, 'E'); _chk(out, torch.float32, 'out')
    if E.dim() != 2 or out.dim() != 1 or int(out.shape[0]) < int(E.shape[0]):
        raise ValueError("rows_inv_norm: E [n, d], out [>= n]")
    if E.shape[0] == 0:
        return
    call("arx_rows_inv_norm", _p(E), _ld(E), int(E.shape[0]), int(E.shape[1]), _p(out), _stream())


def gather_rows_unit(E, rows, out):
    """out[r] = E[rows[r]] / |E[rows[r]]| (a zero row for rows[r] < 0 and for a zero row of E) (arx.h).  The caller
    keeps rows[r] below E.shape[0]."""
    _chk(E, torch.float32, 'E'); _chk(rows, torch.int32, 'rows'); _chk(out, torch.float32, 'out')
    B = int(rows.shape[0])
    if E.dim() != 2 or out.dim() != 2 or int(out.shape[0]) < B or int(out.shape[1]) != int(E.shape[1]):
        raise ValueError("gather_rows_unit: E [n, d], rows [B], out [>= B, d]")
    if B == 0:
        return
    call("arx_gather_rows_unit", _p(E), _ld(E), _p(rows), B, int(E.shape[1]), _p(out), _ld(out), _stream())


def cos_chunk_finish(logits, col0, col_scale, self_col=None):
    """logits[r, c] *= col_scale[col0 + c], then -inf at each row's own column self_col[r] - col0 (arx.h)."""
    _chk(logits, torch.float32, 'logits'); _chk(col_scale, torch.float32, 'col_scale')
    _chk(self_col, torch.int32, 'self_col')
    B, n = int(logits.shape[0]), int(logits.shape[1])
    if int(col_scale.shape[0]) < int(col0) + n or (self_col is not None and int(self_col.shape[0]) < B):
        raise ValueError("cos_chunk_finish: col_scale needs col0 + ncols entries, self_col one per row")
    if B == 0 or n == 0:
        return
    call("arx_cos_chunk_finish", _p(logits), _ld(logits), B, int(col0), n, _p(col_scale), _p(self_col), _stream())


def gemm_nt_topk_filter_cos(A, Bm, col_scale, self_col, thr, col_base, cand_v, cand_i, capp, overflow):
    """gemm_nt_topk_filter with v = (A . Bm^T) * col_scale[col] and no bias; self_col [M] int32 (or None): the
    absolute column col_base + col each row drops (arx.h)."""
    _chk(col_scale, torch.float32, 'col_scale'); _chk(self_col, torch.int32, 'self_col')
    if int(col_scale.shape[0]) < int(Bm.shape[0]) or (self_col is not None and
                                                      int(self_col.shape[0]) < int(A.shape[0])):
        raise ValueError("gemm_nt_topk_filter_cos: col_scale needs an entry per row of Bm, self_col one per row of A")
    call("arx_gemm_nt_topk_filter_cos", _p(A), _ld(A), int(A.shape[0]), _p(Bm), _ld(Bm), int(Bm.shape[0]),
         int(A.shape[1]), _p(col_scale), _p(self_col), _p(thr), int(thr.stride(0)), int(col_base), _p(cand_v),
         _p(cand_i), int(cand_v.stride(0)), int(capp), _p(overflow), _stream())


def topk_merge_shards(v, c, vo, io):
    """W-way merge of per-shard top-k lists into global ids (arx.h): v / c [W, B, k] (shard s's lists in block s,
    local columns, -1 = empty) -> vo / io [B, k], id = c * W + s, order (value desc, id asc); -inf / empty -> -1."""
    W, B, k = (int(x) for x in v.shape)
    for t in (v, c, vo, io):
        if not t.is_contiguous():
            raise ValueError("topk_merge_shards: contiguous tensors only")
    if tuple(c.shape) != (W, B, k) or tuple(vo.shape) != (B, k) or tuple(io.shape) != (B, k):
        raise ValueError("topk_merge_shards: v / c [W, B, k], vo / io [B, k]")
    call("arx_topk_merge_shards", _p(v), _p(c), B, W, k, _p(vo), _p(io), _stream())


def topk_softmax_merge_shards(v, id, lse_part, po, io, lse_out=None):
    """W-way merge of per-shard top-k lists of GLOBAL logit ids into softmax winners (arx.h): v / id [W, B, k] (shard
    s's lists in block s, -1 = empty), lse_part [W, B] (each shard's log-sum-exp over all its columns, -inf: none) ->
    io [B, k] by (value desc, id asc), po [B, k] = exp(value - lse) (0 where io is -1), lse_out [B] (optional)."""
    W, B, k = (int(x) for x in v.shape)
    for t in (v, id, lse_part, po, io, lse_out):
        if t is not None and not t.is_contiguous():
            raise ValueError("topk_softmax_merge_shards: contiguous tensors only")
    if v.dtype != torch.float32 or id.dtype != torch.int32 or lse_part.dtype != torch.float32 or \
            po.dtype != torch.float32 or io.dtype != torch.int32 or \
            (lse_out is not None and lse_out.dtype != torch.float32):
        raise ValueError("topk_softmax_merge_shards: v / lse_part / po / lse_out float32, id / io int32")
    if tuple(id.shape) != (W, B, k) or tuple(lse_part.shape) != (W, B) or tuple(po.shape) != (B, k) or \
            tuple(io.shape) != (B, k) or (lse_out is not None and tuple(lse_out.shape) != (B,)):
        raise ValueError("topk_softmax_merge_shards: v / id [W, B, k], lse_part [W, B], po / io [B, k], lse_out [B]")
    if B == 0:
        return                              # (empty tensors have no pointer to pass)
    call("arx_topk_softmax_merge_shards", _p(v), _p(id), _p(lse_part), B, W, k, _p(po), _p(io), _p(lse_out), _stream())


def gemm_nt_eval_parts(A, Bm, col_bias, tscore, lse_part, relu_part):
    """Full-vocabulary evaluation sums out of the scorer GEMM, no logits (arx.h)."""
    ref = lse_part if lse_part is not None else relu_part
    call("arx_gemm_nt_eval_parts", _p(A), _ld(A), int(A.shape[0]), _p(Bm), _ld(Bm), int(Bm.shape[0]), int(A.shape[1]),
         _p(col_bias), _p(tscore), _p(lse_part), _p(relu_part), int(ref.stride(0)), _stream())


def gemm_nt_eval_rank_parts(A, Bm, col_bias, tscore, tcol, relu_part, cnt_part):
    """warp_eval's margin sums and counts of x > t out of the scorer GEMM, no logits (arx.h): relu_part / cnt_part
    [M, >= gemm_nt_topk_parts(M, N)] with one row stride; tcol [M] int32: each row's target column (counted as (1, 0)),
    or a value outside [0, N)."""
    if relu_part.dtype != torch.float32 or cnt_part.dtype != torch.int32 or tcol.dtype != torch.int32:
        raise ValueError("gemm_nt_eval_rank_parts: relu_part float32, cnt_part / tcol int32")
    if relu_part.stride(0) != cnt_part.stride(0) or tuple(relu_part.shape) != tuple(cnt_part.shape):
        raise ValueError("gemm_nt_eval_rank_parts: relu_part and cnt_part need one shape and row stride")
    if int(relu_part.shape[0]) < int(A.shape[0]) or int(tcol.shape[0]) < int(A.shape[0]):
        raise ValueError("gemm_nt_eval_rank_parts: relu_part / cnt_part / tcol need a row per row of A")
    call("arx_gemm_nt_eval_rank_parts", _p(A), _ld(A), int(A.shape[0]), _p(Bm), _ld(Bm), int(Bm.shape[0]),
         int(A.shape[1]), _p(col_bias), _p(tscore), _p(tcol), _p(relu_part), _p(cnt_part), int(relu_part.stride(0)),
         _stream())


EVAL_MODES = {'ce': 0, 'warp': 1, 'warp_eval': 2}


def eval_shard_reduce(mode, parts, cnt_parts, U, E, bias, tscore, tcol, ex, out, cnt_out):
    """One shard's evaluation partial per row (arx.h arx_eval_shard_reduce): parts [B, npart] (None: a shard without
    columns), cnt_parts likewise int32 ('warp_eval'); masks ex = (row_keys, key_rows, ex_ptr, ex_cols of local columns)
    or None, columns recomputed from U [B, d] and E [V, d] (+ bias).  out [B] float32, cnt_out [B] int32."""
    m = EVAL_MODES[mode] if isinstance(mode, str) else int(mode)
    B = int(out.shape[0])
    if tuple(U.shape[:1]) != (B,) or (parts is not None and int(parts.shape[0]) != B):
        raise ValueError("eval_shard_reduce: U, parts and out need one row per row")
    if (cnt_out is not None and tuple(cnt_out.shape) != (B,)) or \
            (cnt_parts is not None and tuple(cnt_parts.shape) != tuple(parts.shape)):
        raise ValueError("eval_shard_reduce: cnt_out [B], cnt_parts shaped as parts")
    keys, key_rows, ptr, cols = ex if ex is not None else (None, 0, None, None)
    call("arx_eval_shard_reduce", m, _p(parts), int(parts.stride(0)) if parts is not None else 0,
         int(parts.shape[1]) if parts is not None else 0, _p(cnt_parts),
         int(cnt_parts.stride(0)) if cnt_parts is not None else 0, _p(U), _ld(U), _p(E), _ld(E), _p(bias),
         int(U.shape[1]), int(E.shape[0]), _p(tscore), _p(tcol), _p(keys), int(key_rows), _p(ptr), _p(cols), B,
         _p(out), _p(cnt_out), _stream())


def eval_merge_shards(mode, parts, cnts, tscore, out, cnt_out):
    """[W, B] per-shard evaluation partials (shard order) -> the loss of each row (arx.h arx_eval_merge_shards):
    ce logsumexp_w - t, warp log1p(sum_w), warp_eval the margin sum and (cnt_out) the count sum."""
    m = EVAL_MODES[mode] if isinstance(mode, str) else int(mode)
    W, B = (int(x) for x in parts.shape)
    for t in (parts, cnts, tscore, out, cnt_out):
        if t is not None and not t.is_contiguous():
            raise ValueError("eval_merge_shards: contiguous tensors only")
    if tuple(out.shape) != (B,) or (cnts is not None and tuple(cnts.shape) != (W, B)) or \
            (cnt_out is not None and tuple(cnt_out.shape) != (B,)) or (tscore is not None and int(tscore.shape[0]) < B):
        raise ValueError("eval_merge_shards: parts / cnts [W, B], tscore / out / cnt_out [B]")
    call("arx_eval_merge_shards", m, _p(parts), _p(cnts), _p(tscore), B, W, _p(out), _p(cnt_out), _stream())


def take_rows_i32(table, pos, out):
    call("arx_take_rows_i32", _p(table), int(table.stride(0)), _p(pos), int(pos.stride(0)), int(pos.shape[0]),
         int(pos.shape[1]), _p(out), int(out.stride(0)), _stream())


def topk(logits, k, values, indices):
    call("arx_topk", _p(logits), _ld(logits), int(logits.shape[0]), int(logits.shape[1]), int(k),
         _p(values), _p(indices), _stream())


def slate_scores(U, P, pbias, cand, scores):
    """scores[r, j] = U[r] . P[cand[r, j]] + pbias[cand[r, j]] where 0 <= cand[r, j] < P.shape[0], else -inf and
    nothing read (arx_slate.h).  U [B, d], P [V, d], pbias [V] or None, cand [B, C] int32, scores [B, C]; 2-D
    arguments may be strided views."""
    _chk(U, torch.float32, 'U'); _chk(P, torch.float32, 'P'); _chk(pbias, torch.float32, 'pbias')
    _chk(cand, torch.int32, 'cand'); _chk(scores, torch.float32, 'scores')
    if U.dim() != 2 or P.dim() != 2 or cand.dim() != 2 or scores.dim() != 2 or U.shape[1] != P.shape[1] \
            or cand.shape[0] != U.shape[0] or tuple(scores.shape) != tuple(cand.shape):
        raise ValueError("slate_scores: U [B, d], P [V, d], cand and scores [B, C]")
    if pbias is not None and (pbias.dim() != 1 or int(pbias.shape[0]) < int(P.shape[0])):
        raise ValueError("slate_scores: pbias needs one entry per pool row")
    if cand.numel() == 0:
        return
    call("arx_slate_scores", _p(U), _ld(U), int(U.shape[0]), _p(P), _ld(P), _p(pbias), int(P.shape[0]),
         int(U.shape[1]), _p(cand), _ld(cand), int(cand.shape[1]), _p(scores), _ld(scores), _stream())


def slate_merge_shards(parts, out):
    """out[r, j] = max over s of parts[s, r, j] (arx_slate.h): parts [W, B, C] contiguous, every live slot owned by
    one shard and -inf in the others; out [B, C] may be a strided view."""
    _chk(parts, torch.float32, 'parts'); _chk(out, torch.float32, 'out')
    if parts.dim() != 3 or not parts.is_contiguous() or out.dim() != 2 or tuple(out.shape) != tuple(parts.shape[1:]):
        raise ValueError("slate_merge_shards: parts [W, B, C] contiguous, out [B, C]")
    if out.numel() == 0:
        return
    call("arx_slate_merge_shards", _p(parts), int(parts.shape[1]), int(parts.shape[2]), int(parts.shape[0]), _p(out),
         _ld(out), _stream())


EXPLAIN_MAX_FEATS, EXPLAIN_MAX_TOP = 8, 16


class ExplainSet(object):
    """Feature descriptors of arx_explain_slate (arx_explain.h) as host arrays, built once per plan.  feats: objects
    with .kind ('cat' | 'mulhot'), .table (.E [rows, d], .bias [rows] or None) and .maps -- (cat_map | None,) or (vals,
    starts, lens), indexed by logit column: graph.Feature, the entries of EntityEmbed.feats.  V: the logit columns;
    every map must hold that many entries.  with_bias False: the biases of the tables are left out (b_f = 0)."""

    def __init__(self, feats, V, with_bias=True):
        import ctypes as C
        n = len(feats)
        if not 1 <= n <= EXPLAIN_MAX_FEATS:
            raise ValueError("explain_slate: 1 .. %d features, got %d" % (EXPLAIN_MAX_FEATS, n))
        self.n, self.V, self.d = n, int(V), int(feats[0].table.E.shape[1])
        for f in feats:
            if f.kind not in ('cat', 'mulhot'):
                raise ValueError("explain_slate: feature kind %r" % (f.kind,))
            _chk(f.table.E, torch.float32, 'E'); _chk(f.table.bias, torch.float32, 'bias')
            if f.table.E.dim() != 2 or int(f.table.E.shape[1]) != self.d:
                raise ValueError("explain_slate: tables of equal width [rows, d]")
            for m in (f.maps[:1] if f.kind == 'cat' else f.maps):
                _chk(m, torch.int32, 'map')
            for m in (f.maps[:1] if f.kind == 'cat' else f.maps[1:]):
                if m is not None and int(m.shape[0]) < self.V:
                    raise ValueError("explain_slate: a map holds %d entries for %d logit columns" % (m.shape[0], V))
            if f.kind == 'cat' and f.maps[0] is None and int(f.table.E.shape[0]) < self.V:
                raise ValueError("explain_slate: an unmapped table of %d rows for %d logit columns"
                                 % (f.table.E.shape[0], V))
        vp = lambda xs: (C.c_void_p * n)(*[(_p(x) or None) for x in xs])
        cat = [f.kind == 'cat' for f in feats]
        self.kind = (C.c_int * n)(*[0 if c else 1 for c in cat])
        self.E = vp([f.table.E for f in feats])
        self.lde = (C.c_int64 * n)(*[_ld(f.table.E) for f in feats])
        self.bias = vp([f.table.bias if with_bias else None for f in feats])
        self.cat_map = vp([f.maps[0] if c else None for f, c in zip(feats, cat)])
        self.vals = vp([None if c else f.maps[0] for f, c in zip(feats, cat)])
        self.starts = vp([None if c else f.maps[1] for f, c in zip(feats, cat)])
        self.lens = vp([None if c else f.maps[2] for f, c in zip(feats, cat)])
        self._keep = list(feats)


def explain_slate(U, cand, es, T, feat=None, bias=None, tok_val=None, tok_id=None, tok_feat=None):
    """The parts of score(r, c) for c = cand[r, j] (arx_explain.h): feat [B, C, F] the per-feature contributions, bias
    [B, C] the bias part, tok_val / tok_id / tok_feat [B, C, T] the T largest token contributions by (value desc,
    feature asc, bag position asc), (-inf, -1, -1) past the last; an empty slot (cand < 0 or >= es.V) gives 0, 0 and
    (-inf, -1, -1).  U [B, d]; cand [B, C] int32; es an ExplainSet.  Every output may be None (tok_* together); U, cand
    and the outputs may be views whose rows are strided, the inner dimensions contiguous."""
    _chk(U, torch.float32, 'U'); _chk(cand, torch.int32, 'cand'); _chk(feat, torch.float32, 'feat')
    _chk(bias, torch.float32, 'bias'); _chk(tok_val, torch.float32, 'tok_val'); _chk(tok_id, torch.int32, 'tok_id')
    _chk(tok_feat, torch.int32, 'tok_feat')
    if U.dim() != 2 or cand.dim() != 2 or cand.shape[0] != U.shape[0] or int(U.shape[1]) != es.d:
        raise ValueError("explain_slate: U [B, %d], cand [B, C]" % es.d)
    B, C = int(cand.shape[0]), int(cand.shape[1])
    T = int(T)
    toks = (tok_val, tok_id, tok_feat)
    if any(t is None for t in toks) != all(t is None for t in toks):
        raise ValueError("explain_slate: tok_val, tok_id and tok_feat go together")

    def ld3(t, last, name):
        """row stride of t [B, C, last] whose rows are contiguous"""
        if t is None:
            return 0
        if tuple(t.shape) != (B, C, last) or (t.numel() and (t.stride(2) != 1 or t.stride(1) != last)):
            raise ValueError("explain_slate: %s must be [%d, %d, %d] with contiguous rows" % (name, B, C, last))
        return t.stride(0) if B > 1 else max(t.stride(0), C * last)
    ldf = ld3(feat, es.n, 'feat')
    ldt = ld3(tok_val, T, 'tok_val')
    if tok_val is not None and not (ld3(tok_id, T, 'tok_id') == ldt == ld3(tok_feat, T, 'tok_feat')):
        raise ValueError("explain_slate: tok_val, tok_id and tok_feat need one row stride")
    if bias is not None and tuple(bias.shape) != (B, C):
        raise ValueError("explain_slate: bias must be [%d, %d]" % (B, C))
    if cand.numel() == 0:
        return
    call("arx_explain_slate", _p(U), _ld(U), B, es.d, _p(cand), _ld(cand), C, es.V, es.n, es.kind, es.E, es.lde,
         es.bias, es.cat_map, es.vals, es.starts, es.lens, T, _p(feat), ldf, _p(bias),
         _ld(bias) if bias is not None else 0, _p(tok_val), _p(tok_id), _p(tok_feat), ldt, _stream())


def slate_mmr_supported(C, d):
    """True iff arx_slate_mmr takes a slate of C slots over rows of d floats (arx_diverse.h: the one owner of the
    rule)."""
    return bool(call("arx_slate_mmr_supported", int(C), int(d)))


def slate_mmr(P, cand, scores, lam, groups, max_per_group, k, ids, values, pos):
    """The greedy MMR re-rank of a scored slate (arx_diverse.h): k picks per row of cand / scores [B, C] by
    lam[r] * rel - (1 - lam[r]) * (largest cosine with a pick so far), cosines between the rows of P [V, d]; with groups
    [V] int32 and max_per_group [B] int32 at most that many picks per group (both None: no cap).  ids / pos int32 and
    values float32 [B, k] receive the picks in selection order, (-1, -inf, -1) past the last one.  lam [B] float32 on
    the device, every entry in [0, 1].  2-D arguments may be strided views."""
    _chk(P, torch.float32, 'P'); _chk(cand, torch.int32, 'cand'); _chk(scores, torch.float32, 'scores')
    _chk(lam, torch.float32, 'lam'); _chk(groups, torch.int32, 'groups')
    _chk(max_per_group, torch.int32, 'max_per_group'); _chk(ids, torch.int32, 'ids')
    _chk(values, torch.float32, 'values'); _chk(pos, torch.int32, 'pos')
    if P.dim() != 2 or cand.dim() != 2 or tuple(scores.shape) != tuple(cand.shape):
        raise ValueError("slate_mmr: P [V, d], cand and scores [B, C]")
    B, C, k = int(cand.shape[0]), int(cand.shape[1]), int(k)
    if any(t.dim() != 2 or tuple(t.shape) != (B, k) for t in (ids, values, pos)):
        raise ValueError("slate_mmr: ids, values and pos [B, k]")
    if lam.dim() != 1 or int(lam.shape[0]) < B or not lam.is_contiguous():
        raise ValueError("slate_mmr: lam needs one contiguous entry per row")
    if (groups is None) != (max_per_group is None):
        raise ValueError("slate_mmr: groups and max_per_group go together")
    if groups is not None and (groups.dim() != 1 or int(groups.shape[0]) < int(P.shape[0]) or max_per_group.dim() != 1
                               or int(max_per_group.shape[0]) < B):
        raise ValueError("slate_mmr: groups needs one entry per pool row, max_per_group one per row")
    call("arx_slate_mmr", _p(P), _ld(P), int(P.shape[0]), int(P.shape[1]), _p(cand), _ld(cand), _p(scores),
         _ld(scores), B, C, _p(lam), _p(groups), _p(max_per_group), k, _p(ids), _ld(ids), _p(values), _ld(values),
         _p(pos), _ld(pos), _stream())


def slate_sample_supported(C):
    """True iff arx_slate_sample takes a slate of C slots (arx_slate_sample.h: the one owner of the rule)."""
    return bool(call("arx_slate_sample_supported", int(C)))


def slate_sample(cand, scores, sample, k, ids, values, pos, logp=None):
    """k draws without replacement from softmax(scores / tau) over each row's distinct live candidates, in selection
    order, with their log-probabilities (arx_slate_sample.h).  cand int32 / scores float32 [B, C]; sample: (tau float32
    [tau_rows], tau_rows, seed_words int32 [2]) on the device, as ops.topk_gumbel_add takes it; ids / pos int32 and
    values float32 [B, k] receive the picks, (-1, -inf, -1) past the last competitor; logp float32 [B, k] or None: the
    log-probability of each pick given the picks before it (0 for a tau == 0 row and past the last competitor).  2-D
    arguments may be strided views."""
    tau, tau_rows, seed_words = sample
    _chk(cand, torch.int32, 'cand'); _chk(scores, torch.float32, 'scores'); _chk(tau, torch.float32, 'tau')
    _chk(seed_words, torch.int32, 'seed_words'); _chk(ids, torch.int32, 'ids'); _chk(values, torch.float32, 'values')
    _chk(pos, torch.int32, 'pos'); _chk(logp, torch.float32, 'logp')
    if cand.dim() != 2 or tuple(scores.shape) != tuple(cand.shape):
        raise ValueError("slate_sample: cand and scores [B, C]")
    B, C, k = int(cand.shape[0]), int(cand.shape[1]), int(k)
    if any(t.dim() != 2 or tuple(t.shape) != (B, k) for t in (ids, values, pos) + ((logp,) if logp is not None else ())):
        raise ValueError("slate_sample: ids, values, pos and logp [B, k]")
    if tau.dim() != 1 or not tau.is_contiguous() or int(tau_rows) < 1 or int(tau.shape[0]) < min(int(tau_rows), B) \
            or seed_words.dim() != 1 or int(seed_words.shape[0]) < 2 or not seed_words.is_contiguous():
        raise ValueError("slate_sample: tau needs one contiguous entry per noise row, seed_words two int32 words")
    call("arx_slate_sample", _p(cand), _ld(cand), _p(scores), _ld(scores), B, C, _p(tau), int(tau_rows),
         _p(seed_words), k, _p(ids), _ld(ids), _p(values), _ld(values), _p(pos), _ld(pos), _p(logp),
         _ld(logp) if logp is not None else 0, _stream())


def sample_logp_sort(indices, pk_cols, pk_slot):
    """The picks of every row sorted by column, (column, selection slot) with the -1 entries last (arx_sample_logp.h).
    indices int32 [B, k] (may be a strided view); pk_cols / pk_slot int32 [B, k]."""
    _chk(indices, torch.int32, 'indices'); _chk(pk_cols, torch.int32, 'pk_cols'); _chk(pk_slot, torch.int32, 'pk_slot')
    if indices.dim() != 2 or tuple(pk_cols.shape) != tuple(indices.shape) or pk_slot.shape != pk_cols.shape \
            or pk_slot.stride(0) != pk_cols.stride(0):
        raise ValueError("sample_logp_sort: indices, pk_cols, pk_slot [B, k], the two lists with one leading dimension")
    call("arx_sample_logp_sort", _p(indices), _ld(indices), int(indices.shape[0]), int(indices.shape[1]), _p(pk_cols),
         _p(pk_slot), _ld(pk_cols), _stream())


def gemm_nt_rest_mass(A, Bm, col_bias, col_base, sample, picks, m_part, s_part, pick_score, tags=None, ex=None):
    """The streaming mass pass: per row and column range of A . Bm^T + col_bias the (m, S) pair of the eligible columns
    that are no picks of the row, and the picks' scores (arx_sample_logp.h).  sample: (tau, tau_rows, seed_words) --
    the seed is not read; picks: (pk_cols, pk_slot) of sample_logp_sort; tags: (col_tags ALREADY sliced to this launch's
    columns, want_any, want_all, want_rows) or None; ex: exclusion lists or None; m_part / s_part float32
    [M, >= gemm_nt_topk_parts(M, N)]; pick_score float32 [M, k]."""
    tau, tau_rows = sample[0], sample[1]
    pk_cols, pk_slot = picks
    col_tags, want_any, want_all, want_rows = tags if tags is not None else (None, None, None, 0)
    if tags is not None and int(col_tags.shape[0]) < int(Bm.shape[0]):
        raise ValueError("gemm_nt_rest_mass: %d tag words for %d columns" % (int(col_tags.shape[0]), int(Bm.shape[0])))
    if pk_slot.stride(0) != pk_cols.stride(0) or s_part.stride(0) != m_part.stride(0):
        raise ValueError("gemm_nt_rest_mass: pk_cols / pk_slot and m_part / s_part each share a leading dimension")
    keys, key_rows, ptr, cols = ex if ex is not None else (None, 0, None, None)
    call("arx_gemm_nt_rest_mass", _p(A), _ld(A), int(A.shape[0]), _p(Bm), _ld(Bm), int(Bm.shape[0]), int(A.shape[1]),
         _p(col_bias), int(col_base), _p(tau), int(tau_rows), _p(keys), int(key_rows), _p(ptr), _p(cols), _p(col_tags),
         _p(want_any), _p(want_all), int(want_rows), _p(pk_cols), _p(pk_slot), _ld(pk_cols), int(pk_cols.shape[1]),
         _p(m_part), _p(s_part), int(m_part.stride(0)), _p(pick_score), _ld(pick_score), _stream())


def rest_mass_chunk(logits, col0, sample, picks, first, m_run, s_run, pick_score):
    """The materialised mass pass: the columns [col0, col0 + logits.shape[1]) of logits (-inf where ineligible) folded
    into each row's running pair (m_run, s_run) [B] -- first: the pairs start empty -- without the row's picks, whose
    scores go to pick_score [B, k] (arx_sample_logp.h)."""
    tau, tau_rows = sample[0], sample[1]
    pk_cols, pk_slot = picks
    if pk_slot.stride(0) != pk_cols.stride(0):
        raise ValueError("rest_mass_chunk: pk_cols and pk_slot share a leading dimension")
    call("arx_rest_mass_chunk", _p(logits), _ld(logits), int(logits.shape[0]), int(col0), int(logits.shape[1]),
         _p(tau), int(tau_rows), _p(pk_cols), _p(pk_slot), _ld(pk_cols), int(pk_cols.shape[1]), int(bool(first)),
         _p(m_run), _p(s_run), _p(pick_score), _ld(pick_score), _stream())


def sample_logp_finish(indices, pick_score, m_part, s_part, P, sample, logp, values=None):
    """logp [B, k] of the picks `indices` in selection order from REST's P parts per row and the picks' scores; values
    (optional) receive those scores, -inf beside an index -1 (arx_sample_logp.h).  m_part / s_part: [B, >= P], or the
    running pairs [B] with P = 1."""
    tau, tau_rows = sample[0], sample[1]
    _chk(logp, torch.float32, 'logp'); _chk(values, torch.float32, 'values'); _chk(indices, torch.int32, 'indices')
    if tuple(logp.shape) != tuple(indices.shape) or (values is not None and values.shape != logp.shape):
        raise ValueError("sample_logp_finish: indices, logp and values [B, k]")
    ldl = int(m_part.stride(0)) if m_part.dim() == 2 else 1
    if (int(s_part.stride(0)) if s_part.dim() == 2 else 1) != ldl:
        raise ValueError("sample_logp_finish: m_part and s_part share a leading dimension")
    call("arx_sample_logp_finish", _p(indices), _ld(indices), _p(pick_score), _ld(pick_score), _p(m_part), _p(s_part),
         ldl, int(P), _p(tau), int(tau_rows), int(indices.shape[0]), int(indices.shape[1]), _p(logp), _ld(logp),
         _p(values), _ld(values) if values is not None else 0, _stream())


def list_logp_prepare(lists, V, ex, tags, clean, why, pk_cols, pk_slot):
    """A foreign list made fit for the mass pass (arx_list_logp.h): lists int32 [B, k] of logit indices in [0, V), -1 an
    empty slot, anything else allowed; ex: exclusion lists (row_keys, key_rows, ex_ptr, ex_cols) or None; tags:
    (col_tags [V] by ABSOLUTE column, want_any, want_all, want_rows) or None.  clean int32 [B, k]: the column where the
    entry may still be drawn, else -1; why int32 [B, k]: the reason codes 0-5; pk_cols / pk_slot int32 [B, k]: what
    sample_logp_sort writes for `clean`."""
    for t, n in ((lists, 'lists'), (clean, 'clean'), (why, 'why'), (pk_cols, 'pk_cols'), (pk_slot, 'pk_slot')):
        _chk(t, torch.int32, n)
    if lists.dim() != 2 or any(tuple(t.shape) != tuple(lists.shape) for t in (clean, why, pk_cols, pk_slot)) \
            or pk_slot.stride(0) != pk_cols.stride(0):
        raise ValueError("list_logp_prepare: lists, clean, why, pk_cols, pk_slot [B, k], the two sorted lists with one "
                         "leading dimension")
    col_tags, want_any, want_all, want_rows = tags if tags is not None else (None, None, None, 0)
    if tags is not None and int(col_tags.shape[0]) < int(V):
        raise ValueError("list_logp_prepare: %d tag words for %d columns" % (int(col_tags.shape[0]), int(V)))
    keys, key_rows, ptr, cols = ex if ex is not None else (None, 0, None, None)
    call("arx_list_logp_prepare", _p(lists), _ld(lists), int(lists.shape[0]), int(lists.shape[1]), int(V), _p(keys),
         int(key_rows), _p(ptr), _p(cols), _p(col_tags), _p(want_any), _p(want_all), int(want_rows), _p(clean),
         _ld(clean), _p(why), _ld(why), _p(pk_cols), _p(pk_slot), _ld(pk_cols), _stream())


def list_logp_stamp(clean, pick_score, why, logp, values=None):
    """After sample_logp_finish on `clean` (arx_list_logp.h): why = 6 where a clean entry's score came out -inf, then
    logp (and values, optional) = -inf at every entry of code >= 2.  All [B, k]."""
    _chk(clean, torch.int32, 'clean'); _chk(why, torch.int32, 'why'); _chk(pick_score, torch.float32, 'pick_score')
    _chk(logp, torch.float32, 'logp'); _chk(values, torch.float32, 'values')
    if clean.dim() != 2 or any(tuple(t.shape) != tuple(clean.shape) for t in (pick_score, why, logp)) \
            or (values is not None and values.shape != clean.shape):
        raise ValueError("list_logp_stamp: clean, pick_score, why, logp and values [B, k]")
    call("arx_list_logp_stamp", _p(clean), _ld(clean), _p(pick_score), _ld(pick_score), int(clean.shape[0]),
         int(clean.shape[1]), _p(why), _ld(why), _p(logp), _ld(logp), _p(values),
         _ld(values) if values is not None else 0, _stream())


def list_logp_prepare_shard(lists, V_global, W, s, ex, tags, clean, why, pk_cols, pk_slot):
    """list_logp_prepare on shard s of W (arx_list_logp_shard.h): lists int32 [B, k] of GLOBAL ids; an in-range entry of
    another shard is no pick (code 0), an owned one is tested as the LOCAL column id // W against ex (local columns) and
    tags (col_tags of the shard's rows, want_any, want_all, want_rows).  clean: local columns; why: the codes (may be a
    strided int32 view, e.g. into a packed exchange buffer); pk_cols / pk_slot: what picks_to_shard + sample_logp_sort
    write for the merged clean list."""
    for t, n in ((lists, 'lists'), (clean, 'clean'), (why, 'why'), (pk_cols, 'pk_cols'), (pk_slot, 'pk_slot')):
        _chk(t, torch.int32, n)
    if lists.dim() != 2 or any(tuple(t.shape) != tuple(lists.shape) for t in (clean, why, pk_cols, pk_slot)) \
            or pk_slot.stride(0) != pk_cols.stride(0) or any(t.stride(1) != 1 for t in (lists, clean, why, pk_cols)):
        raise ValueError("list_logp_prepare_shard: lists, clean, why, pk_cols, pk_slot [B, k] with unit stride along a "
                         "row, the two sorted lists with one leading dimension")
    col_tags, want_any, want_all, want_rows = tags if tags is not None else (None, None, None, 0)
    if not 0 <= int(s) < int(W):
        raise ValueError("list_logp_prepare_shard: need 0 <= s < W")
    rows = len(range(int(s), int(V_global), int(W)))
    if tags is not None and int(col_tags.shape[0]) < rows:
        raise ValueError("list_logp_prepare_shard: %d tag words for the shard's %d rows" % (int(col_tags.shape[0]), rows))
    keys, key_rows, ptr, cols = ex if ex is not None else (None, 0, None, None)
    call("arx_list_logp_prepare_shard", _p(lists), _ld(lists), int(lists.shape[0]), int(lists.shape[1]), int(V_global),
         int(W), int(s), _p(keys), int(key_rows), _p(ptr), _p(cols), _p(col_tags), _p(want_any), _p(want_all),
         int(want_rows), _p(clean), _ld(clean), _p(why), _ld(why), _p(pk_cols), _p(pk_slot), _ld(pk_cols), _stream())


def list_logp_merge_shards(lists, V_global, codes, clean, why):
    """The owner's merge (arx_list_logp_shard.h): lists int32 [B, k] of GLOBAL ids; codes int32 [W, B, k], shard-major
    slabs of what list_logp_prepare_shard wrote for these rows (a view into the packed exchange buffer is fine: unit
    stride along a row) -> why [B, k] (1 at -1, 2 out of range, else the owner shard's code) and clean [B, k] (the id
    where why is 0, else -1)."""
    for t, n in ((lists, 'lists'), (codes, 'codes'), (clean, 'clean'), (why, 'why')):
        _chk(t, torch.int32, n)
    if lists.dim() != 2 or codes.dim() != 3 or tuple(codes.shape[1:]) != tuple(lists.shape) or codes.stride(2) != 1 \
            or any(tuple(t.shape) != tuple(lists.shape) or t.stride(1) != 1 for t in (clean, why)) or lists.stride(1) != 1:
        raise ValueError("list_logp_merge_shards: lists, clean, why [B, k] and codes [W, B, k], unit stride along a row")
    call("arx_list_logp_merge_shards", _p(lists), _ld(lists), int(lists.shape[0]), int(lists.shape[1]), int(V_global),
         _p(codes), int(codes.stride(1)), int(codes.stride(0)), int(codes.shape[0]), _p(clean), _ld(clean), _p(why),
         _ld(why), _stream())


def picks_to_shard(ids, W, s, cols):
    """cols[r, j] = ids[r, j] // W where the global id ids[r, j] >= 0 belongs to shard s of W (id % W == s), else -1
    (arx_sample_shard.h).  ids / cols int32 [B, k]."""
    _chk(ids, torch.int32, 'ids'); _chk(cols, torch.int32, 'cols')
    if ids.dim() != 2 or tuple(cols.shape) != tuple(ids.shape):
        raise ValueError("picks_to_shard: ids and cols [B, k]")
    call("arx_picks_to_shard", _p(ids), _ld(ids), int(ids.shape[0]), int(ids.shape[1]), int(W), int(s), _p(cols),
         _ld(cols), _stream())


def sample_logp_finish_shards(indices, pick_score, m_part, s_part, P, sample, logp, values=None):
    """sample_logp_finish over W shard-major slabs (arx_sample_shard.h): m_part / s_part [W, B, >= P] and pick_score
    [W, B, k] (views of one packed buffer are fine: each slab [B, .] with its row stride, the slabs one stride apart);
    indices [B, k]: GLOBAL ids in selection order -- pick t's score is read from slab id % W."""
    tau, tau_rows = sample[0], sample[1]
    _chk(logp, torch.float32, 'logp'); _chk(values, torch.float32, 'values'); _chk(indices, torch.int32, 'indices')
    if tuple(logp.shape) != tuple(indices.shape) or (values is not None and values.shape != logp.shape):
        raise ValueError("sample_logp_finish_shards: indices, logp and values [B, k]")
    B, k = int(indices.shape[0]), int(indices.shape[1])
    W = int(m_part.shape[0])
    if m_part.dim() != 3 or s_part.dim() != 3 or pick_score.dim() != 3 or int(pick_score.shape[0]) != W \
            or int(s_part.shape[0]) != W or s_part.stride() != m_part.stride() or int(m_part.shape[2]) < int(P) \
            or tuple(pick_score.shape[1:]) != (B, k) or int(m_part.shape[1]) != B \
            or m_part.stride(2) != 1 or pick_score.stride(2) != 1:
        raise ValueError("sample_logp_finish_shards: m_part / s_part [W, B, >= P] with the same strides, pick_score "
                         "[W, B, k], unit stride along a row")
    call("arx_sample_logp_finish_shards", _p(indices), _ld(indices), _p(pick_score), int(pick_score.stride(1)),
         int(pick_score.stride(0)), _p(m_part), _p(s_part), int(m_part.stride(1)), int(m_part.stride(0)), W, int(P),
         _p(tau), int(tau_rows), B, k, _p(logp), _ld(logp), _p(values), _ld(values) if values is not None else 0,
         _stream())


def lstm_fwd(x, W, b, L, B, din, h, forget_bias, hs, cs, gates):
    call("arx_lstm_fwd", _p(x), _p(W), _p(b), int(L), int(B), int(din), int(h), float(forget_bias),
         _p(hs), _p(cs), _p(gates), _stream())


def lstm_bwd(W, hs, cs, gates, dhs, L, B, din, h, dz, wxt=None):
    """dz of the whole unrolled cell; wxt (optional, [4h, din]) receives W[:din]^T on the way."""
    call("arx_lstm_bwd", _p(W), _p(hs), _p(cs), _p(gates), _p(dhs), int(L), int(B), int(din),
         int(h), _p(dz), _p(wxt), _stream())


def gru_fwd(x, Wg, bg, Wc, bc, L, B, din, h, hs, gates, rh):
    """TF's GRUCell over L steps from the zero state: hs [L*B, h], gates [L*B, 3h] (r, u, c), rh [L*B, h] = r * h_prev."""
    call("arx_gru_fwd", _p(x), _p(Wg), _p(bg), _p(Wc), _p(bc), int(L), int(B), int(din), int(h), _p(hs), _p(gates),
         _p(rh), _stream())


def gru_bwd(Wg, Wc, hs, gates, dhs, L, B, din, h, dzg, dzc):
    """dzg [L*B, 2h] (dzr, dzu) and dzc [L*B, h] of the whole unrolled cell."""
    call("arx_gru_bwd", _p(Wg), _p(Wc), _p(hs), _p(gates), _p(dhs), int(L), int(B), int(din), int(h), _p(dzg),
         _p(dzc), _stream())


def seq_weights(w, L, B, out):
    call("arx_seq_weights", _p(w), int(L), int(B), _p(out), _stream())


@contextlib.contextmanager
def joined(stream):
    """Run the block on `stream`, joined with the current stream on both sides: `stream` waits for the work queued
    so far, the current stream waits for the block's.  None, or the stream that is current already: nothing to join.
    (A block that raises is not waited for.)"""
    outer = torch.cuda.current_stream(stream.device) if stream is not None else None
    if outer is None or outer == stream:
        yield
        return
    stream.wait_stream(outer)
    with torch.cuda.stream(stream):
        yield
    outer.wait_stream(stream)


class CapturedGraph(object):
    """A hipGraph of one step (arx_capture_* in include/arx.h).  end(feeds=...): the placeholder feeds issued inside
    the capture (copy_words) stay addressable -- set_feeds() swaps their sources before a replay.  record() and
    replay() are the one place a step graph is recorded and re-fed; begin / end / set_feeds are their parts."""

    def __init__(self):
        import ctypes as C
        self._exec = C.c_void_p(0)
        self._feeds = C.c_void_p(0)
        self.feed_groups = None      # per captured copy node: the destination pointers of its (<= 8) feeds, in order
        self._node_of = []           # group index -> node index
        self._fed = False            # the nodes hold live sources (else: they copy nothing)

    @classmethod
    def record(cls, fn, feeds=None, fork=False):
        """Capture the launches of fn() -- behind the copy of `feeds` ([(src, dst)]: the graph's first node(s), see
        replay) -- and return the instantiated graph; it has not run.  fork: on a fresh stream forked from and joined
        back to the current one (the legacy default stream cannot be captured); else on the current stream."""
        g = cls()
        with joined(torch.cuda.Stream() if fork else None):
            g.begin()
            try:
                if feeds:
                    copy_words(feeds)
                fn()
            except BaseException:
                # (the capture may already be invalidated: ending it raises again -- the ORIGINAL error is the
                # one that has to surface; advisor, round 4)
                try:
                    g.end()
                except BaseException:
                    pass
                raise
            g.end(feeds=feeds)
        return g

    def replay(self, feeds=None):
        """Launch with this step's feeds: swapped into the captured feed nodes where they address the captured
        destinations, else copied eagerly in front (the nodes then copy nothing).  None / []: nothing is fed."""
        if feeds and self.feeds_match(feeds):
            self.set_feeds(feeds)
        else:
            if feeds:
                copy_words(feeds)            # other placeholders than the captured ones: fed eagerly
            self.set_feeds(None)
        self.launch()

    def begin(self):
        # no cyclic garbage collection between begin() and end(): a collection there runs the finalizers of
        # unreachable models -- CapturedGraph.__del__ (hipGraphExecDestroy), the feed slabs' release (a device
        # synchronize) -- and those HIP calls are illegal inside a capture: it is invalidated, and the next launch
        # fails "due to a previous error during capture".  Whether a collection lands there depends on the
        # allocation counts of the whole process, so the failure came and went with unrelated changes.
        self._gc_was_enabled = gc.isenabled()
        gc.disable()
        try:
            call("arx_capture_begin", _stream())
        except BaseException:
            self._gc_restore()
            raise

    def _gc_restore(self):
        if getattr(self, '_gc_was_enabled', False):
            gc.enable()
        self._gc_was_enabled = False

    def end(self, feeds=None):
        """feeds: the [(src, dst), ...] list copy_words() was called with inside this capture (None: no feed nodes)."""
        try:
            self._end(feeds)
        finally:
            self._gc_restore()

    def _end(self, feeds):
        import ctypes as C
        if not feeds:
            call("arx_capture_end", _stream(), C.byref(self._exec))
            return
        n = C.c_int(0)
        call("arx_capture_end_feeds", _stream(), C.byref(self._exec), C.byref(self._feeds), C.byref(n))
        groups = [feeds[k:k + 8] for k in range(0, len(feeds), 8)]
        first = {}
        for i in range(n.value):
            d0 = C.c_void_p(0)
            call("arx_graph_feed_dst0", self._feeds, i, C.byref(d0))
            first[d0.value] = i
        node_of = [first.get(g[0][1].data_ptr()) for g in groups]
        if n.value != len(groups) or None in node_of or len(set(node_of)) != len(groups):
            raise RuntimeError("captured step: %d feed node(s) found for %d feed group(s)" % (n.value, len(groups)))
        self._node_of = node_of
        self.feed_groups = [tuple((d.data_ptr(), d.numel()) for _, d in g) for g in groups]
        self._fed = True

    def feeds_match(self, feeds):
        """Do these pending feeds address exactly the destinations the capture's feed nodes write?"""
        if self.feed_groups is None:
            return False
        groups = [feeds[k:k + 8] for k in range(0, len(feeds), 8)]
        return [tuple((d.data_ptr(), d.numel()) for _, d in g) for g in groups] == self.feed_groups

    def set_feeds(self, feeds):
        """The sources the feed nodes copy at the next launches; None / []: they copy nothing."""
        import ctypes as C
        if self.feed_groups is None or (not feeds and not self._fed):
            return
        for gi, ni in enumerate(self._node_of):
            grp = feeds[gi * 8:(gi + 1) * 8] if feeds else []
            n = len(grp)
            src, dst, cnt = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))(), (C.c_int64 * max(n, 1))()
            for a, (s_, d_) in enumerate(grp):
                if s_.element_size() != 4 or d_.element_size() != 4 or s_.numel() != d_.numel():
                    raise ValueError("set_feeds: 4-byte tensors of equal size expected")
                src[a], dst[a], cnt[a] = s_.data_ptr(), d_.data_ptr(), s_.numel()
            call("arx_graph_set_feed", self._exec, self._feeds, ni, n, src, dst, cnt)
        self._fed = bool(feeds)

    def launch(self):
        call("arx_graph_launch", self._exec, _stream())

    def __del__(self):
        try:
            if self._exec:
                _lib.lib.arx_graph_destroy(self._exec)
            if self._feeds:
                _lib.lib.arx_graph_feeds_destroy(self._feeds)
        except Exception:
            pass
