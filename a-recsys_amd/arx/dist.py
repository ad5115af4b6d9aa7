"""Row-sharded HMF step over RCCL / xGMI.

One process per GPU (torch.distributed; backend "nccl" is RCCL on ROCm).  The
item embedding table (+ bias, + Adagrad slots) is striped row-wise over the
ranks (owner = item % world); the user table is striped the same way and every
rank trains on interactions of ITS users (pure data parallelism on that side).
One step with B = world * B_loc interactions and a pool of S shared negatives
(S/world owned by each rank) is algebraically the single-process step of
hmf_model.py on the global batch.  Exchanges per step and rank (SURVEY 8e's
"gather the pool rows" alternative -- the [B, S] logits never cross xGMI):

  all_gather      owned pool rows [S/N, d+4] -> pool [S, d+4]        (0.5 MB at S=1024, d=128)
  all_to_all(v)   target item ids  -> their owners                   (4 B per interaction; input routing,
                                                                      done with the batch in prepare_route())
  all_to_all(v)   target rows [*, d+4] back                          (B_loc rows, (N-1)/N cross)
  (local)         logits = U_loc . pool^T + b, WMRB loss, dU, user-shard Adagrad
  reduce_scatter  pool gradient partials [S, d+4] -> owner blocks    (0.5 MB)
  all_to_all(v)   target-row gradients -> owners                     (B_loc rows)
  (local)         item-shard scatter + Adagrad (pool block + received target gradients)

(column d of the packed rows carries the bias / bias gradient.)  Per rank ~2 x B_loc x (d+4) x 4
bytes move per step instead of 2 x B x S x 4 / N for an all-to-all of the logits (16.5 MB vs
134 MB at B_loc=16384, S=1024).  The variable-size exchanges need per-destination counts: they
are a property of the batch (owner = item % N), computed by the data loader on the host
(`prepare_route`), which also orders the batch by owner so the device never permutes rows.
No table gradient ever crosses xGMI and there is no ring all-reduce on the path (the dense
LSTM weights of the sequence model would use one, 128 KB, latency-bound).

The compute stages go through a `backend` object; the product backend is
HipBackend (libarx.so).  tests/ injects a numpy backend to check the sharded
algorithm against the single-process oracle with gloo on CPU -- the package
itself contains no CPU implementation.
"""
from __future__ import annotations

import json
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from . import ops as _ops
from . import slate as _slate
from .topk import (LogpBuffers, TopKScan, check_lists, check_return_logprob, list_taus, no_return_logprob,
                   run_complete, sample_params, similar_scan, tag_words)
from .utils.prepare_train import pair_draw_tables


class _Done(object):
    def wait(self):
        return True


def _all_to_all(out, inp, out_splits=None, in_splits=None, group=None, async_op=False):
    """dist.all_to_all_single -- RCCL in production.  Test rigs run several ranks on ONE GPU over gloo,
    which has no all-to-all for device tensors: there the blocks are staged through the host."""
    if inp.is_cuda and dist.get_backend(group) == 'gloo':
        o = torch.empty(out.shape, dtype=out.dtype)
        dist.all_to_all_single(o, inp.cpu().contiguous(), output_split_sizes=out_splits,
                               input_split_sizes=in_splits, group=group)
        out.copy_(o)
        return _Done()
    w = dist.all_to_all_single(out, inp, output_split_sizes=out_splits, input_split_sizes=in_splits, group=group,
                               async_op=async_op)
    return w if async_op else _Done()


def _reduce_scatter(out, inp, group=None):
    """dist.reduce_scatter_tensor (sum) -- RCCL in production; device tensors over gloo (several ranks on ONE GPU:
    the test rigs) are summed through the host and every rank keeps its block."""
    if inp.is_cuda and dist.get_backend(group) == 'gloo':
        t = inp.cpu().contiguous()
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        n = out.shape[0]
        r = dist.get_rank(group)
        out.copy_(t[r * n:(r + 1) * n])
        return
    dist.reduce_scatter_tensor(out, inp, op=dist.ReduceOp.SUM, group=group)


def owner_order(ids, world):
    """Requests for the rows of global ids `ids` (owner = id % world), ordered by owner -- host only:
    (perm, slot, send): perm orders the requests by owner (stable: inside an owner's group they keep their order),
    slot[i] = place of request i in that order (the inverse of perm: its row of the block that comes back),
    send[g] = number of requests to owner g (int64 [world])."""
    owner = np.asarray(ids) % world
    perm = np.argsort(owner, kind='stable')
    slot = np.empty(len(perm), dtype=np.int32)
    slot[perm] = np.arange(len(perm), dtype=np.int32)
    return perm, slot, np.bincount(owner, minlength=world).astype(np.int64)


class HipBackend(object):
    """Compute stages on libarx.so (include/arx.h)."""

    def __init__(self, device):
        from . import ops
        self.ops = ops
        self.ws = ops.Workspace(device)
        self.ws_k7 = ops.Workspace(device)     # K7's own: its sort half may run ahead, under the GEMMs (which use ws)

    def gather_rows(self, E, bias, rows, out, bias_out, scale=1.0):
        self.ops.gather_onehot(E, bias, None, rows, out, scale=scale, bias_out=bias_out)

    def gather_bags(self, E, bias, vals, starts, lens, ids, out, bias_out, scale=1.0, accumulate=False):
        """out[r] (+)= scale * mean over the bag of ids[r] of E rows; bias_out likewise."""
        self.ops.gather_mulhot_mean(E, bias, vals, starts, lens, ids, out, scale=scale, accumulate=accumulate,
                                    bias_out=bias_out)

    def bags_adagrad(self, E, acc, bias, bias_acc, vals, starts, lens, sites, G, Gb, lr, phase=_ops.K7_BOTH):
        """Two-stage multi-hot pass (arx_sparse_adagrad_bags); sites: [(entity ids, row_base, coef)].
        Tokens >= E.shape[0] (rows of other shards, mapped to the padding row) are dropped.
        phase ops.K7_SORT: both sorts (ids only), K7_APPLY: merge + apply, K7_BOTH: both."""
        ops = self.ops
        # one workspace per SHAPE of the pass (counts, row bases, coefficients); the id tensors may be
        # fresh every step (prepare_route): only the pointer arrays are rebuilt then
        key = tuple((int(i.shape[0]), b, c) for i, b, c in sites)
        ptrs = tuple(i.data_ptr() for i, _, _ in sites)
        cache = self.__dict__.setdefault('_bags', {})
        ent = cache.get(key)
        mx = self.__dict__.setdefault('_bag_maxlen', {})
        if lens.data_ptr() not in mx:
            mx[lens.data_ptr()] = (lens, int(lens.max().item()))      # (the tensor is kept: its address stays its own)
        if ent is None:
            ent = cache[key] = [None, None, ops.Workspace(G.device)]
        if ent[0] != ptrs:
            ent[0], ent[1] = ptrs, ops.BagSiteArgs(sites, mx[lens.data_ptr()][1])
        ops.sparse_adagrad_bags(E, acc, bias, bias_acc, vals, starts, lens, ent[1], G, Gb, lr, ent[2], phase=phase)

    def lookup_het_multi(self, sites):
        """The step's lookups in ONE launch (arx_lookup_multi) where items are HET (id row + bag mean, both halved):
        sites = LookupSet tuples (E_id, bias_id, cat_map, E_tok, bias_tok, vals, starts, lens, ids, out, scale,
        bias_out); static buffers: the descriptor is built once per set of addresses."""
        key = tuple((x[8].data_ptr(), int(x[8].shape[0]), x[9].data_ptr()) for x in sites)
        cache = self.__dict__.setdefault('_lsets', {})
        ls = cache.get(key)
        if ls is None:
            if len(cache) > 16:
                cache.clear()
            ls = cache[key] = self.ops.LookupSet(sites)
        self.ops.lookup_multi(ls)

    def gather_rows_packed(self, E, bias, rows, out):
        self.ops.gather_onehot_packed(E, bias, None, rows, out)

    def gather_rows_multi(self, sites):
        """Several lookups of equal width in one launch; sites: [(E, bias|None|column, rows, out, bias_out)],
        bias an int: that column of E's (packed) rows; bias_out None | a vector | 'packed' (column d of the
        out rows).  Static buffers: the descriptor
        is built once per set of addresses."""
        key = tuple((E.data_ptr(), bi if isinstance(bi, int) else -1, r.data_ptr(), int(r.shape[0]), o.data_ptr(),
                     b if isinstance(b, str) else (b.data_ptr() if b is not None else 0)) for E, bi, r, o, b in sites)
        cache = self.__dict__.setdefault('_gsets', {})
        gs = cache.get(key)
        if gs is None:
            if len(cache) > 16:
                cache.clear()
            gs = cache[key] = self.ops.GatherSet([(E, bias, None, r, o, 1.0, b) for E, bias, r, o, b in sites])
        self.ops.gather_onehot_multi(gs)

    def gemm(self, A, B, C, transA=False, transB=False, beta=0.0, col_bias=None, a_rowsum=None):
        self.ops.gemm(A, B, C, self.ws, transA=transA, transB=transB, beta=beta, col_bias=col_bias,
                      a_rowsum=a_rowsum)

    def dot_score(self, U, T, tb, out):
        self.ops.dot_score(U, T, tb, out)

    def copy_2d(self, src, dst):
        self.ops.copy_2d(src, dst)

    def copy_words(self, feeds):
        """[(src, dst)] of 4-byte elements, one launch per eight pairs: the per-batch index vectors of a step."""
        self.ops.copy_words(feeds)

    def copy_strided(self, src, dst):
        self.ops.copy_strided(src, dst)

    def rows_fingerprint(self, x, row0, row_step, out):
        """out (an int64 device word) += the striping-independent fingerprint of the rows of x (arx_rows_fingerprint)."""
        self.ops.rows_fingerprint(x, row0, row_step, out)

    def transpose(self, src, dst):
        self.ops.transpose(src, dst)

    def gather_rows_wide(self, src, rows, dst):
        self.ops.gather_rows_wide(src, rows, dst)

    def add_2d(self, src, dst):
        """dst += src (2-D, any row strides)."""
        self.ops.add_rows_bcast(1.0, src, 1.0, dst)

    def shard_route(self, ids, world, rank, zero_row, rows_out, keys_out):
        self.ops.shard_route(ids, world, rank, zero_row, rows_out, keys_out)

    def pool_blocks(self, ids, world, rank, zero_row, cap, counts, gidx=None, my_slots=None, pool_rows=None):
        self.ops.pool_blocks(ids, world, rank, zero_row, cap, counts, gidx, my_slots, pool_rows)

    def loss_mw_fused_pos(self, logits, U, T, tb, urows, ptr, items, i2s, bl, dl, t_out, dt, dU, dT, gscale,
                          kind='mw'):
        """loss ('mw' | 'mce') + target score + rank-one gradients in one kernel; tb / dt may be strided columns."""
        self.ops.loss_mw_fused_pos(logits, U, T, tb, urows, ptr, items, i2s, bl, dl, t_out, dt, dU, dT, gscale,
                                   kind=kind)

    def pair_loss_slots(self, U, R, pos_slot, neg_slot, kind, gscale, pos_score, neg_score, bl, dU, dR, counts):
        """'bpr' / 'bpr-hinge' of row r against the packed rows R[pos_slot[r]] / R[neg_slot[r]] (bias in column d):
        scores, loss, dU (written) and the two gradient rows into the same slots of dR; neg_slot < 0: a void row.
        counts: int32 [2] = (sum of sign(neg - pos), rows that are not void) (arx_pair_loss_slots)."""
        self.ops.pair_loss_slots(U, R, pos_slot, neg_slot, kind, gscale, pos_score, neg_score, bl, dU=dU, dR=dR,
                                 auc_counts=counts)

    def window_slots_fwd(self, R, slots, n, scale, base, base_scale, out):
        """out[b] = base_scale * base[b] + scale * sum_t R[slots[t * mb + b]], ascending t (arx_window_slots_fwd)."""
        self.ops.window_slots_fwd(R, slots, n, out, scale=scale, base=base, base_scale=base_scale)

    def window_slots_bwd(self, dX, slots, n, scale, base_scale, dbase, acc_dbase, dR):
        """dbase[b] (+)= base_scale * dX[b]; dR[slots[t * mb + b]] = scale * dX[b] for every t; rows of dR that no
        slot names keep what they held (arx_window_slots_bwd)."""
        self.ops.window_slots_bwd(dX, slots, n, dbase, dR, scale=scale, base_scale=base_scale, acc_dbase=acc_dbase)

    def neg_draw_uniform(self, urows, ex_ptr, ex_cols, V, seed, counter, out):
        """out[r] = one item of [0, V) outside the sorted, unique list of local user row urows[r] (CSR ex_ptr /
        ex_cols), uniform by rank-select, keyed by (seed, counter, r); -1 where the list is all of [0, V)
        (arx_neg_draw_uniform, no col2item)."""
        self.ops.neg_draw_uniform(urows, ex_ptr, ex_cols, V, None, seed, None, counter, out)

    def neg_draw_weighted(self, urows, ex_ptr, ex_cols, ex_cum, cum, V, seed, counter, out):
        """out[r] = one item of [0, V) outside the list of local user row urows[r], drawn in proportion to the integer
        weights whose exclusive prefix sum is cum (int64 [V + 1]; ex_cum: the prefix sums along each list), keyed by
        (seed, counter, r); -1 where no weight is left outside the list (arx_neg_draw_weighted, no col2item)."""
        self.ops.neg_draw_weighted(urows, ex_ptr, ex_cols, ex_cum, cum, V, None, seed, None, counter, out)

    def sum_scaled(self, x, scale, out):
        self.ops.sum_scaled(x, scale, out)

    def sparse_adagrad_multi(self, tables, sites, G, Gb, lr, phase=_ops.K7_BOTH):
        """tables: [(E, acc, bias|None, bias_acc|None)]; sites: [(table, local_rows, row_base)]:
        one fused pass (arx_sparse_adagrad_cat_multi).  phase ops.K7_SORT: keys + sorts + run records (needs the
        ids only), K7_APPLY: apply, K7_BOTH: both."""
        ops = self.ops
        sites = [(x[0], x[1], x[2], x[3] if len(x) > 3 else 1.0) for x in sites]   # (table, rows, base[, coef])
        key = tuple((t, r.data_ptr(), int(r.shape[0]), b, c) for t, r, b, c in sites)
        cache = self.__dict__.setdefault('_multi', {})
        ent = cache.get(key)
        if ent is None:
            if len(cache) > 64:
                cache.clear()
            dev = G.device
            cnts = self.__dict__.setdefault('_cnt', {})
            tabs = []
            for E, acc, bias, bacc in tables:
                ck = (E.data_ptr(), int(E.shape[0]))      # (E_item[:ni] and E_item share a pointer, not a row count)
                c = cnts.get(ck)
                if c is None:
                    c = cnts[ck] = torch.zeros((E.shape[0],), dtype=torch.int32, device=dev)
                tabs.append((E, acc, bias, bacc, c))
            args = ops.MultiCatArgs(tabs, [(t, None, r, b, c) for t, r, b, c in sites])
            n = max(args.total, 1)
            bufs = self.__dict__.get('_multi_bufs')
            if bufs is None or bufs[0].shape[0] < n:
                bufs = self._multi_bufs = (torch.empty(n, dtype=torch.int32, device=dev),
                                           torch.empty(n, dtype=torch.int32, device=dev),
                                           torch.empty(n, dtype=torch.float32, device=dev))
            ent = cache[key] = args
        kb, sb, cb = self._multi_bufs
        if kb.shape[0] < ent.total:
            self._multi_bufs = kb, sb, cb = (torch.empty(ent.total, dtype=torch.int32, device=G.device),
                                             torch.empty(ent.total, dtype=torch.int32, device=G.device),
                                             torch.empty(ent.total, dtype=torch.float32, device=G.device))
        ops.sparse_adagrad_cat_multi(ent, G, Gb, lr, kb, sb, cb, self.ws_k7, phase=phase)

    def bags_grad_dense(self, D, Db, vals, starts, lens, sites, G, Gb, phase=_ops.K7_BOTH):
        """D[t] += sum of the gradient rows of the bags that hold token t (coefficient coef / len), Db likewise: the
        two-stage multi-hot pass in its gradient-descent form (no slots) with a step of -1 onto a gradient table --
        0 - (-1) g = g, the merged sums themselves, bit for bit.  Tokens >= D.shape[0] are dropped."""
        if getattr(self, '_neg_one', None) is None:
            self._neg_one = torch.tensor([-1.0], dtype=torch.float32, device=D.device)
        self.bags_adagrad(D, None, Db, None, vals, starts, lens, sites, G, Gb, self._neg_one, phase=phase)

    def adagrad_rows_nonzero(self, W, acc, bias, bias_acc, G, Gb, lr):
        """Adagrad on the rows whose dense gradient row is not all zero; the consumed gradient is zeroed (arx.h)."""
        self.ops.adagrad_rows_nonzero(W, acc, bias, bias_acc, G, Gb, lr)

    def fill_zero(self, t):
        self.ops.fill_f32(t, 0.0)

    def take_i32(self, table, idx, out, fill):
        self.ops.take_i32(table, idx, out, fill=fill)

    def slot_map_set(self, m, ids, clear):
        self.ops.slot_map_set(m, ids, clear=clear)

    def attach_pool_bitmap(self, m, bits):
        self.ops.slot_map_attach_bitmap(m, bits)

    def copy_i32(self, src, dst):
        dst.copy_(src, non_blocking=True)

    def het_rows_range(self, E_id, bias_id, E_tok, bias_tok, vals, starts, lens, n_items, world, rank, c0, c1, out,
                       bias_out=None, all_owners=False, scale=0.5, block_rows=0):
        """HET rows of the shard columns [c0, c1) -- of this rank, or of every owner in owner-major blocks -- with no
        id array (arx_het_rows_range); bias_out None: column d of the (packed) out rows."""
        self.ops.het_rows_range(E_id, bias_id, E_tok, bias_tok, vals, starts, lens, n_items, world, rank, c0, c1, out,
                                bias_out=bias_out, all_owners=all_owners, scale=scale, block_rows=block_rows)

    def shard_topk(self, U, E, bias, k, ex, values, indices, lse=None, tags=None, sample=None):
        """Recommend's local stage: values / indices [B, k] = every row's k best of U . E^T + bias over the shard's
        rows, by (value desc, local column asc); ex: exclusion lists (row_keys, key_rows, ex_ptr, ex_cols of local
        columns) or None.  The streaming top-k of StreamTopK (topk.TopKScan: fused filter GEMM, the chunked path
        after an overflow or for shapes the fused kernel does not take); a shard with fewer than k rows fills the rest
        with (-inf, -1).  lse [B] (optional): the log-sum-exp of every row's logits over ALL the shard's rows, excluded
        ones included (TopKScan's want_lse); -inf for a shard without rows.  tags (optional): (col_tags [V] int32 of
        the shard's rows, want_any, want_all, want_rows) -- only the rows eligible by their tag words enter a result
        (TopKScan.run).  sample (optional): the keyed sample of the sampled recommend (tau [B], B, seed_words,
        world, shard, the rows' global user ids: arx_sample_shard.h) -- the lists are then the k best KEYS, NOT
        stripped: the merge across shards compares keys.  Buffers and GEMM workspace are this stage's own (captured
        step graphs keep theirs)."""
        ops = self.ops
        B, V, d = int(U.shape[0]), int(E.shape[0]), int(U.shape[1])
        if getattr(self, 'ws_rec', None) is None:
            self.ws_rec, self._scans = ops.Workspace(U.device), {}
        if V < k:
            ops.fill_f32(values, float('-inf'))
            ops.fill_i32(indices, -1)
            if V == 0 or B == 0:
                if lse is not None and B:
                    ops.fill_f32(lse, float('-inf'))
                return
            kk = V
        else:
            kk = k
        key = (B, V, d, kk, lse is not None)
        scan = self._scans.get(key)
        if scan is None:
            if len(self._scans) > 8:
                self._scans.clear()
            scan = self._scans[key] = TopKScan(B, V, d, kk, U.device, want_lse=lse is not None)
            scan.fused = scan.fused and int(E.shape[1]) == d
            if kk < k:
                scan.short = (torch.empty((B, kk), dtype=torch.float32, device=U.device),
                              torch.empty((B, kk), dtype=torch.int32, device=U.device))
        vo, io = (values, indices) if kk == k else scan.short
        # (a candidate segment too short: this rank once more, chunked)
        if sample is None:
            run_complete(scan, lambda: scan.run(U, E, bias, self.ws_rec, vo, io, ex, tags=tags))
        else:
            run_complete(scan, lambda: scan.run(U, E, bias, self.ws_rec, vo, io, ex, tags=tags, sample=sample,
                                                strip=False))
        if kk < k:
            values[:, :kk].copy_(vo)
            indices[:, :kk].copy_(io)
        if lse is not None:
            lse.copy_(scan.lse)

    def shard_mass_parts(self, B, V, d):
        """The number of REST parts per row shard_rest_mass writes for a shard of V rows (every rank computes it for
        every shard: the packed rows are sized by the largest): the column ranges of the streaming mass pass where the
        fused scorer applies and the shard is past the first chunk, else the one running pair."""
        if V > 65536 and d in (32, 64, 128) and os.environ.get('ARX_TOPK_FUSED', '1') != '0':
            return self.ops.gemm_nt_topk_parts(B, V)
        return 1

    def _mass_bufs_of(self, B, k, device):
        """The mass pass's buffers of (B, k): (LogpBuffers, the picks as this shard's columns [B, k])."""
        lbs = self.__dict__.setdefault('_mass_bufs', {})
        lb = lbs.get((B, k))
        if lb is None:
            if len(lbs) > 8:
                lbs.clear()
            lb = lbs[(B, k)] = (LogpBuffers(B, k, device), torch.empty((B, k), dtype=torch.int32, device=device))
        return lb

    def shard_list_prepare(self, lists, n_items, world, shard, V, ex, tags, codes):
        """list_logprob's per-shard prepare (arx_list_logp_prepare_shard): lists [B, k] GLOBAL ids of ANY origin -> the
        reason codes this shard can give (codes int32 [B, k]; may be a view into the packed exchange buffer), and the
        surviving owned entries as this shard's sorted picks, in the buffers shard_rest_mass(prepared=) reads -- in
        place of arx_picks_to_shard + arx_sample_logp_sort.  V: the shard's rows; ex / tags: as shard_rest_mass takes
        them.  Returns the handle for shard_rest_mass(prepared=)."""
        B, k = int(lists.shape[0]), int(lists.shape[1])
        if V == 0 or B == 0:
            if B:
                codes.zero_()                          # (no entry in range is this shard's: nothing to say)
            return None
        lb, cols = self._mass_bufs_of(B, k, lists.device)
        self.ops.list_logp_prepare_shard(lists, n_items, world, shard, ex, tags, cols, codes, lb.pk_cols, lb.pk_slot)
        return lb, cols

    def list_logp_merge_shards(self, lists, n_items, codes, clean, why):
        """The owner's merge of list_logprob (arx_list_logp_merge_shards): lists [B_loc, k] global ids, codes
        [W, B_loc, k] -> why and the global clean list the finish reads."""
        self.ops.list_logp_merge_shards(lists, n_items, codes, clean, why)

    def list_logp_stamp(self, clean, values, why, logp):
        """After the finish over `clean`: NOSCORE where a clean entry's score (the finish's values) came out -inf, then
        logp = value = -inf at every code >= 2 (arx_list_logp_stamp)."""
        self.ops.list_logp_stamp(clean, values, why, logp, values)

    def shard_rest_mass(self, U, E, bias, ex, picks, world, shard, sample, packed, P_max, tags=None, prepared=None):
        """The propensities' local stage (arx_sample_logp.h's mass pass over ONE shard): picks [B, k] GLOBAL ids in
        selection order -> this shard's columns (arx_picks_to_shard), REST's mass of the shard's rows per request row,
        and the scores of the picks the shard owns.  packed float32 [B, 2 P_max + k]: columns [0, P_max) the m parts,
        [P_max, 2 P_max) the S parts -- past this shard's own parts the empty mass (-FLT_MAX, 0) --, the rest the pick
        scores, -inf where the shard does not own the pick.  prepared (list_logprob): the handle of shard_list_prepare
        over `picks` -- the shard's columns and their sorted form are already in place, everything after is shared."""
        ops = self.ops
        B, V, d, k = int(U.shape[0]), int(E.shape[0]), int(U.shape[1]), int(picks.shape[1])
        # (column blocks of the packed rows are strided views: filled as views, not as runs of numel() words)
        packed[:, :P_max].fill_(-3.4028234663852886e38)
        packed[:, P_max:2 * P_max].fill_(0.0)
        packed[:, 2 * P_max:].fill_(float('-inf'))
        if V == 0 or B == 0:
            return
        if getattr(self, 'ws_rec', None) is None:
            self.ws_rec, self._scans = ops.Workspace(U.device), {}
        if prepared is None:
            lb, cols = self._mass_bufs_of(B, k, U.device)
            ops.picks_to_shard(picks, world, shard, cols)
        else:
            lb, cols = prepared
        key = (B, V, d, 'mass')
        scan = self._scans.get(key)
        if scan is None:
            scan = self._scans[key] = TopKScan(B, V, d, 1, U.device)
            scan.fused = scan.fused and int(E.shape[1]) == d
        streaming = scan.mass_streams(U, E) and self.shard_mass_parts(B, V, d) > 1
        ops.fill_f32(lb.pick_score, float('-inf'))
        m, sp, P = scan.mass_pass(U, E, bias, self.ws_rec, cols, ex, tags, sample, streaming, lb,
                                  presorted=prepared is not None)
        if P > P_max:
            raise RuntimeError("shard_rest_mass: %d parts for rows of %d" % (P, P_max))
        packed[:, :P].copy_(m if m.dim() == 2 else m.view(B, 1))
        packed[:, P_max:P_max + P].copy_(sp if sp.dim() == 2 else sp.view(B, 1))
        packed[:, 2 * P_max:].copy_(lb.pick_score)

    def sample_strip(self, values, indices, sample):
        """The merged winners' keys back into scores at their owner (arx_topk_gumbel_strip_keyed over global ids)."""
        self.ops.topk_gumbel_strip(values, indices, sample)

    def sample_logp_finish_shards(self, indices, recv, P_max, sample, logp, values):
        """logp / exact values [B_loc, k] of the picks `indices` (global ids in selection order) from the W packed
        slabs recv [W, B_loc, >= 2 P_max + k] of shard_rest_mass (arx_sample_logp_finish_shards; list_logprob's rows
        carry k more words behind the pick scores)."""
        k = int(indices.shape[1])
        self.ops.sample_logp_finish_shards(indices, recv[:, :, 2 * P_max:2 * P_max + k], recv[:, :, :P_max],
                                           recv[:, :, P_max:2 * P_max], P_max, sample, logp, values)

    sim_chunk = 65536       # first-chunk width of shard_similar's TopKScan (tests narrow it to reach the fused kernel)

    def gather_rows_unit(self, E, rows, out):
        """out[r] = E[rows[r]] / |E[rows[r]]|; a zero row for rows[r] < 0 and for a zero row (arx_gather_rows_unit)."""
        self.ops.gather_rows_unit(E, rows, out)

    def shard_similar(self, Q, E, k, self_cols, values, indices):
        """similar_items' local stage: values / indices [B, k] = every row's k best cosines of the unit rows Q [B, d]
        with the shard's rows E [V, d], by (cosine desc, local column asc).  self_cols [B] int32 (None: keep them):
        the local column each row leaves out, anything outside [0, V) for a query of another shard.  The inverse norms
        of the shard are recomputed here (one read of it), then the streaming top-k with the cosine scale
        (topk.similar_scan); a shard with fewer than k rows -- or k rows and one left out -- fills the rest with
        (-inf, -1).  Buffers and GEMM workspace are this stage's own."""
        ops = self.ops
        B, V, d = int(Q.shape[0]), int(E.shape[0]), int(Q.shape[1])
        if getattr(self, 'ws_sim', None) is None:
            self.ws_sim, self._sim_scans = ops.Workspace(Q.device), {}
        if B == 0:
            return
        if V < k:
            ops.fill_f32(values, float('-inf'))
            ops.fill_i32(indices, -1)
            if V == 0:
                return
            kk = V
        else:
            kk = k
        key = (B, V, d, kk, self.sim_chunk)
        scan = self._sim_scans.get(key)
        if scan is None:
            if len(self._sim_scans) > 8:
                self._sim_scans.clear()
            scan = self._sim_scans[key] = TopKScan(B, V, d, kk, Q.device, chunk=self.sim_chunk)
            scan.fused = scan.fused and int(E.shape[1]) == d
            if kk < k:
                scan.short = (torch.empty((B, kk), dtype=torch.float32, device=Q.device),
                              torch.empty((B, kk), dtype=torch.int32, device=Q.device))
        vo, io = (values, indices) if kk == k else scan.short
        similar_scan(scan, E, Q, vo, io, self.ws_sim, self_cols is None, self_cols)
        if kk < k:
            values[:, :kk].copy_(vo)
            indices[:, :kk].copy_(io)

    def topk_merge_shards(self, v, c, vo, io):
        """[W, B, k] per-shard lists (local columns) -> [B, k] global ids (arx_topk_merge_shards)."""
        self.ops.topk_merge_shards(v, c, vo, io)

    def slate_scores(self, U, E, bias, local_cols, out):
        """score_items' local stage: out[r, j] = U[r] . E[c] + bias[c] for c = local_cols[r, j] in [0, rows of E),
        -inf (nothing read) for a slot of another shard or an empty one (arx_slate_scores)."""
        self.ops.slate_scores(U, E, bias, local_cols, out)

    def slate_merge_shards(self, parts, out):
        """[W, B, C] per-shard scores (-inf where the shard does not own the slot) -> [B, C] (arx_slate_merge_shards)."""
        self.ops.slate_merge_shards(parts, out)

    def slate_order(self, scores, cand, k, values, pos, ids):
        """The k best slots of every row by (score desc, slot asc) and their candidate ids (arx.slate.slate_order)."""
        _slate.slate_order(scores, cand, k, values, pos, ids)

    def shard_eval(self, U, E, bias, t, tcol, loss, ex, part, cnt):
        """Evaluation's local stage: per row of U [B, d], this shard's partial over the V rows of E (+ bias) -- 'ce':
        log sum exp of the logits (-inf when V = 0); 'warp': sum of relu(x - t + 1); 'warp_eval': that sum and cnt =
        #{x > t}, the row's target column tcol (local; out of range: on another shard) counted as (1, 0) -- with the
        masked columns of ex (row_keys, key_rows, ex_ptr, ex_cols of local columns; None: none) taken out again.
        part [B] float32, cnt [B] int32 ('warp_eval').  The fused eval GEMM (arx_gemm_nt_eval_parts / _rank_parts)
        where d is 32, 64 or 128; other widths score chunks of logits (ops.gemm + arx_eval_chunk_accum, or a
        log-sum-exp per chunk) and have no 'warp_eval'.  Then arx_eval_shard_reduce.  Buffers and GEMM workspace are
        this stage's own (captured step graphs keep theirs)."""
        ops = self.ops
        B, V, d = int(U.shape[0]), int(E.shape[0]), int(U.shape[1])
        if getattr(self, 'ws_eval', None) is None:
            self.ws_eval, self._ev = ops.Workspace(U.device), {}
        fused = (d in (32, 64, 128) and int(E.shape[1]) == d and U.stride(0) % 4 == 0 and E.stride(0) % 4 == 0
                 and U.data_ptr() % 16 == 0 and E.data_ptr() % 16 == 0)
        if loss == 'warp_eval' and not fused:
            raise NotImplementedError("evaluate(loss='warp_eval'): the rank counts come out of the fused eval GEMM "
                                      "only -- embedding widths 32, 64 and 128 (got %d)" % d)
        if B == 0:
            return
        parts = cparts = None
        if V > 0 and fused:
            npart = ops.gemm_nt_topk_parts(B, V)
            key = ('fused', B, npart)
            if key not in self._ev:
                if len(self._ev) > 8:
                    self._ev.clear()
                self._ev[key] = (torch.empty((B, npart), dtype=torch.float32, device=U.device),
                                 torch.empty((B, npart), dtype=torch.int32, device=U.device))
            parts, cparts = self._ev[key]
            if loss == 'ce':
                ops.gemm_nt_eval_parts(U, E, bias, None, parts, None)
            elif loss == 'warp':
                ops.gemm_nt_eval_parts(U, E, bias, t, None, parts)
            else:
                ops.gemm_nt_eval_rank_parts(U, E, bias, t, tcol, parts, cparts)
        elif V > 0:
            chunk = min(65536, V)
            nch = (V + chunk - 1) // chunk
            key = ('chunked', B, chunk, nch)
            if key not in self._ev:
                if len(self._ev) > 8:
                    self._ev.clear()
                self._ev[key] = (torch.empty((B, chunk), dtype=torch.float32, device=U.device),
                                 torch.empty((B, nch), dtype=torch.float32, device=U.device),
                                 torch.empty((B,), dtype=torch.float32, device=U.device))
            lg_buf, lse_parts, lse0 = self._ev[key]
            for c in range(nch):
                c0, c1 = c * chunk, min(V, (c + 1) * chunk)
                lg = lg_buf[:, :c1 - c0]
                ops.gemm(U, E[c0:c1], lg, self.ws_eval, transB=True, col_bias=bias[c0:c1] if bias is not None else None)
                if loss == 'ce':
                    ops.row_logsumexp(lg, lse0)
                    lse_parts[:, c].copy_(lse0)
                else:
                    ops.eval_chunk_accum(lg, t, 1, c == 0, lse0, None)
            parts = lse_parts if loss == 'ce' else lse0.view(B, 1)
        if cparts is not None and loss != 'warp_eval':
            cparts = None
        ops.eval_shard_reduce(loss, parts, cparts, U, E, bias, t, tcol, ex if loss != 'ce' else None, part,
                              cnt if loss == 'warp_eval' else None)

    def eval_merge_shards(self, loss, parts, cnts, t, out, cnt_out):
        """[W, B] per-shard partials -> per-row loss ('warp_eval': margin_rank, true_rank) (arx_eval_merge_shards)."""
        self.ops.eval_merge_shards(loss, parts, cnts, t, out, cnt_out)


PAIR_LOSSES = ('bpr', 'bpr-hinge')


class ShardedHMF(object):
    """id-only HMF with row-sharded tables.  Global ids everywhere in
    the API; `users` passed to step() must all be owned by this rank.

    loss: 'mw' (the default) or 'mce' -- the sampled losses over the shared pool, the same step with another loss
    kernel -- or a pair loss, 'bpr' / 'bpr-hinge' (exchange='rows' only): no pool, one negative per interaction, fed
    with the batch or drawn on the device (prepare_pair_negatives); _step_body_pair.

    A step is a body (named segments of kernels between the collectives) run by one driver (_run_step): as captured
    hipGraph segments on the product backend, kernel by kernel everywhere else (graphs=False, ARX_DIST_EAGER=1, the
    numpy double of the CPU tests) -- the same launches, padding and exchanges either way.  _step_body is the ONE body
    of the sampled-pool step with exchange='rows', for this class, ShardedW2V and ShardedHMFRepTokens: it scores "the
    scorer's input" and a subclass overrides what differs -- more blocks of the index vector, feeds and key entries
    (_step_blocks, _static_feeds, _key_more), the lookups and the K7 pass (_gather, _k7), the input and its gradient
    (_scorer_io, _input_fwd, _input_bwd), their exchanges (_send_input_rows, _return_input_grads), launches behind the
    apply segment and the entry of a step that is not a replay (_after_apply, _fresh_step).  The pair step
    (_step_body_pair) and ShardedHMFBags._step_body have other collectives and bodies of their own; all of them share
    the router (_route_requests over owner_order), the index feed (_index_feed) and the scorer call (_scorer_loss,
    _scorer_bwd).  exchange='logits' is a separate, eager-only step (_step_logits)."""

    loss_name, pair, n_draws = 'mw', False, 0          # (instances set their own; a serving view keeps these)

    def __init__(self, n_users, n_items, d, B_loc, S, learning_rate, rank, world, device,
                 backend=None, group=None, tables=None, seed=0, acc0=0.1, graphs=None, exchange='rows', loss='mw'):
        if S % 4 != 0 or d % 4 != 0:
            raise ValueError("n_sampled and d must be multiples of 4")
        if exchange not in ('rows', 'logits'):
            raise ValueError("exchange: 'rows' (gather the pool rows) or 'logits' (all-to-all of the logits)")
        if exchange == 'logits' and type(self) is not ShardedHMF:
            raise ValueError("exchange='logits' is the id-only step's alternative (ShardedHMF)")
        if loss not in ('mw', 'mce') + PAIR_LOSSES:
            raise ValueError("loss: 'mw', 'mce', 'bpr' or 'bpr-hinge', got %r" % (loss,))
        pair = loss in PAIR_LOSSES
        if pair and type(self) is not ShardedHMF:
            raise NotImplementedError("%s: loss=%r -- the pair losses are on the id-only ShardedHMF; the HET classes "
                                      "train 'mw' and 'mce'" % (type(self).__name__, loss))
        if pair and exchange == 'logits':
            raise ValueError("loss=%r has no pool to score: exchange='logits' moves pool logits (use 'rows')" % (loss,))
        self.loss_name, self.pair = loss, pair
        self.seed, self.n_draws = int(seed), 0              # the pair draw: keyed by (seed, rank, n_draws)
        self._neg_csr = None                                # (ptr, cols) of prepare_pair_negatives
        self._neg_tables = None                             # (ex_cum, cum) of a weighted draw, None: uniform
        # 'logits' (the exchange north_star words): the latents are all-gathered, every owner
        # scores the WHOLE batch against its pool block, the [B, S_g] partial logits cross by all_to_all, and their
        # gradients cross back -- _step_logits.  Eager launches (no graph segments).
        self.exchange = exchange
        if exchange == 'logits':
            graphs = False
        self.n_users, self.n_items, self.d = n_users, n_items, d
        # The shared pool is ONE draw over all items (prepare_train.py:7-17), so the number of pool items
        # a rank owns varies from draw to draw: the owned blocks travel padded to `cap` rows (the largest
        # owner count of the current pool, a multiple of 4; set_pool).  Sg = capacity of a block.
        self.B_loc, self.S, self.Sg = B_loc, S, S
        self.rank, self.world = rank, world
        self.B = B_loc * world
        self.device = torch.device(device)
        self.group = group
        self.be = backend if backend is not None else HipBackend(self.device)
        # (a backend that knows 'mw' alone -- the default -- is never handed a kind)
        self._loss_fused = self.be.loss_mw_fused_pos if loss == 'mw' else \
            (lambda *a: self.be.loss_mw_fused_pos(*a, kind=loss))
        # "this model captures graphs" (_run_step): the product backend on a GPU, unless switched off -- otherwise the
        # same step body runs kernel by kernel on the caller's stream
        if graphs is None:
            graphs = not os.environ.get("ARX_DIST_EAGER")
        self.use_graphs = bool(graphs) and isinstance(self.be, HipBackend) and self.device.type == 'cuda'
        self._graphs, self._graph_key, self._warm_key, self.g_idx = {}, None, None, None
        self.n_captures, self.n_replays = 0, 0
        # (the legacy default stream cannot be captured: the step runs on a stream of its own, joined with
        # the caller's stream on both sides)
        self._stream = torch.cuda.Stream(device=self.device) if self.use_graphs else None
        self._side = torch.cuda.Stream(device=self.device) if self.use_graphs else None
        dev = self.device
        f32, i32 = torch.float32, torch.int32
        nu = (n_users - rank + world - 1) // world        # owned rows
        ni = (n_items - rank + world - 1) // world
        self.nu_loc, self.ni_loc = nu, ni
        self.zero_row = ni                                 # padding row of the item shard
        if tables is not None:                             # explicit global tables (tests)
            U = np.asarray(tables['user'], dtype=np.float32)[rank::world]
            I = np.asarray(tables['item'], dtype=np.float32)[rank::world]
            bI = np.asarray(tables['item_bias'], dtype=np.float32).reshape(-1)[rank::world]
            self.E_user = torch.from_numpy(np.ascontiguousarray(U)).to(dev)
            self.E_item = torch.zeros((ni + 1, d), dtype=f32, device=dev)
            self.E_item[:ni].copy_(torch.from_numpy(np.ascontiguousarray(I)))
            self.b_item = torch.zeros((ni + 1,), dtype=f32, device=dev)
            self.b_item[:ni].copy_(torch.from_numpy(np.ascontiguousarray(bI)))
        else:
            g = torch.Generator(device=dev)
            g.manual_seed(seed * 1009 + rank)
            lim_u = float(np.sqrt(6.0 / (n_users + 2 + d)))
            lim_i = float(np.sqrt(6.0 / (n_items + 2 + d)))
            self.E_user = torch.empty((nu, d), dtype=f32, device=dev).uniform_(-lim_u, lim_u, generator=g)
            self.E_item = torch.empty((ni + 1, d), dtype=f32, device=dev).uniform_(-lim_i, lim_i, generator=g)
            self.E_item[ni].zero_()
            self.b_item = torch.empty((ni + 1,), dtype=f32, device=dev).uniform_(-lim_i, lim_i, generator=g)
            self.b_item[ni] = 0.0
        self.acc0 = float(acc0)
        self.A_user = torch.full_like(self.E_user, acc0)
        self.A_item = torch.full_like(self.E_item, acc0)
        self.Ab_item = torch.full_like(self.b_item, acc0)
        self.lr = torch.tensor([float(learning_rate)], dtype=f32, device=dev)
        # save / restore (collectives; utils/checkpoint.py ShardedSaver): per-rank files of the owned rows, restorable
        # on another world size.  n_restores: what a serving view compares beside `steps` (a restore may land on the
        # step count the view has seen)
        from .utils.checkpoint import ShardedSaver
        self.saver = ShardedSaver(self)
        self.n_restores = 0

        Sg, W = self.Sg, world
        dp = d + 4                                          # packed row: d values + bias (+ pad)
        self.dp = dp
        z = lambda *s: torch.zeros(s, dtype=f32, device=dev)
        zi = lambda *s: torch.zeros(s, dtype=i32, device=dev)
        self.urows = zi(B_loc)
        self.U_loc = z(B_loc, d)
        self.bl, self.loss = z(B_loc), z(1)
        self.steps = 0
        self.cap_r = 0                                      # capacity for received target rows
        if pair:
            # no pool and nothing sized by it (S may be 0; Sg = 0 lays the K7 arena out as [dU ; received rows]);
            # an interaction asks for TWO rows: the received block and its gradient block hold 2 B_loc packed rows
            self.S = self.Sg = 0
            self.cap = 0
            self.R_pack, self.dR_pack = z(2 * B_loc, dp), z(2 * B_loc, dp)
            self.pos_score, self.neg_score = z(B_loc), z(B_loc)
            self.auc_counts, self.g_slots = zi(2), zi(2 * B_loc)
            self._alloc_recv(2 * B_loc)
            self.pos_ptr, self.pos_items = zi(nu + 2), zi(1)
            return
        self.pool_ids = zi(S)                               # owner-major global ids
        self.pool_rows = zi(Sg)                             # local rows of the owned block (padding row behind it)
        self.cap = S if world == 1 else 0                   # rows of a block in the current exchange
        self.gidx = zi(S)                                   # pool slot -> row of the gathered blocks
        self.my_slots = zi(S)                               # block row -> pool slot (S: none, a zero row)
        self.I_gath = z(world * S, dp) if world > 1 else None
        self.pool_old = None
        self.item2slot = torch.full((n_items + 1,), -1, dtype=i32, device=dev)
        if hasattr(self.be, 'attach_pool_bitmap'):          # (1 bit per item in front of the map: HIP backend)
            self._pool_bits = torch.zeros((n_items + 1 + 32) // 32, dtype=i32, device=dev)
            self.be.attach_pool_bitmap(self.item2slot, self._pool_bits)
        self.I_pack, self.b_g = z(Sg, dp), z(Sg)            # owned pool rows | bias in column d
        self.I_all, self.b_all = z(S, dp), z(S)             # gathered pool
        self.logits = z(B_loc, S)
        self.T_pack, self.tb = z(B_loc, dp), z(B_loc)       # target rows as received back
        self.t_loc, self.dt_loc = z(B_loc), z(B_loc)
        self.dlogits = z(B_loc, S)
        self.dI_all, self.gb_all = z(S + 1, dp), z(S)       # pool-gradient partials (all columns) + a zero row
        self.dT_pack = z(B_loc, dp)                         # target-row gradients to send
        self._alloc_recv(B_loc)
        self.pos_ptr = zi(nu + 2)
        self.pos_items = zi(1)

    def _alloc_recv(self, cap):
        """Buffers that scale with R = target rows this rank owns in a batch.  The gradient
        arena holds [dU_loc (B_loc) ; dI_g (Sg) ; received dT (R)] so that both tables are
        updated by ONE fused sparse-Adagrad pass."""
        if cap <= self.cap_r:
            return
        dev, f32, i32 = self.device, torch.float32, torch.int32
        B_loc, Sg, dp = self.B_loc, self.Sg, self.dp
        if self.use_graphs and self.cap_r > 0:
            cap = (cap + cap // 8 + 63) // 64 * 64        # new buffers = new graphs: grow with slack
        self.cap_r = cap
        self.recv_ids = torch.zeros((cap,), dtype=i32, device=dev)
        self.recv_rows = torch.zeros((cap,), dtype=i32, device=dev)
        self.T_send = torch.zeros((cap, dp), dtype=f32, device=dev)
        self.tb_send = torch.zeros((cap,), dtype=f32, device=dev)
        self.arena = torch.zeros((B_loc + Sg + cap, dp), dtype=f32, device=dev)
        self.arena_b = torch.zeros((B_loc + Sg + cap,), dtype=f32, device=dev)

    # ------------------------------------------------------------------ state
    def set_positives(self, ptr_local, items_global):
        """CSR over this rank's LOCAL user rows; item ids are global."""
        dev = self.device
        self.pos_ptr = torch.as_tensor(np.asarray(ptr_local, dtype=np.int32)).to(dev) \
            if not isinstance(ptr_local, torch.Tensor) else ptr_local.to(dev, torch.int32)
        it = items_global if isinstance(items_global, torch.Tensor) else \
            torch.as_tensor(np.asarray(items_global, dtype=np.int32))
        self.pos_items = it.to(dev, torch.int32)

    def set_pool(self, pool_ids):
        """The shared negative pool, global item ids in slot order -- any owners (one draw over all
        items: embed_attribute.py:320-348 update_sampled, sharded).  Every rank sees the same ids and
        derives the same block layout: owner g's pool items, in slot order, are rows [0, count_g) of
        its block; all blocks travel padded to cap = max_g count_g rows."""
        if self.pair:
            raise RuntimeError("set_pool: a %r model has no pool (its negatives come with the batch: prepare_route)"
                               % self.loss_name)
        be = self.be
        new = pool_ids if isinstance(pool_ids, torch.Tensor) else \
            torch.as_tensor(np.asarray(pool_ids, dtype=np.int32))
        new = new.to(self.device, torch.int32)
        if self.pool_old is not None:
            be.slot_map_set(self.item2slot, self.pool_old, True)
        else:
            self.pool_old = torch.empty_like(self.pool_ids)
        be.copy_i32(new, self.pool_ids)
        be.copy_i32(new, self.pool_old)
        be.slot_map_set(self.item2slot, self.pool_ids, False)
        W, r, S = self.world, self.rank, self.S
        if W == 1:
            be.shard_route(self.pool_ids, W, r, self.zero_row, self.pool_rows, None)
            if self.exchange == 'logits':
                self._logits_layout(np.arange(S, dtype=np.int32))
            return
        # block layout (redraw path, every n_resample steps): two launches of arx_pool_blocks around ONE host
        # read of the W owner counts (the block capacity is a host decision: it sizes the exchanges)
        if getattr(self, '_pool_counts', None) is None:
            self._pool_counts = torch.zeros(W + 1, dtype=torch.int32, device=self.device)   # [W] = negative ids
        be.pool_blocks(self.pool_ids, W, r, self.zero_row, 0, self._pool_counts)
        cnts = self._pool_counts.cpu().tolist()
        if cnts[W] != 0:
            raise ValueError("set_pool: %d negative item id(s) in the pool (a short draw of the device sampler "
                             "leaves -1: redraw or pass valid ids)" % cnts[W])
        cap = (max(cnts[:W]) + 3) // 4 * 4
        if self.use_graphs:      # block capacity only grows (a new capacity = new graphs), with slack
            cap = self.cap if cap <= self.cap else min(S, (cap + cap // 8 + 15) // 16 * 16)
        self.cap = cap
        be.pool_blocks(self.pool_ids, W, r, self.zero_row, cap, self._pool_counts, self.gidx, self.my_slots,
                       self.pool_rows)
        if self.exchange == 'logits':
            self._logits_layout(self.gidx.cpu().numpy())

    def _logits_layout(self, gidx):
        """Buffers and the inverse block map of the logits exchange, per pool draw (host; the redraw path):
        blk2slot[g * cap + j] = pool slot of row j of owner g's block (S = padding: a zero row), the order
        in which the gradient rows of the transposed logits are sent back to the owners."""
        W, S, cap, B_loc, dp = self.world, self.S, self.cap, self.B_loc, self.dp
        inv = np.full(W * cap, S, dtype=np.int32)
        inv[np.asarray(gidx, dtype=np.int64)] = np.arange(S, dtype=np.int32)
        self.blk2slot = torch.from_numpy(inv).to(self.device)
        if W == 1:
            self.gidx = torch.arange(S, dtype=torch.int32, device=self.device)
        if getattr(self, '_lg_cap', -1) != cap:
            z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.device)
            self._lg_cap = cap
            self.U_aug = z(B_loc, dp)                  # [U | 1 | 0 0 0]: the bias column of the packed pool rows
            self.U_aug[:, self.d] = 1.0                # rides through the scorer GEMM
            self.U_all = z(W * B_loc, dp)
            self.Pt_send, self.Pt_recv = z(W * cap, B_loc), z(W * cap, B_loc)    # [owner | dest][block row][batch row]
            self.logitsT, self.dlogitsT = z(S, B_loc), z(S + 1, B_loc)           # (+ a zero row for the padding)
            self.dPt_send, self.dPt_recv = z(W * cap, B_loc), z(W * cap, B_loc)
            self.dI_blk = z(cap, dp)
            self.dU_part = z(W * B_loc, self.d)
            self.dU_red = z(B_loc, self.d)

    # ------------------------------------------------------------------ route
    def prepare_pair_negatives(self, seed=None, power=None, smooth=1.0, counts=None):
        """Makes this rank's set_positives lists the exclusion lists of the pair draw (prepare_route without
        neg_items): checks the ids, sorts every user's list and drops its duplicates -- the rank-select draw
        (arx_neg_draw_uniform) needs sorted, unique lists.  The lists set_positives holds stay as they are.
        seed: the draw's seed (default: the constructor's); the draw counter starts again only with a new seed.
        power None: the draw is uniform over the items outside the list.  A number: in proportion to (counts +
        smooth) ** power (arx_neg_draw_weighted) -- counts int [n_items] per global item id, the same on every rank;
        by default the number of users of ALL ranks whose list holds the item (one all-reduce of n_items int64 over
        the model's group: a collective, every rank calls with power set).  The prefix sums of the weights are
        replicated: 8 bytes per item and 8 bytes per local history entry on every rank."""
        if not self.pair:
            raise RuntimeError("prepare_pair_negatives: a %r model draws no negatives" % self.loss_name)
        ptr = self.pos_ptr.cpu().numpy().astype(np.int64)
        items = self.pos_items.cpu().numpy().astype(np.int64)
        if len(ptr) < 2 or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] > len(items):
            raise ValueError("prepare_pair_negatives: set_positives' ptr must start at 0, not decrease and end "
                             "within the items")
        items = items[:ptr[-1]]
        if len(items) and (items.min() < 0 or items.max() >= self.n_items):
            raise ValueError("prepare_pair_negatives: item ids must lie in [0, %d)" % self.n_items)
        row = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
        o = np.lexsort((items, row))
        row, items = row[o], items[o]
        if len(items):
            keep = np.ones(len(items), dtype=bool)
            keep[1:] = (row[1:] != row[:-1]) | (items[1:] != items[:-1])
            row, items = row[keep], items[keep]
        nptr = np.zeros(len(ptr), dtype=np.int64)
        np.cumsum(np.bincount(row, minlength=len(ptr) - 1), out=nptr[1:])
        if len(items) == 0:
            items = np.zeros(1, dtype=np.int64)             # (a valid device pointer; every list is empty)
        tables = None
        if power is not None:
            if counts is None:
                cnt = torch.from_numpy(np.bincount(items[:nptr[-1]], minlength=self.n_items).astype(np.int64))
                if self.world > 1:
                    cnt = cnt.to(self.device)
                    dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=self.group)
                counts = cnt.cpu().numpy()
            counts = np.asarray(counts).reshape(-1)
            if len(counts) != self.n_items:
                raise ValueError("prepare_pair_negatives: counts holds one entry per item (%d, not %d)"
                                 % (self.n_items, len(counts)))
            cum, ex_cum = pair_draw_tables(counts, power, smooth, nptr, items)
            tables = (torch.from_numpy(ex_cum).to(self.device), torch.from_numpy(cum).to(self.device))
        self._neg_tables = tables
        self._neg_csr = (torch.from_numpy(nptr.astype(np.int32)).to(self.device),
                         torch.from_numpy(items.astype(np.int32)).to(self.device))
        if seed is not None and int(seed) != self.seed:
            self.seed, self.n_draws = int(seed), 0

    def _prepare_route_pair(self, users, items, neg_items):
        """The loader side of a pair step.  An interaction asks for TWO item rows -- its positive and its negative,
        owners unrelated -- so the received rows cannot be lined up with the batch rows by sorting the batch: the
        2 B_loc requests (positives, then negatives; a void row asks for no negative) are ordered by owner, the
        packed rows come back in that order, and every batch row is told the SLOT of its positive and of its
        negative row in the received block (neg_slot -1: void).  Every slot belongs to one request: an item asked for
        twice travels twice and K7 merges its gradient rows.  The batch itself keeps the caller's order.
        neg_items None: one negative per row is drawn here, on the device, from the lists of
        prepare_pair_negatives -- here and not inside the captured step because the variable-size exchange needs
        the per-owner counts on the host."""
        W, B_loc, dev = self.world, self.B_loc, self.device
        u = users.cpu().numpy() if isinstance(users, torch.Tensor) else np.asarray(users)
        it = items.cpu().numpy() if isinstance(items, torch.Tensor) else np.asarray(items)
        u, it = u.astype(np.int32).reshape(-1), it.astype(np.int32).reshape(-1)
        if len(u) != B_loc or len(it) != B_loc:
            raise ValueError("prepare_route: B_loc = %d users and items per rank" % B_loc)
        if len(it) and (it.min() < 0 or it.max() >= self.n_items):
            raise ValueError("prepare_route: item ids must lie in [0, %d)" % self.n_items)
        users_d = torch.from_numpy(np.ascontiguousarray(u)).to(dev)
        urows = torch.zeros((B_loc,), dtype=torch.int32, device=dev)
        self.be.shard_route(users_d, W, self.rank, 0, urows, None)         # all owned: local rows
        if neg_items is None:
            if self._neg_csr is None:
                raise RuntimeError("prepare_route without neg_items draws the negatives: call "
                                   "prepare_pair_negatives() first (after set_positives)")
            drawn = torch.zeros((B_loc,), dtype=torch.int32, device=dev)
            if self._neg_tables is None:
                self.be.neg_draw_uniform(urows, self._neg_csr[0], self._neg_csr[1], self.n_items,
                                         self.seed * 1000003 + self.rank, self.n_draws, drawn)
            else:
                self.be.neg_draw_weighted(urows, self._neg_csr[0], self._neg_csr[1], self._neg_tables[0],
                                          self._neg_tables[1], self.n_items, self.seed * 1000003 + self.rank,
                                          self.n_draws, drawn)
            self.n_draws += 1
            ng = drawn.cpu().numpy().astype(np.int32)
        else:
            ng = neg_items.cpu().numpy() if isinstance(neg_items, torch.Tensor) else np.asarray(neg_items)
            ng = ng.astype(np.int32).reshape(-1)
            if len(ng) != B_loc:
                raise ValueError("prepare_route: one negative per interaction (%d for %d)" % (len(ng), B_loc))
            if ng.max(initial=-1) >= self.n_items:
                raise ValueError("prepare_route: negative ids must lie below %d (< 0: a void row)" % self.n_items)
        live = ng >= 0
        req = np.concatenate([it, ng[live]])                                # the requests: positives, live negatives
        route, slot = self._route_requests(req)[:2]                         # request -> its row of the received block
        neg_slot = np.full(B_loc, -1, dtype=np.int32)
        neg_slot[np.nonzero(live)[0]] = slot[B_loc:]
        self._alloc_recv(route['R'])
        route.update(users=users_d, items=torch.from_numpy(np.ascontiguousarray(it)).to(dev),
                     neg_items=torch.from_numpy(np.ascontiguousarray(ng)).to(dev),
                     slots=torch.from_numpy(np.concatenate([slot[:B_loc], neg_slot])).to(dev), n_req=int(len(req)),
                     urows=urows)
        return route

    def _count_exchange(self, send):
        """send[g] = what this rank sends to rank g (int64 [world], host) -> what it receives from every rank: one
        tiny all_to_all."""
        st = torch.from_numpy(send).to(self.device)
        rt = torch.empty_like(st)
        _all_to_all(rt, st, group=self.group)
        return [int(v) for v in rt.cpu().tolist()]

    def _route_requests(self, req):
        """The router of every variable-size exchange: the requests req (int32 global item ids, host) are ordered by
        owner (owner_order), the counts cross, then the ids, and every owner resolves the ids it received to rows of
        its shard.  Two collectives, in this order.  Returns ({send, recv: the split sizes; R: rows this rank serves;
        recv_ids, recv_rows: what it serves, as ids and as local rows (device)}, slots (host: request -> its row of
        the block that comes back), perm (host), the requests in the order they were sent (device))."""
        W, dev = self.world, self.device
        perm, slot, send = owner_order(req, W)
        recv = self._count_exchange(send)
        send = [int(v) for v in send.tolist()]
        R = int(sum(recv))
        ids = torch.from_numpy(np.ascontiguousarray(req[perm])).to(dev)
        recv_ids = torch.zeros((R,), dtype=torch.int32, device=dev)
        _all_to_all(recv_ids, ids, recv, send, group=self.group)
        recv_rows = torch.zeros((R,), dtype=torch.int32, device=dev)
        if R > 0:
            self.be.shard_route(recv_ids, W, self.rank, self.zero_row, recv_rows, None)
        return {'send': send, 'recv': recv, 'R': R, 'recv_ids': recv_ids, 'recv_rows': recv_rows}, slot, perm, ids

    def prepare_route(self, users, items, neg_items=None):
        """Data-loader side of a batch (host): orders the interactions by the owner of their
        target item and returns what the variable-size exchanges need.  One tiny all_to_all
        of the per-destination counts (not on the step path).  A pair model ('bpr' / 'bpr-hinge') routes two rows per
        interaction, the negatives fed (neg_items; < 0: a void row) or drawn: _prepare_route_pair."""
        if self.pair:
            return self._prepare_route_pair(users, items, neg_items)
        if neg_items is not None:
            raise ValueError("prepare_route: neg_items belong to the pair losses, this model trains %r"
                             % self.loss_name)
        W = self.world
        u = users.cpu().numpy() if isinstance(users, torch.Tensor) else np.asarray(users)
        it = items.cpu().numpy() if isinstance(items, torch.Tensor) else np.asarray(items)
        # The ids themselves are routed here too (they are input data, like the owner ordering): every owner learns
        # which of its rows this batch asks for, and the local row of every id is resolved once.  The step path then
        # starts at the table lookups.
        route, _, perm, items_d = self._route_requests(it.astype(np.int32))
        self._alloc_recv(route['R'])
        users_d = torch.from_numpy(np.ascontiguousarray(u.astype(np.int32)[perm])).to(self.device)
        urows = torch.zeros((self.B_loc,), dtype=torch.int32, device=self.device)
        self.be.shard_route(users_d, W, self.rank, 0, urows, None)          # all owned: local rows
        route.update(users=users_d, items=items_d, urows=urows)
        return route

    # ------------------------------------------------------------------- step
    def step(self, users, items=None, neg_items=None):
        """One training step.  `users` is either a route from prepare_route() (the fast way:
        nothing but kernels and collectives on the step path) or a users array with `items`
        (routed here on the host; a pair model: with neg_items too, or drawn)."""
        if self.world > 1 and self.cap <= 0 and not self.pair:
            raise RuntimeError("%s.step before set_pool(): the pool's block layout sizes the exchanges"
                               % type(self).__name__)
        if isinstance(users, dict):
            route = users
        elif self.pair:
            route = self.prepare_route(users, items, neg_items)
        else:
            route = self.prepare_route(users, items)
        if self.exchange == 'logits':
            return self._step_logits(route)
        self._run_step(route)

    def _step_logits(self, route):
        """The step with the exchange north_star words (hmf_model.py:52-99 on the global
        batch, embed_attribute.py:148-206 scorer, :641-649 'mw'): the [B, S] logits are computed WHERE THE POOL
        ROWS LIVE and cross xGMI, instead of the pool rows travelling to the batch rows.

          all_gather      latents [B_loc, d+4] -> [B, d+4]                      (column d = 1: carries the pool bias)
          (local)         Pt[h] = I_g . U_h^T  [cap, B_loc] for every destination h (owned pool block, padded to cap)
          all_to_all      Pt blocks -> rank h holds [W . cap, B_loc] = its rows against every owner's block
          (local)         block rows -> pool slots (gather), transpose -> logits [B_loc, S]; target rows as in step();
                          WMRB loss, dlogits; transpose, slots -> block rows (gather; padding reads a zero row)
          all_to_all      dlogits^T blocks back -> owner g holds dP^T [W][cap, B_loc]
          (local)         dI_g = sum_h dP_h^T-blocks . U_h  (column d: the bias gradient), dU partials for ALL B rows
          reduce_scatter  dU partials [B, d] -> [B_loc, d]
          (local)         the same fused scatter + Adagrad pass as step()

        Bytes per rank and step: 2 . (W-1)/W . B_loc . W . cap . 4 for the logits (cap ~ S / W: ~2 . B_loc . S . 4)
        + 2 . B . (d+4) . 4 for the latents, against 2 . B_loc . (d+4) . 4 + ~2 . S . (d+4) . 4 for the 'rows'
        exchange: it pays when S . (d+4) > B_loc . S, i.e. B_loc < d + 4 -- small batches against huge pools.  The
        product default stays 'rows'; this form is kept measured and tested (tests/test_dist_cpu.py, test_dist_gpu.py)."""
        be, W = self.be, self.world
        B, B_loc, S, Sg, d, dp, cap = self.B, self.B_loc, self.S, self.Sg, self.d, self.dp, self.cap
        grp = self.group
        send, recv, R = route['send'], route['recv'], route['R']
        arena, arena_b = self.arena, self.arena_b
        urows, recv_rows = route['urows'], route['recv_rows']
        self.urows = urows
        # ---- forward ----
        be.gather_rows(self.E_user, None, urows, self.U_aug[:, :d], None)
        be.copy_2d(self.U_aug[:, :d], self.U_loc)
        if W == 1:
            be.copy_2d(self.U_aug, self.U_all)
        else:
            dist.all_gather_into_tensor(self.U_all, self.U_aug, group=grp)
        be.gather_rows_packed(self.E_item, self.b_item, self.pool_rows[:cap], self.I_pack[:cap])
        T_send = self.T_send[:R]
        if R > 0:
            be.gather_rows_packed(self.E_item, self.b_item, recv_rows, T_send)
        w_rows = _all_to_all(self.T_pack, T_send, send, recv, group=grp, async_op=True)   # target rows back ...
        for h in range(W):                                                                 # ... under the scorer
            be.gemm(self.I_pack[:cap], self.U_all[h * B_loc:(h + 1) * B_loc], self.Pt_send[h * cap:(h + 1) * cap],
                    transB=True)
        if W == 1:
            Pt = self.Pt_send
        else:
            _all_to_all(self.Pt_recv, self.Pt_send, group=grp)
            Pt = self.Pt_recv
        be.gather_rows_wide(Pt, self.gidx, self.logitsT)                 # block rows -> pool slots
        be.transpose(self.logitsT, self.logits)
        w_rows.wait()
        dU = arena[:B_loc, :d]
        self._scorer_loss(False, self.U_loc, None, self.urows, self.dT_pack[:, d], dU, self.dT_pack[:, :d])
        # ---- backward ----
        w_dt = _all_to_all(arena[B_loc + Sg:B_loc + Sg + R], self.dT_pack, recv, send, group=grp, async_op=True)
        be.transpose(self.dlogits, self.dlogitsT[:S])
        be.gather_rows_wide(self.dlogitsT, self.blk2slot, self.dPt_send)  # slots -> block rows of every owner
        if W == 1:
            dPt = self.dPt_send
        else:
            _all_to_all(self.dPt_recv, self.dPt_send, group=grp)
            dPt = self.dPt_recv
        for h in range(W):
            blk, Uh = dPt[h * cap:(h + 1) * cap], self.U_all[h * B_loc:(h + 1) * B_loc]
            be.gemm(blk, Uh, self.dI_blk, beta=0.0 if h == 0 else 1.0)           # [cap, d+4]: column d = bias gradient
            be.gemm(blk, self.I_pack[:cap, :d], self.dU_part[h * B_loc:(h + 1) * B_loc], transA=True)
        if W == 1:
            be.copy_2d(self.dU_part, self.dU_red)
        else:
            _reduce_scatter(self.dU_red, self.dU_part, group=grp)
        be.add_2d(self.dU_red, dU)                                                # dU = dt . T (loss kernel) + dL . pool
        be.copy_2d(self.dI_blk, arena[B_loc:B_loc + cap])
        w_dt.wait()
        be.copy_strided(arena[B_loc:B_loc + Sg + R, d], arena_b[B_loc:B_loc + Sg + R])
        sites = [(0, self.urows, 0), (1, self.pool_rows[:cap], B_loc)]
        if R > 0:
            sites.append((1, recv_rows, B_loc + Sg))
        be.sparse_adagrad_multi([(self.E_user, self.A_user, None, None),
                                 (self.E_item, self.A_item, self.b_item, self.Ab_item)],
                                sites, arena[:, :d], arena_b, self.lr)
        self.steps += 1

    def _fused_scorer(self):
        """True when the step takes the bf16-pipe scorer (switches on, shapes it supports); allocates its buffers."""
        ops_ = getattr(self.be, 'ops', None)          # (the numpy test double has no kernels to pick from)
        if ops_ is None:
            return False
        # 'mce': the same surface (MceScorer: fwd() writes the COMPLETE latent gradient, bwd_dU(beta=1) adds nothing)
        mce = self.loss_name == 'mce'
        if not (ops_.mce_scorer_supported if mce else ops_.mw_scorer_supported)(self.B_loc, self.S, self.d):
            return False
        if getattr(self, 'scorer', None) is None:
            self.scorer = (ops_.MceScorer if mce else ops_.MwScorer)(self.B_loc, self.S, self.d, self.device)
        return True

    @property
    def stream(self):
        """The stream the graph-segment step runs on (None: no captured graphs, the caller's stream).  A training loop
        that makes it the current stream (`with torch.cuda.stream(model.stream)`) saves the two stream
        joins per step that a caller on another stream pays."""
        return self._stream

    # ------------------------------------------------ step: one body per class, one driver
    def _run_step(self, route):
        """Driver of the step of all three classes: the class's _step_body(route) gives the graph key and the body --
        kernels grouped into named segments between the collectives -- and this runs it.  A model that captures
        graphs (use_graphs) works on its own stream, joined with the caller's on both sides (the legacy default
        stream cannot be captured): a configuration (the key: capacities and buffer addresses) runs eagerly once
        (module loads, workspaces), is captured on its second step and replayed from then on;
        ARX_DIST_NO_CAPTURE=1 keeps it eager (profiling: the same launches, kernel by kernel).  Any other model
        (graphs=False / ARX_DIST_EAGER=1, a backend without kernels, a CPU device) runs the same body eagerly on the
        caller's stream, K7's sort half in line.  A step that raises leaves no captured graph behind: the next one
        runs eagerly again."""
        with _ops.joined(self._stream if self.use_graphs else None):
            self._run_step_here(route)

    def _run_step_here(self, route):
        try:
            key, body = self._step_body(route)
            if not self.use_graphs or os.environ.get("ARX_DIST_NO_CAPTURE"):
                mode = 'eager'
            elif self._graph_key == key:
                mode = 'replay'
            elif self._warm_key == key:
                mode, self._graphs = 'capture', {}
            else:
                mode, self._graphs, self._graph_key = 'eager', {}, None
            if mode != 'replay':
                self._fresh_step()
            body(mode)
        except BaseException:
            self._graphs, self._graph_key, self._warm_key = {}, None, None
            raise
        if mode == 'eager':
            self._warm_key = key
        elif mode == 'capture':
            self._graph_key = key
            self.n_captures += 1
        else:
            self.n_replays += 1
        self.steps += 1

    def _segment(self, mode, name, fn, feeds=None):
        """eager: run; capture: record the launches of `fn` into a hipGraph, keep it, launch it;
        replay: launch the kept graph.  feeds ([(src, dst)], the step's first segment): the copy of the batch's
        index vectors is the graph's first node, its source replaced before every replay
        (ops.CapturedGraph.replay)."""
        be = self.be
        if mode == 'eager':
            if feeds:
                be.copy_words(feeds)
            fn()
        elif mode == 'capture':
            self._graphs[name] = g = be.ops.CapturedGraph.record(fn, feeds)
            g.launch()
        else:
            self._graphs[name].replay(feeds)

    def _k7_sorts(self, mode, k7, own_graph):
        """k7(K7_SORT) -- K7's keys, sorts and run records, which need the ids only -- on the second stream, under the
        forward kernels (the ~70 us chain leaves the critical path): a graph of its own between the segments
        (own_graph), or a branch of the one graph at world 1.  Returns what _k7_join waits for before the apply half.
        A model without a second stream runs it in line."""
        if self._side is None:
            k7(_ops.K7_SORT)
            return None
        main, side = torch.cuda.current_stream(self.device), self._side
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)
        with torch.cuda.stream(side):
            if own_graph:
                self._segment(mode, 'k7_sorts', lambda: k7(_ops.K7_SORT))
            else:
                k7(_ops.K7_SORT)
            done = torch.cuda.Event()
            done.record(side)
        return done

    def _k7_join(self, done):
        if done is not None:
            torch.cuda.current_stream(self.device).wait_event(done)

    def _step_body(self, route):
        """The ONE body of the sampled-pool step ('mw' / 'mce', exchange='rows') of ShardedHMF, ShardedW2V and
        ShardedHMFRepTokens, with every buffer at a fixed address and a fixed size, so that the kernels between two
        collectives are ONE hipGraph launch each (5 segments + K7's sort half as a sixth, on a second stream under
        the forward kernels + 4 collectives per step instead of ~35 kernel launches from Python; world 1: ONE graph,
        the sort half a branch of it).  What varies from batch to batch is the index vector [user rows ; received
        target rows], padded with the shard's padding row to the capacity cap_r (gathers: a zero row; K7: the tables
        are passed without the padding row, so padded keys are out of range and dropped) and fed by the first node
        of the first segment, and the split sizes of the two all-to-alls, which stay outside the graphs.  The two
        large exchanges (target rows out, target-row gradients back: B_loc x (d+4) floats each) are issued
        asynchronously and waited for only where their result is needed, so that they travel under the scorer and
        under the two backward GEMMs.  Returns (graph key, body(mode)) for _run_step.

        The body scores "the scorer's input" X and writes its gradient dX; a subclass supplies what differs by
        overriding (the defaults are the id-only step):
          _step_blocks, _static_feeds, _key_more   more blocks of the index vector, more feeds, more key entries
          _gather, _k7                             the lookups of fwd_gather, the fused scatter + Adagrad pass
          _scorer_io, _input_fwd, _input_bwd       X / dX (U_loc / the arena's user rows), X formed at the head of
                                                   fwd_score, dX consumed at the tail of bwd_gemms
          _send_input_rows, _return_input_grads    the exchanges of a model whose input has rows on other ranks
          _after_apply, _fresh_step                launches behind the apply segment; a step that is not a replay"""
        if self.pair:
            return self._step_body_pair(route)
        be, W = self.be, self.world
        B_loc, S, Sg, d = self.B_loc, self.S, self.Sg, self.d
        grp = self.group
        send, recv, R = route['send'], route['recv'], route['R']
        feed = self._index_feed(route, self._step_blocks(route))
        cap, cap_r = self.cap, self.cap_r
        feed += self._static_feeds(route, cap_r)       # (subclasses: more per-batch index vectors)
        key = (cap, cap_r, self.g_idx.data_ptr(), self.arena.data_ptr(), self.pos_ptr.data_ptr(),
               self.pos_items.data_ptr()) + self._key_more()
        arena, arena_b = self.arena, self.arena_b
        urows, rrows = self.g_idx[:B_loc], self.g_idx[B_loc:B_loc + (B_loc if W == 1 else cap_r)]
        self.urows = urows
        base_t = B_loc + Sg
        X, dX = self._scorer_io()
        # world 1: nothing travels, so nothing is packed twice -- the pool bias goes straight to b_all, the pool
        # gradient and its row sums straight into the K7 arena, the target-bias gradient straight into arena_b
        T_in = self.T_pack if W == 1 else self.T_send[:cap_r]              # target rows as gathered
        dT = arena[base_t:base_t + B_loc] if W == 1 else self.dT_pack
        # default (ARX_SCORER_F32=1: the f32-MFMA logits / loss / GEMM kernels): the scorer on the bf16 matrix pipe --
        # hinge GEMM (act bits instead of logits / dlogits) + the two bit-operand backward products
        fused = self._fused_scorer()

        def fwd_gather():      # the step's lookups, one launch
            self._gather(urows, rrows, T_in)

        def fwd_score():
            self._input_fwd()
            if W > 1:    # blocks -> pool (slot) order, their bias column -> b_all
                be.gather_rows_multi([(self.I_gath, d, self.gidx, self.I_all, self.b_all)])
            if not fused:
                be.gemm(X, self.I_all[:, :d], self.logits, transB=True, col_bias=self.b_all)

        def loss():
            # (global mean => gscale = 1/B; the target score and its rank-one gradients are formed by the same
            # kernel, straight from / into the packed rows: bias and dt live in column d)
            dt = arena_b[base_t:base_t + B_loc] if W == 1 else dT[:, d]
            self._scorer_loss(fused, X, self.I_all[:, :d], urows, dt, dX, dT[:, :d])

        def bwd_gemms():
            if W == 1:
                self._scorer_bwd(fused, X, self.I_all[:, :d], dX, arena[B_loc:B_loc + S, :d],
                                 arena_b[B_loc:B_loc + S])
            else:
                self._scorer_bwd(fused, X, self.I_all[:, :d], dX, self.dI_all[:S, :d], self.gb_all)
                be.copy_strided(self.gb_all, self.dI_all[:S, d])
            self._input_bwd()

        def k7(phase):         # one fused scatter + Adagrad pass over all shards
            self._k7(phase, urows, rrows)

        def apply():
            if W > 1:    # the rows of this rank's block out of the summed pool gradient (bias column -> arena_b),
                #              the bias column of the received target-row gradients
                be.gather_rows_multi([(self.dI_all, d, self.my_slots[:cap], arena[B_loc:B_loc + cap],
                                       arena_b[B_loc:B_loc + cap])])
                be.copy_strided(arena[base_t:base_t + cap_r, d], arena_b[base_t:base_t + cap_r])
            k7(_ops.K7_APPLY)

        def body(mode):
            seg = lambda name, fn, feeds=None: self._segment(mode, name, fn, feeds)

            def whole_step():
                fwd_gather()
                # (with the branch's kernels captured BEHIND the scorer's forward launches -- the order arx/graph.py
                # uses -- the two chains overlap from the start, and the HET step got slower: 436 against 412-427 us.
                # Captured first, the sorts run ahead of the scorer and only their tail overlaps it: kept)
                sorted_ = self._k7_sorts(mode, k7, False)
                fwd_score()
                loss()
                bwd_gemms()
                self._k7_join(sorted_)
                apply()
                self._after_apply(lambda name, fn: fn())     # (one rank: in the same graph, at once)

            if W == 1:
                return seg('step', whole_step, feed)
            seg('fwd_gather', fwd_gather, feed)
            sorted_ = self._k7_sorts(mode, k7, True)
            dist.all_gather_into_tensor(self.I_gath[:W * cap], self.I_pack[:cap], group=grp)
            w_rows = _all_to_all(self.T_pack, self.T_send[:R], send, recv, group=grp, async_op=True)
            self._send_input_rows(route)
            seg('fwd_score', fwd_score)                       # scorer GEMM under the target-row exchange
            w_rows.wait()
            seg('loss', loss)
            w_dt = _all_to_all(arena[base_t:base_t + R], self.dT_pack, recv, send, group=grp, async_op=True)
            seg('bwd_gemms', bwd_gemms)                       # dX, dI under the gradient exchange
            w_dx = self._return_input_grads(route)
            # 0.5 MB: summed everywhere, every owner picks the rows of its block (padding -> the zero row)
            dist.all_reduce(self.dI_all[:S], op=dist.ReduceOp.SUM, group=grp)
            w_dt.wait()
            w_dx.wait()
            self._k7_join(sorted_)
            seg('apply', apply)
            self._after_apply(seg)

        return key, body

    # ---- what a subclass overrides in _step_body (here: the id-only step) ----
    def _step_blocks(self, route):
        """Grows the capacities to this route and returns the (rows, capacity) blocks of the index vector behind the
        user rows."""
        if route['R'] > self.cap_r:
            self._alloc_recv(route['R'])
        return [(route['recv_rows'], self.cap_r)]

    def _static_feeds(self, route, cap_r):
        return []

    def _key_more(self):
        return ()

    def _gather(self, urows, rrows, T_in, more=()):
        """The step's lookups in one launch: the user rows, the owned pool block, the requested target rows
        (+ more sites)."""
        cap = self.cap
        pool = (self.E_item, self.b_item, self.pool_rows, self.I_all, self.b_all) if self.world == 1 else \
            (self.E_item, self.b_item, self.pool_rows[:cap], self.I_pack[:cap], 'packed')
        self.be.gather_rows_multi([(self.E_user, None, urows, self.U_loc, None), pool,
                                   (self.E_item, self.b_item, rrows, T_in, 'packed'), *more])

    def _k7(self, phase, urows, rrows, tables=(), sites=()):
        """One fused scatter + Adagrad pass over the user shard and the item shard (+ more tables and their sites)."""
        B_loc, d, ni = self.B_loc, self.d, self.ni_loc
        self.be.sparse_adagrad_multi([(self.E_user, self.A_user, None, None),
                                      (self.E_item[:ni], self.A_item[:ni], self.b_item[:ni], self.Ab_item[:ni]),
                                      *tables],
                                     [(0, urows, 0), (1, self.pool_rows[:self.cap], B_loc),
                                      (1, rrows, B_loc + self.Sg), *sites],
                                     self.arena[:, :d], self.arena_b, self.lr, phase=phase)

    def _scorer_io(self):
        """(X, dX): what the scorer multiplies with the pool, and where its gradient goes."""
        return self.U_loc, self.arena[:self.B_loc, :self.d]

    def _input_fwd(self):
        pass

    def _input_bwd(self):
        pass

    def _send_input_rows(self, route):
        """Issued behind the target-row all-to-all; back before fwd_score."""

    def _return_input_grads(self, route):
        """Issued behind bwd_gemms; returns what the step waits for beside the target-row gradients."""
        return _Done()

    def _after_apply(self, seg):
        """Behind the apply segment; seg(name, fn) runs launches as a segment of the step."""

    def _fresh_step(self):
        """Before the body of a step that is not a replay (the first eager one, a capture, the step after an
        exception)."""

    # ---- shared by the bodies: the index feed and the scorer call ----
    def _index_feed(self, route, blocks):
        """The per-batch index vector [user rows ; the rows of every (rows, capacity) block, padded to its capacity
        with the shard's zero row], built once per route and set of capacities (kept on the route), and g_idx, the
        static vector it is copied into by the step's first node.  Returns the feed [(idx, g_idx)]."""
        B_loc = self.B_loc
        caps = tuple([c for _, c in blocks])
        idx = route.get('idx')
        if idx is None or route['idx_caps'] != caps:
            idx = torch.full((B_loc + sum(caps),), self.zero_row, dtype=torch.int32, device=self.device)
            idx[:B_loc] = route['urows']
            at = B_loc
            for rows, c in blocks:
                if rows.shape[0] > 0:
                    idx[at:at + rows.shape[0]] = rows
                at += c
            route['idx'], route['idx_caps'] = idx, caps
        if self.g_idx is None or self.g_idx.shape[0] != idx.shape[0]:
            self.g_idx = torch.empty(idx.shape[0], dtype=torch.int32, device=self.device)
        return [(idx, self.g_idx)]             # (a kernel: a device-to-device hipMemcpyAsync costs more)

    def _scorer_loss(self, fused, X, pool, urows, dt, dX, dT):
        """Loss, dlogits (fused: act bits), the target score and its rank-one gradients (dt, dX, dT) in one kernel:
        the bf16-pipe scorer's forward on (X, pool), or the loss kernel over the logits."""
        d = self.d
        if fused:
            self.scorer.fwd(X, pool, self.b_all, self.T_pack[:, :d], self.T_pack[:, d], urows, self.pos_ptr,
                            self.pos_items, self.item2slot, self.bl, self.t_loc, dt, dX, dT, 1.0 / self.B)
        else:
            self._loss_fused(self.logits, X, self.T_pack[:, :d], self.T_pack[:, d], urows, self.pos_ptr,
                             self.pos_items, self.item2slot, self.bl, self.dlogits, self.t_loc, dt, dX, dT,
                             1.0 / self.B)

    def _scorer_bwd(self, fused, X, pool, dX, dI, db):
        """The backward products: dX += dL . pool, dI = dL^T . X and its row sums db (the bias gradient)."""
        if fused:
            self.scorer.bwd_dU(dX, beta=1.0)
            self.scorer.bwd_dI(dI, db=db)
        else:
            self.be.gemm(self.dlogits, pool, dX, beta=1.0)
            self.be.gemm(self.dlogits, X, dI, transA=True, a_rowsum=db)

    def _step_body_pair(self, route):
        """The 'bpr' / 'bpr-hinge' step (hmf_model.py:96-107 on the global batch, gscale = 1 / B), a body for the same
        driver: no pool, so no scorer and no pool exchange -- lookups, ONE pair kernel, K7.

          fwd_gather   user rows -> U_loc; the requested rows (positives and negatives of any rank) -> the send block
          all_to_all   packed rows [2 B_loc - voids, d+4] out, in request order (route: slots)
          pair         arx_pair_loss_slots: scores, loss, dU into the arena, (-c U | -c) and (c U | c) into the slots
                       of the gradient block, the two integers of the auc
          all_to_all   gradient rows back to the owners, into the K7 arena [dU ; received rows]
          apply        one sparse_adagrad_multi over the user shard and the item shard: an item that is the positive
                       of one row and the negative of another -- on any ranks -- is one merged key, one update

        The per-batch vectors -- [user rows ; received rows, padded to cap_r with the shard's zero row] and the
        2 B_loc slots -- are fed by the segment's first node; K7's ids-only half runs on the side stream.  World 1:
        ONE graph, the rows gathered straight into the block the kernel reads and the gradient rows written straight
        into the arena.  Rows of the blocks that no slot names (behind the requests of a batch with void rows) are
        never read by the kernel, and their arena rows carry the padding key: K7 drops them."""
        be, W = self.be, self.world
        B, B_loc, d = self.B, self.B_loc, self.d
        grp = self.group
        send, recv, R, n_req = route['send'], route['recv'], route['R'], route['n_req']
        feed = self._index_feed(route, self._step_blocks(route)) + [(route['slots'], self.g_slots)]
        cap_r = self.cap_r
        key = ('pair', cap_r, self.g_idx.data_ptr(), self.arena.data_ptr(), self.g_slots.data_ptr())
        arena, arena_b = self.arena, self.arena_b
        urows, rrows = self.g_idx[:B_loc], self.g_idx[B_loc:]
        self.urows = urows
        ni = self.ni_loc
        n_rows = 2 * B_loc if W == 1 else cap_r            # rows of the gather / of K7's item site
        rrows = rrows[:n_rows]
        dU = arena[:B_loc, :d]
        T_in = self.R_pack if W == 1 else self.T_send[:cap_r]
        dR = arena[B_loc:B_loc + 2 * B_loc] if W == 1 else self.dR_pack
        pos_slot, neg_slot = self.g_slots[:B_loc], self.g_slots[B_loc:]
        kind = self.loss_name

        def fwd_gather():
            be.gather_rows_multi([(self.E_user, None, urows, self.U_loc, None),
                                  (self.E_item, self.b_item, rrows, T_in, 'packed')])

        def pair():
            be.pair_loss_slots(self.U_loc, self.R_pack, pos_slot, neg_slot, kind, 1.0 / B, self.pos_score,
                               self.neg_score, self.bl, dU, dR, self.auc_counts)

        def k7(phase):
            be.sparse_adagrad_multi([(self.E_user, self.A_user, None, None),
                                     (self.E_item[:ni], self.A_item[:ni], self.b_item[:ni], self.Ab_item[:ni])],
                                    [(0, urows, 0), (1, rrows, B_loc)], arena[:, :d], arena_b, self.lr, phase=phase)

        def apply():
            be.copy_strided(arena[B_loc:B_loc + n_rows, d], arena_b[B_loc:B_loc + n_rows])
            k7(_ops.K7_APPLY)

        def body(mode):
            seg = lambda name, fn, feeds=None: self._segment(mode, name, fn, feeds)

            def whole_step():
                fwd_gather()
                sorted_ = self._k7_sorts(mode, k7, False)
                pair()
                self._k7_join(sorted_)
                apply()

            if W == 1:
                return seg('step', whole_step, feed)
            seg('fwd_gather', fwd_gather, feed)
            sorted_ = self._k7_sorts(mode, k7, True)
            w_rows = _all_to_all(self.R_pack[:n_req], self.T_send[:R], send, recv, group=grp, async_op=True)
            w_rows.wait()
            seg('pair', pair)
            w_dr = _all_to_all(arena[B_loc:B_loc + R], self.dR_pack[:n_req], recv, send, group=grp, async_op=True)
            w_dr.wait()
            self._k7_join(sorted_)
            seg('apply', apply)

        return key, body

    def read_auc(self):
        """auc of the last pair step over the global batch: 0.5 - 0.5 * mean sign(neg_score - pos_score) over the rows
        that are not void (0.5 without such a row), as a python float.  A collective: the two integers of every rank
        (sign sum, live rows) are summed first."""
        if not self.pair:
            raise RuntimeError("read_auc: a pair-loss model's figure, this model trains %r" % self.loss_name)
        c = self.auc_counts.clone()
        dist.all_reduce(c, op=dist.ReduceOp.SUM, group=self.group)
        sg, cnt = (int(v) for v in c.cpu().tolist())
        return 0.5 - 0.5 * sg / cnt if cnt > 0 else 0.5

    def read_loss(self):
        """Global mean loss of the last step (device scalar; one tiny all-reduce)."""
        self.be.sum_scaled(self.bl, 1.0 / self.B, self.loss)
        dist.all_reduce(self.loss, op=dist.ReduceOp.SUM, group=self.group)
        return self.loss

    # --------------------------------------------------------------- recommend
    def prepare_recommend_exclusions(self, item_sets):
        """The items recommend(exclude_seen=True) leaves out per user -- typically the training history.  A
        collective: every rank passes the histories of users IT owns, {global user: global items} or a
        (users, ptr, items) CSR triple.  The (user, item) pairs travel to the item's owner (all_to_all); each rank
        keeps, on the device, a CSR keyed by global user id (ptr: n_users + 1 entries) over its own local columns
        (item // world), sorted, without duplicates.  A second call replaces the lists."""
        self._rec_ex = self._route_item_sets(item_sets, "exclusions", "exclusion lists")

    def _route_item_sets(self, item_sets, what, lists):
        """Per-user item sets of the users this rank owns -> the device CSR (ptr [n_users + 1], local columns) of the
        pairs whose item this rank owns (a collective: the pairs cross by all_to_all).  what / lists: the names in
        the error messages."""
        W, r = self.world, self.rank
        if isinstance(item_sets, dict):
            keys = list(item_sets.keys())
            parts = [np.asarray(list(item_sets[u]), dtype=np.int64).reshape(-1) for u in keys]
            users = np.repeat(np.asarray(keys, dtype=np.int64), [len(x) for x in parts])
            items = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
        elif isinstance(item_sets, tuple) and len(item_sets) == 3:
            u0 = np.asarray(item_sets[0], dtype=np.int64).reshape(-1)
            ptr = np.asarray(item_sets[1], dtype=np.int64).reshape(-1)
            items = np.asarray(item_sets[2], dtype=np.int64).reshape(-1)
            if len(ptr) != len(u0) + 1 or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] > len(items):
                raise ValueError("%s: ptr must have len(users) + 1 entries, start at 0, not decrease and "
                                 "end within the items" % what)
            users = np.repeat(u0, np.diff(ptr))
            items = items[:ptr[-1]]
        else:
            raise ValueError("%s: a {user: items} dict or a (users, ptr, items) CSR triple" % what)
        if len(users) and (users.min() < 0 or users.max() >= self.n_users or np.any(users % W != r)):
            raise ValueError("%s: every user must be a global id in [0, %d) owned by rank %d (id %% %d == %d)"
                             % (what, self.n_users, r, W, r))
        if len(items) and (items.min() < 0 or items.max() >= self.n_items):
            raise ValueError("%s: item ids must lie in [0, %d)" % (what, self.n_items))
        order, _, send = owner_order(items, W)
        pairs = np.stack([users, items], 1)[order].astype(np.int32).reshape(-1)
        if W == 1:
            recv = pairs
        else:
            cnt = self._count_exchange(send)
            out = torch.zeros((2 * sum(cnt),), dtype=torch.int32, device=self.device)
            _all_to_all(out, torch.from_numpy(pairs).to(self.device), [2 * c for c in cnt],
                        [2 * int(c) for c in send.tolist()], group=self.group)
            recv = out.cpu().numpy()
        ru, cols = recv[0::2].astype(np.int64), recv[1::2].astype(np.int64) // W
        o = np.lexsort((cols, ru))
        ru, cols = ru[o], cols[o]
        if len(ru):
            keep = np.ones(len(ru), dtype=bool)
            keep[1:] = (ru[1:] != ru[:-1]) | (cols[1:] != cols[:-1])
            ru, cols = ru[keep], cols[keep]
        ptr = np.zeros(self.n_users + 1, dtype=np.int64)
        np.cumsum(np.bincount(ru, minlength=self.n_users), out=ptr[1:])
        if ptr[-1] >= 2 ** 31:
            raise ValueError("%s: more than 2^31 - 1 entries on one rank" % lists)
        if len(cols) == 0:
            cols = np.zeros(1, dtype=np.int64)          # (a valid device pointer; every list is empty)
        return (torch.from_numpy(ptr.astype(np.int32)).to(self.device),
                torch.from_numpy(cols.astype(np.int32)).to(self.device))

    def prepare_item_tags(self, tags):
        """The items' 32-bit tag words for recommend(tags_any=, tags_all=): the FULL integer array [n_items] of words
        in [0, 2^32), the same on every rank.  Each rank keeps its stripe tags[rank::world] on the device as int32 bit
        patterns; not a collective.  A second call replaces the words.  (Serving metadata, like the exclusion lists:
        checkpoints do not store them.)"""
        t = tags.cpu().numpy() if isinstance(tags, torch.Tensor) else np.asarray(tags)
        if t.ndim != 1 or len(t) != self.n_items or t.dtype == np.bool_ or not np.issubdtype(t.dtype, np.integer):
            raise ValueError("item tags: an integer array of n_items = %d words" % self.n_items)
        if len(t) and (t.min() < 0 or t.max() >= 2 ** 32):
            raise ValueError("item tags: words must lie in [0, 2^32)")
        mine = np.ascontiguousarray(t[self.rank::self.world].astype(np.uint32)).view(np.int32)
        self._rec_tags = torch.from_numpy(mine).to(self.device)

    def recommend(self, users, k, exclude_seen=False, return_values=False, tags_any=None, tags_all=None):
        """Full-vocabulary top-k (run_hmf.py:340-409: top_k(logits, top_N) per user) of the row-sharded model.  A
        collective: every rank calls it with the same k and exclude_seen, and all with or all without tags.  users: global ids this rank owns,
        0 <= len(users) <= B_loc (the count may differ between ranks).  Returns int32 global item ids
        [len(users), k] on the device, ordered by (score desc, id asc) -- tf.nn.top_k's rule -- (and their float32
        scores with return_values); -1 (score -inf) where a user has fewer than k eligible items.  exclude_seen:
        leave out each user's items of prepare_recommend_exclusions (ValueError without it).  tags_any / tags_all
        (an int: one word for every user, or one int per user): only the items whose tag word of prepare_item_tags
        has a bit of `any` (0: no constraint) and every bit of `all`; the words travel with the user keys (two more
        all_gathers); composes with exclude_seen.

          gather          this rank's user rows -> [B_loc, d] (padding rows: zeros, key -1)
          all_gather      latents [B_loc, d] -> [B, d], user ids [B_loc] -> [B]
          (local)         top-k of U_all . E_item[:ni]^T + b_item[:ni] over the shard's rows (backend.shard_topk:
                          the fused filter GEMM of StreamTopK, chunked after an overflow -- on this rank only)
          all_to_all      value / local-column lists [B, k] -> the ranks that own the rows: [W][B_loc][k]
          (local)         W-way merge into global ids c * W + s (arx_topk_merge_shards)

        Eager (no capture); with graph segments on the model's stream, joined with the caller's on both sides as
        step() is, so a recommend right after a step reads that step's tables.  Its buffers are its own, per k.
        (The SAMPLED recommend and its propensities: recommend_sampled, an entry of its own -- this parameter list is
        pinned by tests/test_sharded_recommend_tags_cpu.py.)"""
        return self.recommend_sampled(users, k, exclude_seen=exclude_seen, return_values=return_values,
                                      tags_any=tags_any, tags_all=tags_all)

    def recommend_sampled(self, users, k, exclude_seen=False, return_values=False, tags_any=None, tags_all=None,
                          sample_temperature=None, sample_seed=None, return_logprob=False):
        """recommend (its rules for users, k, exclude_seen, return_values and the tags hold) with
        sample_temperature (None: recommend itself, bit for bit -- no further collective, no further launch): the SAMPLED
        recommend -- k distinct items drawn from softmax(score / tau) over the user's whole eligible vocabulary ACROSS
        the shards, one after the other without replacement, ids in SELECTION order; one number, or one per user of
        this rank (topk.sample_params; tau = 0: that user's row is the plain top-k).  All ranks pass a temperature, or
        none does.  sample_seed: an int in [0, 2^63), the SAME on every rank like k (ValueError on every rank where
        the ranks' seeds differ); None counts up a per-model counter, the same on every rank that calls in lockstep.
        The noise is g(seed, GLOBAL user id, GLOBAL item id) of arx_sample.h: a draw depends on (seed, user, item) and
        the scores alone -- not on the world size, B_loc, the user's position in the call or who else is in it, so a
        logged draw can be recomputed for one user later.  (Not the single-device convention, where the noise row is
        the batch row.)  Two rows of the same user in one call (possible with ShardedW2V) share their noise.
        return_values: the picks' scores -- the stripped keys, within 2^-23 (|key| + |score|) of the score; with
        return_logprob the exact bits of the shard's scorer GEMM.  return_logprob=True (ValueError without a
        temperature: topk.check_return_logprob): the tuple ends with logprob [len(users), k], the log-probability of
        every pick given the picks before it by the rule of arx_sample_logp.h over the whole eligible vocabulary
        (exclude_seen and the tags included): 0 for a tau = 0 row and beside an id -1.  The sampled call adds:

          all_gather      + tau bits [B_loc] and the two seed words, in ONE int32 buffer -> every rank
          (local)         the shard top-k is that of the KEYS (TopKScan with the keyed sample: noise column
                          c * W + s, noise row the user id), NOT stripped; overflow -> chunked, as above
          all_to_all      key / local-column lists, as above
          (local)         arx_topk_merge_shards on the keys (ties: lower global id) -> ids in selection order
           without logp:  arx_topk_gumbel_strip_keyed at the owner (global ids: col_mul 1, col_add 0)
           with logp:     all_gather of the picks [B_loc, k] -> [B, k]; per shard: arx_picks_to_shard,
                          arx_sample_logp_sort, the rest-mass pass over the shard (arx_gemm_nt_rest_mass where the
                          fused form applies, arx_rest_mass_chunk otherwise), pick scores pre-filled with -inf;
                          ONE all_to_all of a packed float buffer [B, 2 P_max + k] (m parts, S parts, pick scores;
                          a shard with fewer parts pads with the empty mass) -> owners;
                          arx_sample_logp_finish_shards over the W slabs

        Eager, on the model's stream, as recommend is."""
        W, r = self.world, self.rank
        u = users.cpu().numpy() if isinstance(users, torch.Tensor) else np.asarray(users)
        u = u.astype(np.int64).reshape(-1)
        k = int(k)
        if not 1 <= k <= min(1024, self.n_items):
            raise ValueError("recommend: need 1 <= k <= min(1024, n_items)")
        if len(u) > self.B_loc:
            raise ValueError("recommend: at most B_loc = %d users per call and rank" % self.B_loc)
        if len(u) and (u.min() < 0 or u.max() >= self.n_users or np.any(u % W != r)):
            raise ValueError("recommend: users must be global ids in [0, %d) owned by rank %d" % (self.n_users, r))
        if exclude_seen and getattr(self, '_rec_ex', None) is None:
            raise ValueError("exclude_seen=True needs prepare_recommend_exclusions() first")
        words = None
        if tags_any is not None or tags_all is not None:
            if getattr(self, '_rec_tags', None) is None:
                raise ValueError("tags_any / tags_all need prepare_item_tags() first")
            words = tag_words(tags_any, tags_all, len(u))
        check_return_logprob(return_logprob, True, sample_temperature)
        more = {}
        if sample_temperature is not None:
            seed = sample_seed if sample_seed is not None else getattr(self, 'sample_draws', 0)
            tau, seed_words = sample_params(sample_temperature, seed, len(u))
            if sample_seed is None:                     # (after the checks: a refused call does not move the counter)
                self.sample_draws = seed + 1
            more['sample'] = (tau, seed_words, bool(return_logprob))
        if words is not None:
            more['tags'] = words
        with _ops.joined(self._stream if self.use_graphs else None):
            out = self._recommend(u, k, exclude_seen, **more)
        n = len(u)
        ids = out[1][:n].clone()
        res = (ids,) + ((out[0][:n].clone(),) if return_values else ()) + \
            ((out[2][:n].clone(),) if return_logprob else ())
        return res if len(res) > 1 else ids

    def _gather_request(self, u, exclude_seen, tags=None, sample=None):
        """The request of a full-vocabulary serving call on every rank (recommend, recommend_sampled, list_logprob):
        this rank's latents and keys (padding rows: zeros, key -1), its temperatures as bits with the two seed words
        (padding rows: 0) and its tag words (padding rows: 0) are all_gathered; the buffers are kept on the model.
        tags: (any, all) host words or None; sample: (tau, seed words) on the host or None.  Returns (keys_loc, U_all,
        keys_all, ex, the backend's tags tuple or None, the backend's sample tuple or None, tau_all, seed_dev)."""
        be, W, B_loc, B, d = self.be, self.world, self.B_loc, self.B, self.d
        dev, f32, i32 = self.device, torch.float32, torch.int32
        n = len(u)
        if getattr(self, '_rec_lat', None) is None:     # [B_loc] keys, [B_loc, d] rows; gathered: [B], [B, d]
            kl, ul = torch.full((B_loc,), -1, dtype=i32, device=dev), torch.zeros((B_loc, d), dtype=f32, device=dev)
            self._rec_lat = (kl, ul) + ((kl, ul) if W == 1 else
                                        (torch.empty((B,), dtype=i32, device=dev),
                                         torch.empty((B, d), dtype=f32, device=dev)))
            self._rec_k = {}
        keys_loc, U_loc, keys_all, U_all = self._rec_lat
        kh = np.full(B_loc, -1, dtype=np.int32)
        kh[:n] = u
        keys_loc.copy_(torch.from_numpy(kh))
        self._serve_latents(u, U_loc[:n])
        if n < B_loc:
            be.fill_zero(U_loc[n:])
        if W > 1:
            dist.all_gather_into_tensor(U_all, U_loc, group=self.group)
            dist.all_gather_into_tensor(keys_all, keys_loc, group=self.group)
        ex = (keys_all, B, self._rec_ex[0], self._rec_ex[1]) if exclude_seen else None
        smp = tau_all = seed_dev = btags = None
        if sample is not None:
            # this rank's temperatures (as bits; padding rows: 0) and the two seed words -> every rank in ONE buffer;
            # `sample=` goes to the backend only here, as `tags=` does
            tau_h, seed_h = sample
            if getattr(self, '_rec_smp', None) is None:
                loc = torch.zeros((B_loc + 2,), dtype=i32, device=dev)
                self._rec_smp = (loc, loc if W == 1 else torch.empty((W * (B_loc + 2),), dtype=i32, device=dev),
                                 torch.empty((B,), dtype=f32, device=dev), torch.empty((2,), dtype=i32, device=dev))
            smp_loc, smp_all, tau_all, seed_dev = self._rec_smp
            h = np.zeros(B_loc + 2, dtype=np.int32)
            h[:n] = np.ascontiguousarray(tau_h, dtype=np.float32).view(np.int32)
            h[B_loc:] = seed_h
            smp_loc.copy_(torch.from_numpy(h))
            if W > 1:
                dist.all_gather_into_tensor(smp_all, smp_loc, group=self.group)
                sw = smp_all.view(W, B_loc + 2)[:, B_loc:].cpu().numpy()
                if np.any(sw != sw[0]):                 # (every rank sees the same words: they all raise)
                    raise ValueError("recommend: sample_seed must be the same on every rank")
            g = smp_all.view(W, B_loc + 2)
            tau_all.view(W, B_loc).copy_(g[:, :B_loc].view(f32))
            seed_dev.copy_(g[0, B_loc:])
            smp = (tau_all, B, seed_dev, W, self.rank, keys_all)
        if tags is not None:
            # the request words of this rank's users (padding rows: no constraint) -> every rank, like the keys;
            # `tags=` goes to the backend only here, so one that does not know the argument serves the plain calls
            if getattr(self, '_rec_words', None) is None:
                z = lambda m: torch.zeros((m,), dtype=i32, device=dev)
                loc = (z(B_loc), z(B_loc))
                self._rec_words = loc + (loc if W == 1 else (z(B), z(B)))
            any_loc, all_loc, any_all, all_all = self._rec_words
            for dst, w in ((any_loc, tags[0]), (all_loc, tags[1])):
                h = np.zeros(B_loc, dtype=np.int32)
                h[:n] = w
                dst.copy_(torch.from_numpy(h))
            if W > 1:
                dist.all_gather_into_tensor(any_all, any_loc, group=self.group)
                dist.all_gather_into_tensor(all_all, all_loc, group=self.group)
            btags = (self._rec_tags[:self.ni_loc], any_all, all_all, B)
        return keys_loc, U_all, keys_all, ex, btags, smp, tau_all, seed_dev

    def _recommend(self, u, k, exclude_seen, tags=None, sample=None):
        be, W, B_loc, B, d = self.be, self.world, self.B_loc, self.B, self.d
        dev, f32, i32 = self.device, torch.float32, torch.int32
        want_logp = sample is not None and sample[2]
        keys_loc, U_all, keys_all, ex, btags, smp, tau_all, seed_dev = self._gather_request(
            u, exclude_seen, tags, sample[:2] if sample is not None else None)
        bk = self._rec_k.get(k)
        if bk is None:
            e = lambda dt, *sh: torch.empty(sh, dtype=dt, device=dev)
            bk = self._rec_k[k] = (e(f32, B, k), e(i32, B, k), e(f32, W, B_loc, k), e(i32, W, B_loc, k),
                                   e(f32, B_loc, k), e(i32, B_loc, k))
        out_v, out_i, recv_v, recv_c, vo, io = bk
        ni = self.ni_loc
        more = {}
        if smp is not None:
            more['sample'] = smp
        if btags is not None:
            more['tags'] = btags
        be.shard_topk(U_all, self.E_item[:ni], self.b_item[:ni], k, ex, out_v, out_i, **more)
        if W == 1:
            recv_v, recv_c = out_v.view(1, B, k), out_i.view(1, B, k)
        else:
            _all_to_all(recv_v.view(B, k), out_v, group=self.group)
            _all_to_all(recv_c.view(B, k), out_i, group=self.group)
        be.topk_merge_shards(recv_v, recv_c, vo, io)
        if smp is None:
            return vo, io
        # the owner's own rows: its temperatures, global item ids as the noise columns
        r0 = self.rank * B_loc
        own = (tau_all[r0:r0 + B_loc], B_loc, seed_dev, 1, 0, keys_loc)
        if not want_logp:
            be.sample_strip(vo, io, own)
            return vo, io
        P_max = max(be.shard_mass_parts(B, len(range(s, self.n_items, W)), d) for s in range(W))
        lk = self.__dict__.setdefault('_rec_logp', {})
        bl = lk.get((k, P_max))
        if bl is None:
            wd = 2 * P_max + k
            bl = lk[(k, P_max)] = (torch.empty((B, wd), dtype=f32, device=dev),
                                   None if W == 1 else torch.empty((W, B_loc, wd), dtype=f32, device=dev),
                                   io if W == 1 else torch.empty((B, k), dtype=i32, device=dev),
                                   torch.empty((B_loc, k), dtype=f32, device=dev))
        packed, recv_p, picks_all, lp = bl
        if W > 1:
            dist.all_gather_into_tensor(picks_all, io, group=self.group)
        kw = {'tags': more['tags']} if tags is not None else {}
        be.shard_rest_mass(U_all, self.E_item[:ni], self.b_item[:ni], ex, picks_all, W, self.rank, smp, packed, P_max,
                           **kw)
        if W == 1:
            recv_p = packed.view(1, B, 2 * P_max + k)
        else:
            _all_to_all(recv_p.view(B, 2 * P_max + k), packed, group=self.group)
        be.sample_logp_finish_shards(io, recv_p, P_max, own, lp, vo)
        return vo, io, lp

    # ------------------------------------------------------------- list_logprob
    def list_logprob(self, users, lists, sample_temperature, exclude_seen=False, tags_any=None, tags_all=None,
                     return_values=False, return_why=False):
        """The log-probability of GIVEN ordered lists under recommend_sampled's policy at sample_temperature -- the
        numerator of the importance weight whose denominator recommend_sampled(return_logprob=True) logged
        (arx.utils.ope), over the user's whole eligible vocabulary ACROSS the shards.  A collective with
        recommend_sampled's calling rules: every rank calls it with the same k = lists.shape[1] (1 <= k <= 1024, tied to
        nothing else) and exclude_seen, and all with or all without tags; users: global ids this rank owns,
        0 <= len(users) <= B_loc (the count may differ between ranks); lists [len(users), k]: GLOBAL item ids of any
        origin (topk.check_lists), -1 an empty slot; sample_temperature: one number or one per user, every one > 0
        (topk.list_taus).  There is no seed: the noise plays no part in a propensity.  Returns float32 logprob
        [len(users), k] on the device, or the tuple (logprob[, values][, why]); the semantics are arx_list_logp.h's:
        logp[r][t] of entry t given the drawable entries before it, 0 at -1, -inf at the reason codes 2-6 (such an
        entry is ABSENT for the others), so the row sum is -inf exactly when the policy cannot produce the list;
        values: the exact bits of the owner shard's scorer, -inf elsewhere; why int32: the codes.  A list
        recommend_sampled(return_logprob=True) drew itself comes back with its logged logprob and values bit for bit.
        Every check runs before any collective.

          gather / all_gather   latents, keys, tau bits, tag words as recommend_sampled; + the lists [B_loc, k] -> [B, k]
                                (padding rows: -1)
          (local)               arx_list_logp_prepare_shard: the codes this shard can give (the exclusion lists and the
                                tag words live with the item's owner), its surviving entries as sorted picks; then the
                                rest-mass pass of recommend_sampled over them (no arx_picks_to_shard, no sort)
          all_to_all            ONE packed float buffer [B, 2 P_max + 2 k] -> owners: m parts, S parts, pick scores and
                                the k codes, which travel as int32 BITS in the same buffer (it is viewed as int32 where
                                they are written and where they are read; the exchange moves bytes)
          (local)               arx_list_logp_merge_shards (why, the global clean list), then
                                arx_sample_logp_finish_shards over the clean list and arx_list_logp_stamp

        Eager, on the model's stream, as recommend is; its buffers are its own, per (k, P_max)."""
        what = 'list_logprob'
        W, r = self.world, self.rank
        u = users.cpu().numpy() if isinstance(users, torch.Tensor) else np.asarray(users)
        u = u.astype(np.int64).reshape(-1)
        if len(u) > self.B_loc:
            raise ValueError("%s: at most B_loc = %d users per call and rank" % (what, self.B_loc))
        if len(u) and (u.min() < 0 or u.max() >= self.n_users or np.any(u % W != r)):
            raise ValueError("%s: users must be global ids in [0, %d) owned by rank %d" % (what, self.n_users, r))
        a, k = check_lists(lists, len(u), what)
        tau = list_taus(sample_temperature, len(u), what)
        if not len(u) and np.ndim(sample_temperature) == 0:
            list_taus(sample_temperature, 1, what)      # (a rank without users refuses the number the others refuse)
        if exclude_seen and getattr(self, '_rec_ex', None) is None:
            raise ValueError("exclude_seen=True needs prepare_recommend_exclusions() first")
        words = None
        if tags_any is not None or tags_all is not None:
            if getattr(self, '_rec_tags', None) is None:
                raise ValueError("tags_any / tags_all need prepare_item_tags() first")
            words = tag_words(tags_any, tags_all, len(u), what)
        with _ops.joined(self._stream if self.use_graphs else None):
            lp, vals, why = self._list_logprob(u, a, k, tau, exclude_seen, words)
        n = len(u)
        res = (lp[:n].clone(),) + ((vals[:n].clone(),) if return_values else ()) + \
            ((why[:n].clone(),) if return_why else ())
        return res if len(res) > 1 else res[0]

    def _list_logprob(self, u, lists, k, tau, exclude_seen, tags):
        be, W, B_loc, B, d = self.be, self.world, self.B_loc, self.B, self.d
        dev, f32, i32 = self.device, torch.float32, torch.int32
        n = len(u)
        keys_loc, U_all, keys_all, ex, btags, smp, tau_all, seed_dev = self._gather_request(
            u, exclude_seen, tags, (tau, np.zeros(2, dtype=np.int32)))
        P_max = max(be.shard_mass_parts(B, len(range(s, self.n_items, W)), d) for s in range(W))
        lk = self.__dict__.setdefault('_list_bufs', {})
        bl = lk.get((k, P_max))
        if bl is None:
            if len(lk) > 8:
                lk.clear()
            wd = 2 * P_max + 2 * k
            e = lambda dt, *sh: torch.empty(sh, dtype=dt, device=dev)
            lists_loc = e(i32, B_loc, k)
            bl = lk[(k, P_max)] = (lists_loc, lists_loc if W == 1 else e(i32, B, k), e(f32, B, wd),
                                   None if W == 1 else e(f32, W, B_loc, wd), e(i32, B_loc, k), e(i32, B_loc, k),
                                   e(f32, B_loc, k), e(f32, B_loc, k))
        lists_loc, lists_all, packed, recv_p, clean, why, lp, vals = bl
        wd = 2 * P_max + 2 * k
        if isinstance(lists, torch.Tensor):
            lists_loc[:n].copy_(lists)
        elif n:
            lists_loc[:n].copy_(torch.from_numpy(lists))
        if n < B_loc:
            lists_loc[n:].fill_(-1)
        if W > 1:
            dist.all_gather_into_tensor(lists_all, lists_loc, group=self.group)
        ni = self.ni_loc
        prepared = be.shard_list_prepare(lists_all, self.n_items, W, self.rank, ni, ex, btags,
                                         packed.view(i32)[:, 2 * P_max + k:])
        kw = {'tags': btags} if btags is not None else {}
        be.shard_rest_mass(U_all, self.E_item[:ni], self.b_item[:ni], ex, lists_all, W, self.rank, smp,
                           packed[:, :2 * P_max + k], P_max, prepared=prepared, **kw)
        if W == 1:
            recv_p = packed.view(1, B, wd)
        else:
            _all_to_all(recv_p.view(B, wd), packed, group=self.group)
        be.list_logp_merge_shards(lists_loc, self.n_items, recv_p.view(i32)[:, :, 2 * P_max + k:], clean, why)
        r0 = self.rank * B_loc
        own = (tau_all[r0:r0 + B_loc], B_loc, seed_dev, 1, 0, keys_loc)
        be.sample_logp_finish_shards(clean, recv_p, P_max, own, lp, vals)
        be.list_logp_stamp(clean, vals, why, lp)
        return lp, vals, why

    # ------------------------------------------------------------ similar_items
    def similar_items(self, items, k, include_self=False, return_values=False, return_logprob=False):
        """(return_logprob=True: NotImplementedError.)
        Cosine nearest neighbours of items over the full item vocabulary of the row-sharded model, in the latent
        space recommend scores against (E_item; the bias plays no part).  A collective with recommend's calling rules:
        every rank calls it with the same k and include_self.  items: global ids this rank OWNS (id % world == rank),
        0 <= len(items) <= B_loc (the count may differ between ranks; an id may come twice).  Returns int32 global item
        ids [len(items), k] on the device ordered by (cosine desc, id asc) (and their float32 cosines with
        return_values); include_self False leaves the query itself out; -1 (cosine -inf) where fewer than k items are
        left.  A zero row has cosine 0 with everything, also as a query.

          gather          this rank's query rows as UNIT rows -> [B_loc, d] (backend.gather_rows_unit; padding: zeros)
          all_gather      rows [B_loc, d] -> [B, d], item ids [B_loc] -> [B] (padding: -1)
          (local)         the local column of every query this shard owns (arx_shard_route's keys; none elsewhere)
          (local)         inverse norms of the shard, recomputed at every call (one read of it: no cache to go stale),
                          then the top-k of Q_all . E_item[:ni]^T * inv_norm over the shard (backend.shard_similar)
          all_to_all      value / local-column lists [B, k] -> the ranks that own the queries: [W][B_loc][k]
          (local)         W-way merge into global ids (arx_topk_merge_shards)

        Eager, joined with the model's stream as recommend is; its buffers are its own, per k."""
        no_return_logprob("%s.similar_items" % type(self).__name__, return_logprob)
        W, r = self.world, self.rank
        it = items.cpu().numpy() if isinstance(items, torch.Tensor) else np.asarray(items)
        it = it.astype(np.int64).reshape(-1)
        k = int(k)
        if not 1 <= k <= min(1024, self.n_items):
            raise ValueError("similar_items: need 1 <= k <= min(1024, n_items)")
        if len(it) > self.B_loc:
            raise ValueError("similar_items: at most B_loc = %d items per call and rank" % self.B_loc)
        if len(it) and (it.min() < 0 or it.max() >= self.n_items or np.any(it % W != r)):
            raise ValueError("similar_items: items must be global ids in [0, %d) owned by rank %d" % (self.n_items, r))
        with _ops.joined(self._stream if self.use_graphs else None):
            vo, io = self._similar(it, k, bool(include_self))
        n = len(it)
        ids = io[:n].clone()
        return (ids, vo[:n].clone()) if return_values else ids

    def _similar(self, it, k, include_self):
        be, W, B_loc, B, d = self.be, self.world, self.B_loc, self.B, self.d
        dev, f32, i32 = self.device, torch.float32, torch.int32
        n = len(it)
        if getattr(self, '_sim_lat', None) is None:     # [B_loc] ids / local rows, [B_loc, d] rows; gathered: [B], [B, d]
            kl, ql = torch.full((B_loc,), -1, dtype=i32, device=dev), torch.zeros((B_loc, d), dtype=f32, device=dev)
            self._sim_lat = (kl, ql, torch.full((B_loc,), -1, dtype=i32, device=dev),
                             torch.empty((B,), dtype=i32, device=dev)) + \
                ((kl, ql) if W == 1 else (torch.empty((B,), dtype=i32, device=dev),
                                          torch.empty((B, d), dtype=f32, device=dev)))
            self._sim_k = {}
        keys_loc, Q_loc, rows_loc, self_cols, keys_all, Q_all = self._sim_lat
        bk = self._sim_k.get(k)
        if bk is None:
            e = lambda dt, *sh: torch.empty(sh, dtype=dt, device=dev)
            bk = self._sim_k[k] = (e(f32, B, k), e(i32, B, k), e(f32, W, B_loc, k), e(i32, W, B_loc, k),
                                   e(f32, B_loc, k), e(i32, B_loc, k))
        out_v, out_i, recv_v, recv_c, vo, io = bk
        kh = np.full(B_loc, -1, dtype=np.int32)
        kh[:n] = it
        keys_loc.copy_(torch.from_numpy(kh))
        kh = np.full(B_loc, -1, dtype=np.int32)
        kh[:n] = it // W
        rows_loc.copy_(torch.from_numpy(kh))
        ni = self.ni_loc
        be.gather_rows_unit(self.E_item[:ni], rows_loc, Q_loc)          # (a padding row, -1: zeros)
        if W > 1:
            dist.all_gather_into_tensor(Q_all, Q_loc, group=self.group)
            dist.all_gather_into_tensor(keys_all, keys_loc, group=self.group)
        if not include_self:
            # (ids < 0 and items of other shards: ARX_KEY_NONE, a column of no shard)
            be.shard_route(keys_all, W, self.rank, self.zero_row, None, self_cols)
        be.shard_similar(Q_all, self.E_item[:ni], k, None if include_self else self_cols, out_v, out_i)
        if W == 1:
            recv_v, recv_c = out_v.view(1, B, k), out_i.view(1, B, k)
        else:
            _all_to_all(recv_v.view(B, k), out_v, group=self.group)
            _all_to_all(recv_c.view(B, k), out_i, group=self.group)
        be.topk_merge_shards(recv_v, recv_c, vo, io)
        return vo, io

    # -------------------------------------------------------------- score_items
    def score_items(self, users, candidates, k=None):
        """What the model thinks of THESE items for THIS user: every user against a slate of its own (re-ranking
        another retriever's candidates, an editorial slate, sampled-negative evaluation).  A collective with
        recommend's calling rules: every rank calls it with the same C and k.  users: global ids this rank owns,
        0 <= len(users) <= B_loc (the count may differ between ranks); candidates: [len(users), C] GLOBAL item ids,
        -1 an empty slot.  k None: float32 [len(users), C] scores on the device, -inf at empty slots.
        1 <= k <= min(1024, C): (ids int32 [len(users), k], values float32) by (score desc, slot asc) -- duplicates
        and ties keep slate order --, (-1, -inf) where a user has fewer than k live slots.  Build-defined.

          gather          this rank's latents (_serve_latents) -> [B_loc, d]; padding rows zero, their slots -1
          all_gather      latents -> [B, d]; candidates [B_loc, C] -> [B, C]
          (local)         arx_shard_route: global id -> local column or ARX_KEY_NONE; arx_slate_scores over
                          E_item[:ni] / b_item[:ni] (a slot of another shard: -inf, nothing read)
          all_to_all      partial scores [B, C] -> the rows' owners: [W][B_loc][C]
          (local)         arx_slate_merge_shards; with k, slate_order over the owner's [B_loc, C] and its own GLOBAL
                          candidate ids

        Eager, joined with the caller's stream on both sides as recommend is; its buffers are its own, per (C, k)."""
        W, r = self.world, self.rank
        u = users.cpu().numpy() if isinstance(users, torch.Tensor) else np.asarray(users)
        u = u.astype(np.int64).reshape(-1)
        if len(u) > self.B_loc:
            raise ValueError("score_items: at most B_loc = %d users per call and rank" % self.B_loc)
        if len(u) and (u.min() < 0 or u.max() >= self.n_users or np.any(u % W != r)):
            raise ValueError("score_items: users must be global ids in [0, %d) owned by rank %d" % (self.n_users, r))
        cand = _slate.check_slate(candidates, len(u), self.n_items)
        k = _slate.check_k(k, int(cand.shape[1]))
        with _ops.joined(self._stream if self.use_graphs else None):
            sc, vo, io = self._score_items(u, cand, k)
        n = len(u)
        if k is None:
            return sc[:n].clone()
        return io[:n].clone(), vo[:n].clone()

    def _score_items(self, u, cand, k):
        be, W, B_loc, B, d = self.be, self.world, self.B_loc, self.B, self.d
        dev, f32, i32 = self.device, torch.float32, torch.int32
        n, C = len(u), int(cand.shape[1])
        if getattr(self, '_sl_lat', None) is None:       # [B_loc, d] latents; gathered: [B, d]
            ul = torch.zeros((B_loc, d), dtype=f32, device=dev)
            self._sl_lat = (ul, ul if W == 1 else torch.empty((B, d), dtype=f32, device=dev))
            self._sl_k = {}
        U_loc, U_all = self._sl_lat
        bk = self._sl_k.get((C, k))
        if bk is None:
            if len(self._sl_k) >= 8:
                self._sl_k.clear()
            e = lambda dt, *sh: torch.empty(sh, dtype=dt, device=dev)
            cl = e(i32, B_loc, C)
            bk = self._sl_k[(C, k)] = (cl, cl if W == 1 else e(i32, B, C), e(i32, B, C), e(f32, B, C),
                                       e(f32, W, B_loc, C), e(f32, B_loc, C)) + \
                ((e(f32, B_loc, k), e(i32, B_loc, k), e(i32, B_loc, k)) if k is not None else (None, None, None))
        cand_loc, cand_all, cols, part, recv, merged, vo, pos, io = bk
        ch = np.full((B_loc, C), -1, dtype=np.int32)
        ch[:n] = cand
        cand_loc.copy_(torch.from_numpy(ch))
        self._serve_latents(u, U_loc[:n])
        if n < B_loc:
            be.fill_zero(U_loc[n:])
        if W > 1:
            dist.all_gather_into_tensor(U_all, U_loc, group=self.group)
            dist.all_gather_into_tensor(cand_all, cand_loc, group=self.group)
        # (ids < 0 and items of other shards: ARX_KEY_NONE, a column of no shard)
        be.shard_route(cand_all.view(-1), W, self.rank, self.zero_row, None, cols.view(-1))
        ni = self.ni_loc
        be.slate_scores(U_all, self.E_item[:ni], self.b_item[:ni], cols, part)
        if W == 1:
            recv = part.view(1, B, C)
        else:
            _all_to_all(recv.view(B, C), part, group=self.group)
        be.slate_merge_shards(recv, merged)
        if k is not None:
            be.slate_order(merged, cand_loc, k, vo, pos, io)
        return merged, vo, io

    def _serve_latents(self, u, out):
        """The latents recommend / evaluate score against the item shard, for the users u (global ids this rank owns)
        -> out [len(u), d]: this model's are its user rows."""
        if len(u):
            rows = torch.from_numpy((u // self.world).astype(np.int32)).to(self.device)
            self.be.gather_rows(self.E_user, None, rows, out, None)

    # -------------------------------------------------------------- evaluate
    def prepare_eval_positives(self, item_sets):
        """The items evaluate('warp' / 'warp_eval') leaves out per user -- prepare_warp's pos_item_set_eval
        (embed_attribute.py:729-741).  A collective, routed and kept as prepare_recommend_exclusions' lists are:
        every rank passes the sets of users IT owns, {global user: global items} or a (users, ptr, items) CSR triple;
        an empty dict masks nothing.  A second call replaces the sets."""
        self._eval_pos = self._route_item_sets(item_sets, "eval positives", "eval positive lists")

    def evaluate(self, users, items, loss='warp', return_rows=False):
        """Full-vocabulary evaluation loss (run_hmf.py:280-337: model.step(..., forward_only=True) on the dev set) of
        the row-sharded model.  A collective: every rank calls it with the same loss.  users: global ids this rank
        owns, 0 <= n <= B_loc (n may differ between ranks); items: their held-out targets, global ids, one per user.
        Per row (user u, target i, t = U[u] . I[i] + b[i], x_j likewise over all n_items, P_u = u's eval positives):
          'warp'       log(1 + sum_{j not in P_u} relu(x_j - t + 1))     (embed_attribute.py:605-618, :729-741)
          'ce'         logsumexp_j x_j - t                                 (no mask)
          'warp_eval'  margin_rank = sum_{j not in P_u} relu(x_j - t + 1), true_rank = #{j not in P_u, j != i:
                       x_j > t} (:620-639; the target adds exactly 1 to the margin unless masked; ties do not count)
        'warp' / 'ce' return the global mean over all ranks' rows as a python float (nan without rows), with
        return_rows also this rank's float32 [n] rows on the device; 'warp_eval' returns (margin_rank float32 [n],
        true_rank int32 [n]) on the device.  'warp' / 'warp_eval' need prepare_eval_positives() first.

          gather          this rank's user rows -> [B_loc, d] (padding rows: zeros, key -1)
          all_gather      latents [B, d], user ids [B], targets [B]
          (local)         t: the target rows (non-owned: the shard's zero row) . latents; all_reduce(SUM) -> [B]
          (local)         this shard's partial per row over E_item[:ni] (backend.shard_eval: the fused eval GEMM, then
                          arx_eval_shard_reduce takes the masked local columns out)
          all_to_all      partials [B] (+ int32 counts) -> the ranks that own the rows: [W][B_loc]
          (local)         W-way combine, the loss per row (arx_eval_merge_shards); sum_scaled + all_reduce: the mean

        Eager (no capture); with graph segments on the model's stream, joined with the caller's on both sides as
        step() is.  Its buffers and GEMM workspace are its own."""
        W, r = self.world, self.rank
        if loss not in ('warp', 'ce', 'warp_eval'):
            raise ValueError("evaluate: loss must be 'warp', 'ce' or 'warp_eval', got %r" % (loss,))
        u = users.cpu().numpy() if isinstance(users, torch.Tensor) else np.asarray(users)
        it = items.cpu().numpy() if isinstance(items, torch.Tensor) else np.asarray(items)
        u, it = u.astype(np.int64).reshape(-1), it.astype(np.int64).reshape(-1)
        if len(u) != len(it):
            raise ValueError("evaluate: one target item per user (%d users, %d items)" % (len(u), len(it)))
        if len(u) > self.B_loc:
            raise ValueError("evaluate: at most B_loc = %d users per call and rank" % self.B_loc)
        if len(u) and (u.min() < 0 or u.max() >= self.n_users or np.any(u % W != r)):
            raise ValueError("evaluate: users must be global ids in [0, %d) owned by rank %d" % (self.n_users, r))
        if len(it) and (it.min() < 0 or it.max() >= self.n_items):
            raise ValueError("evaluate: item ids must lie in [0, %d)" % self.n_items)
        if loss != 'ce' and getattr(self, '_eval_pos', None) is None:
            raise ValueError("evaluate(loss=%r) needs prepare_eval_positives() first (an empty dict masks nothing)"
                             % loss)
        with _ops.joined(self._stream if self.use_graphs else None):
            rows_f, rows_i, sc = self._evaluate(u, it, loss)
        n = len(u)
        if loss == 'warp_eval':
            return rows_f[:n].clone(), rows_i[:n].clone()
        tot, cnt = (float(x) for x in sc.cpu().tolist())
        mean = tot / cnt if cnt > 0 else float('nan')
        return (mean, rows_f[:n].clone()) if return_rows else mean

    def _evaluate(self, u, it, loss):
        be, W, r, B_loc, B, d = self.be, self.world, self.rank, self.B_loc, self.B, self.d
        dev, f32, i32 = self.device, torch.float32, torch.int32
        n = len(u)
        if getattr(self, '_ev_buf', None) is None:
            e = lambda dt, *sh: torch.empty(sh, dtype=dt, device=dev)
            kl, ul, tl = torch.full((B_loc,), -1, dtype=i32, device=dev), torch.zeros((B_loc, d), dtype=f32,
                                                                                      device=dev), e(i32, B_loc)
            lat = (kl, ul, tl) + ((kl, ul, tl) if W == 1 else (e(i32, B), e(f32, B, d), e(i32, B)))
            # trow [B] (= the local target column; the zero row ni: not here), T [B, d], tb [B], t [B]; the shard's
            # partials [B] and counts; the received [W][B_loc]; the rows' results; (sum, count) of the mean
            self._ev_buf = lat + (e(i32, B), e(f32, B, d), e(f32, B), e(f32, B), e(f32, B), e(i32, B),
                                  e(f32, W, B_loc), e(i32, W, B_loc), e(f32, B_loc), e(i32, B_loc), e(f32, 2))
        (keys_loc, U_loc, tgt_loc, keys_all, U_all, tgt_all, trow, T, tb, t, part, cnt, recv_p, recv_c, rows_f,
         rows_i, sc) = self._ev_buf
        kh, th = np.full(B_loc, -1, dtype=np.int32), np.zeros(B_loc, dtype=np.int32)
        kh[:n], th[:n] = u, it
        keys_loc.copy_(torch.from_numpy(kh))
        tgt_loc.copy_(torch.from_numpy(th))
        self._serve_latents(u, U_loc[:n])
        if n < B_loc:
            be.fill_zero(U_loc[n:])
        if W > 1:
            dist.all_gather_into_tensor(U_all, U_loc, group=self.group)
            dist.all_gather_into_tensor(keys_all, keys_loc, group=self.group)
            dist.all_gather_into_tensor(tgt_all, tgt_loc, group=self.group)
        # the target logit: the owner's row, every other rank's zero row -- one non-zero summand per row (exact)
        be.shard_route(tgt_all, W, r, self.zero_row, trow, None)
        be.gather_rows(self.E_item, self.b_item, trow, T, tb)
        be.dot_score(U_all, T, tb, t)
        if W > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        ni = self.ni_loc
        ex = (keys_all, B, self._eval_pos[0], self._eval_pos[1]) if loss != 'ce' else None
        be.shard_eval(U_all, self.E_item[:ni], self.b_item[:ni], t, trow, loss, ex, part, cnt)
        if W == 1:
            recv_p, recv_c = part.view(1, B), cnt.view(1, B)
        else:
            _all_to_all(recv_p.view(B), part, group=self.group)
            if loss == 'warp_eval':
                _all_to_all(recv_c.view(B), cnt, group=self.group)
        wev = loss == 'warp_eval'
        be.eval_merge_shards(loss, recv_p, recv_c if wev else None, t[r * B_loc:(r + 1) * B_loc], rows_f,
                             rows_i if wev else None)
        if not wev:
            be.sum_scaled(rows_f[:n], 1.0, sc[:1])
            sc[1:].copy_(torch.tensor([float(n)], dtype=f32))
            dist.all_reduce(sc, op=dist.ReduceOp.SUM, group=self.group)
        return rows_f, rows_i, sc

    # ---- checkpoints (utils/checkpoint.py ShardedSaver) and the full gather of the tests ----
    def _checkpoint_arrays(self):
        """(name, tensor, global rows, layout) of every table and Adagrad slot ('<name>/Adagrad'); the tensors are the
        whole buffers, zero row included -- the saver takes the owned rows."""
        return [('user', self.E_user, self.n_users, 'rows'), ('user/Adagrad', self.A_user, self.n_users, 'rows'),
                ('item', self.E_item, self.n_items, 'rows'), ('item/Adagrad', self.A_item, self.n_items, 'rows'),
                ('item_bias', self.b_item, self.n_items, 'rows'),
                ('item_bias/Adagrad', self.Ab_item, self.n_items, 'rows')]

    def _token_arrays(self, layout):
        return [('token', self.E_tok, self.n_tokens, layout), ('token/Adagrad', self.A_tok, self.n_tokens, layout),
                ('token_bias', self.b_tok, self.n_tokens, layout),
                ('token_bias/Adagrad', self.Ab_tok, self.n_tokens, layout)]

    def _checkpoint_scalars(self):
        sc = {'steps': int(self.steps), 'learning_rate': float(self.lr.item()), 'd': int(self.d),
              'n_users': int(self.n_users), 'n_items': int(self.n_items)}
        if hasattr(self, 'n_tokens'):
            sc['n_tokens'] = int(self.n_tokens)
        # the loss that trained the tables (a note: they restore into a model of any loss) and the pair draw's counter
        sc['loss'] = self.loss_name
        sc['n_draws'] = int(self.n_draws)
        return sc

    def _checkpoint_set_scalars(self, sc):
        self.steps = int(sc['steps'])
        self.lr.fill_(float(sc['learning_rate']))           # (in place: captured graphs read this word)
        self.n_draws = int(sc.get('n_draws', self.n_draws)) # (a manifest from before the pair losses has none)

    def _checkpoint_restored(self):
        self.n_restores += 1                                # every ShardedHetView of this model is stale now

    def gather_global_tables(self, slots=False):
        """Reassemble the striped tables on every rank (tests only; O(table)); slots: the Adagrad slots too, as
        '<name>/Adagrad'.  (Checkpoints do not come this way: model.saver writes each rank's rows.)"""
        W = self.world
        out = {}
        for name, t, n, layout in self._checkpoint_arrays():
            if name.endswith('/Adagrad') and not slots:
                continue
            if layout == 'replicated':
                out[name] = t[:n].cpu().numpy()
                continue
            t = t[:(n - self.rank + W - 1) // W]
            rows = (n + W - 1) // W
            pad = torch.zeros((rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            pad[:t.shape[0]] = t
            parts = [torch.empty_like(pad) for _ in range(W)]
            dist.all_gather(parts, pad, group=self.group)
            full = torch.stack(parts, 1).reshape((rows * W,) + tuple(t.shape[1:]))[:n]
            out[name] = full.cpu().numpy()
        return out


W2V_TABLES = ('userembed_cat_0', 'itemembed_cat_0', 'item_outputembed_cat_0', 'item_output_bias_cat_0')


class ShardedW2V(ShardedHMF):
    """The id-only skip-gram / CBOW recommender (word2vec/linear_seq.py LinearSeq, use_sep_item=True) with row-sharded
    tables: the user table, the CONTEXT (input) item table without bias and the OUTPUT item table with bias, all
    striped by id % world; the context shard has its own padding (zero) row.  A batch row is (user, n_input context
    items, target) and its model input is
        CBOW, train and test:   x = 0.5 u + (0.5 / n) sum_t C[ctx_t]
        skip-gram, train:       x = 0.5 u + 0.5 C[ctx_0]          (test: the CBOW form)
    The pool logits, the target score, the positive mask, the loss ('mw' | 'mce'), gscale = 1 / B of the global batch
    and read_loss() are ShardedHMF's with x in the place of the user row; du = 0.5 dx and context position t gets
    w_t dx (0.5 / n; skip-gram training: 0.5 for t = 0 and nothing else).

    tables / checkpoint arrays carry the names the single-process model gives these tables -- 'userembed_cat_0',
    'itemembed_cat_0' (context), 'item_outputembed_cat_0', 'item_output_bias_cat_0' -- with one row per id (the
    single-process tables without their two reserved leading rows).

    The context rows of a batch live on any ranks, so they are routed like the two rows of a pair step
    (_prepare_route_pair): the n B_loc requests (skip-gram training: the B_loc of t = 0) are ordered by owner, the
    rows come back in that order and every (t, b) knows the SLOT of its row in the received block.  One slot serves one
    request: an item asked for twice travels twice and K7 merges its gradient rows.  The step IS
    ShardedHMF._step_body: this class overrides its hooks and adds one more gather site, one more pair of all-to-alls
    and the two slot-addressed window kernels (arx_window_slots_fwd / _bwd); K7 is one pass over the three tables.

      fwd_gather   + one site: the requested context rows -> the packed send block [cap_c, d]
      all_to_all   context rows out, in request order (asynchronous, beside the target-row exchange)
      fwd_score    arx_window_slots_fwd: X = 0.5 U_loc + w sum_t C_pack[slot(t, b)]; then the scorer on X
      loss, bwd_gemms   as ShardedHMF with X / dX for U_loc / dU; then arx_window_slots_bwd: 0.5 dX into the
                   arena's user rows, w dX into the n slots of the gradient block
      all_to_all   context gradient rows back to their owners, into the arena behind the received target rows
      apply        ONE sparse_adagrad_multi over the three tables: user rows, pool, received targets, received
                   context rows

    The per-batch vectors -- [user rows ; received target rows (cap_r) ; received context rows (cap_c)], padded with
    the shard's zero row, and the slots -- are fed by the first node.

    loss: 'mw' | 'mce'; exchange: 'rows'; n_input >= 1 (ValueError otherwise).  Out of scope: use_sep_item=False (one
    shared item table), multi-hot or several features per entity, output_feat != 1, dropout, n_input_items = 0."""

    def __init__(self, n_users, n_items, d, B_loc, S, n_input, learning_rate, rank, world, device, cbow=True,
                 loss='mw', tables=None, backend=None, group=None, seed=0, acc0=0.1, graphs=None, exchange='rows'):
        if loss not in ('mw', 'mce'):
            raise ValueError("ShardedW2V: loss is 'mw' or 'mce' (the sampled losses of this family), got %r" % (loss,))
        if exchange != 'rows':
            raise ValueError("ShardedW2V: exchange='rows' only (the window's rows travel, not the logits), got %r"
                             % (exchange,))
        if int(n_input) < 1:
            raise ValueError("ShardedW2V: n_input >= 1 context items per row, got %r" % (n_input,))
        if d > 256:
            raise ValueError("ShardedW2V: d <= 256 (the window kernels)")
        self.n_input, self.cbow = int(n_input), bool(cbow)
        # rows of the window a TRAINING row asks for, and their weight in x
        self.n_train = self.n_input if self.cbow else 1
        self.cap_c = 0                                      # capacity for received context requests
        t = None
        if tables is not None:
            missing = [k for k in W2V_TABLES if k not in tables]
            if missing:
                raise ValueError("ShardedW2V: tables lacks %s" % ', '.join(missing))
            t = {'user': tables['userembed_cat_0'], 'item': tables['item_outputembed_cat_0'],
                 'item_bias': tables['item_output_bias_cat_0']}
        super().__init__(n_users, n_items, d, B_loc, S, learning_rate, rank, world, device, backend=backend,
                         group=group, tables=t, seed=seed, acc0=acc0, graphs=graphs, exchange='rows', loss=loss)
        dev, f32, ni = self.device, torch.float32, self.ni_loc
        if tables is not None:
            C = np.asarray(tables['itemembed_cat_0'], dtype=np.float32)[rank::world]
            self.E_ctx = torch.zeros((ni + 1, d), dtype=f32, device=dev)
            self.E_ctx[:ni].copy_(torch.from_numpy(np.ascontiguousarray(C)))
        else:
            g = torch.Generator(device=dev)
            g.manual_seed(seed * 1009 + rank + 500009)
            lim = float(np.sqrt(6.0 / (n_items + 2 + d)))
            self.E_ctx = torch.empty((ni + 1, d), dtype=f32, device=dev).uniform_(-lim, lim, generator=g)
            self.E_ctx[ni].zero_()
        self.A_ctx = torch.full_like(self.E_ctx, self.acc0)
        n_req = self.n_train * B_loc
        self.X = torch.zeros((B_loc, d), dtype=f32, device=dev)              # the model input, its gradient
        self.dX = torch.zeros((B_loc, d), dtype=f32, device=dev)
        self.C_pack = torch.zeros((n_req, d), dtype=f32, device=dev)         # context rows as received, by slot
        self.dC_pack = torch.zeros((n_req, self.dp), dtype=f32, device=dev) if world > 1 else None
        self.g_cslots = torch.zeros((n_req,), dtype=torch.int32, device=dev)
        self._serve_ctx = None
        self._alloc_recv(self.cap_r, n_req)

    def _alloc_recv(self, cap, cap_c=0):
        """ShardedHMF's buffers, and what scales with the context requests this rank serves: the arena is
        [dU_loc (B_loc) ; dI_g (Sg) ; received dT (cap_r) ; received context gradient rows (cap_c)]."""
        cap_r0, cap_c0 = self.cap_r, self.cap_c
        super()._alloc_recv(cap)
        if cap_c > cap_c0:
            if self.use_graphs and cap_c0 > 0:
                cap_c = (cap_c + cap_c // 8 + 63) // 64 * 64
            self.cap_c = cap_c
            self.C_send = torch.zeros((cap_c, self.d), dtype=torch.float32, device=self.device)
        if self.cap_r != cap_r0 or self.cap_c != cap_c0:
            rows = self.B_loc + self.Sg + self.cap_r + self.cap_c
            self.arena = torch.zeros((rows, self.dp), dtype=torch.float32, device=self.device)
            self.arena_b = torch.zeros((rows,), dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ route
    def _context_array(self, context, m, what):
        c = context.cpu().numpy() if isinstance(context, torch.Tensor) else np.asarray(context)
        c = c.astype(np.int64)
        if c.size != self.n_input * m:
            raise ValueError("%s: context is [n_input = %d][%d] (time-major), got %s"
                             % (what, self.n_input, m, tuple(np.shape(context))))
        c = c.reshape(self.n_input, m)
        if c.size and (c.min() < 0 or c.max() >= self.n_items):
            raise ValueError("%s: context ids must lie in [0, %d)" % (what, self.n_items))
        return c

    def _route_context(self, ctx):
        """The requests ctx [n_win][m] (time-major) of this rank, ordered by owner: one count exchange and one id
        exchange resolve them to local rows of the owners' context shards; cslots[t * m + b] = the row of request
        (t, b) in the block that comes back."""
        r, slot = self._route_requests(ctx.reshape(-1).astype(np.int32))[:2]
        return {'cslots': torch.from_numpy(slot).to(self.device), 'csend': r['send'], 'crecv': r['recv'],
                'Rc': r['R'], 'crecv_rows': r['recv_rows'], 'n_win': int(ctx.shape[0]), 'n_req': int(ctx.size)}

    def prepare_route(self, users, items, context):
        """ShardedHMF.prepare_route for (users, targets) -- the batch ordered by the target's owner -- with the
        context columns permuted alongside and the window's requests routed by slot (_route_context).  context:
        [n_input][B_loc], time-major, as LinearSeq.step takes item_input; a skip-gram model asks for row t = 0 only.
        Ids outside [0, n_items) raise before anything is sent."""
        B_loc = self.B_loc
        u = users.cpu().numpy() if isinstance(users, torch.Tensor) else np.asarray(users)
        it = items.cpu().numpy() if isinstance(items, torch.Tensor) else np.asarray(items)
        u, it = u.astype(np.int32).reshape(-1), it.astype(np.int32).reshape(-1)
        if len(u) != B_loc or len(it) != B_loc:
            raise ValueError("prepare_route: B_loc = %d users and items per rank" % B_loc)
        if it.min() < 0 or it.max() >= self.n_items:
            raise ValueError("prepare_route: item ids must lie in [0, %d)" % self.n_items)
        ctx = self._context_array(context, B_loc, "prepare_route")
        perm = owner_order(it, self.world)[0]
        route = super().prepare_route(u[perm], it[perm])         # (sorted already: its own stable sort keeps the order)
        ctx = ctx[:, perm]
        route['context'] = torch.from_numpy(np.ascontiguousarray(ctx.astype(np.int32))).to(self.device)
        route.update(self._route_context(ctx[:self.n_train]))
        self._alloc_recv(route['R'], route['Rc'])
        return route

    def step(self, users, items=None, context=None):
        """One training step: a route of prepare_route(), or (users, items, context), routed here."""
        if self.world > 1 and self.cap <= 0:
            raise RuntimeError("ShardedW2V.step before set_pool(): the pool's block layout sizes the exchanges")
        route = users if isinstance(users, dict) else self.prepare_route(users, items, context)
        self._run_step(route)

    # ------------------------------------------- step: what ShardedHMF._step_body takes from this class
    # World 1: the context rows are gathered straight into the block the window kernel reads and their gradient rows
    # written straight into the arena.  Arena rows behind the received requests carry the padding key: K7 drops them.
    def _step_blocks(self, route):
        if route.get('n_win') != self.n_train:
            raise ValueError("step: the route asks for %r window rows, a training step of this model for %d"
                             % (route.get('n_win'), self.n_train))
        if route['R'] > self.cap_r or route['Rc'] > self.cap_c:
            self._alloc_recv(route['R'], route['Rc'])
        return [(route['recv_rows'], self.cap_r), (route['crecv_rows'], self.cap_c)]

    def _static_feeds(self, route, cap_r):
        return [(route['cslots'], self.g_cslots)]

    def _key_more(self):
        return (self.cap_c, self.C_send.data_ptr(), self.g_cslots.data_ptr())

    def _ctx(self):
        """(rows to look up, the block they are gathered into, their gradient block, its row in the arena): the
        context requests this rank serves."""
        B_loc, n_req = self.B_loc, self.n_train * self.B_loc
        base_c = B_loc + self.Sg + self.cap_r
        crows = self.g_idx[B_loc + self.cap_r:]
        if self.world == 1:
            return crows[:n_req], self.C_pack, self.arena[base_c:base_c + n_req], base_c
        return crows, self.C_send[:self.cap_c], self.dC_pack, base_c

    def _gather(self, urows, rrows, T_in):
        crows, C_in = self._ctx()[:2]
        super()._gather(urows, rrows, T_in, [(self.E_ctx, None, crows, C_in, None)])

    def _k7(self, phase, urows, rrows):
        ni = self.ni_loc
        crows, _, _, base_c = self._ctx()
        super()._k7(phase, urows, rrows, [(self.E_ctx[:ni], self.A_ctx[:ni], None, None)], [(2, crows, base_c)])

    def _scorer_io(self):
        return self.X, self.dX

    def _input_fwd(self):      # arx_window_slots_fwd: X = 0.5 U_loc + w sum_t C_pack[slot(t, b)]
        n = self.n_train
        self.be.window_slots_fwd(self.C_pack, self.g_cslots, n, 0.5 / n, self.U_loc, 0.5, self.X)

    def _input_bwd(self):      # dX -> 0.5 dX into the user rows of the arena, w dX into the window's slots
        n, d = self.n_train, self.d
        self.be.window_slots_bwd(self.dX, self.g_cslots, n, 0.5 / n, 0.5, self.arena[:self.B_loc, :d], False,
                                 self._ctx()[2][:, :d])

    def _send_input_rows(self, route):         # context rows out, in request order
        _all_to_all(self.C_pack[:self.n_train * self.B_loc], self.C_send[:route['Rc']], route['csend'],
                    route['crecv'], group=self.group, async_op=True).wait()

    def _return_input_grads(self, route):      # context gradient rows back, into the arena behind the target rows
        base_c = self.B_loc + self.Sg + self.cap_r
        return _all_to_all(self.arena[base_c:base_c + route['Rc']], self.dC_pack[:self.n_train * self.B_loc],
                           route['crecv'], route['csend'], group=self.group, async_op=True)

    # ---------------------------------------------------------------- serving
    def _serve_latents(self, u, out):
        """x_test = 0.5 u + (0.5 / n) sum_t C[ctx_t] over the FULL window (skip-gram too), eagerly: the window's
        requests are routed (a collective, like the calls that use it), the rows cross and the forward window
        kernel forms the latents."""
        be, W, d, n, m = self.be, self.world, self.d, self.n_input, len(u)
        f32, dev = torch.float32, self.device
        ctx = self._serve_ctx
        r = self._route_context(ctx)
        send_blk = torch.zeros((max(r['Rc'], 1), d), dtype=f32, device=dev)
        if r['Rc'] > 0:
            be.gather_rows(self.E_ctx, None, r['crecv_rows'], send_blk[:r['Rc']], None)
        if W == 1:
            block = send_blk
        else:
            block = torch.zeros((max(r['n_req'], 1), d), dtype=f32, device=dev)
            _all_to_all(block[:r['n_req']], send_blk[:r['Rc']], r['csend'], r['crecv'], group=self.group)
        if m:
            base = torch.zeros((m, d), dtype=f32, device=dev)
            super()._serve_latents(u, base)
            be.window_slots_fwd(block, r['cslots'], n, 0.5 / n, base, 0.5, out)

    def recommend(self, users, context, k, exclude_seen=False, return_values=False, tags_any=None, tags_all=None):
        """ShardedHMF.recommend over x_test of (users, context): context is [n_input][len(users)], time-major."""
        return self.recommend_sampled(users, context, k, exclude_seen=exclude_seen, return_values=return_values,
                                      tags_any=tags_any, tags_all=tags_all)

    def recommend_sampled(self, users, context, k, exclude_seen=False, return_values=False, tags_any=None,
                          tags_all=None, sample_temperature=None, sample_seed=None, return_logprob=False):
        """ShardedHMF.recommend_sampled over x_test of (users, context).  The sampled recommend's noise row is the USER
        id: two rows of the same user in one call share their noise."""
        u = users.cpu().numpy() if isinstance(users, torch.Tensor) else np.asarray(users)
        self._serve_ctx = self._context_array(context, int(u.size), "recommend")
        try:
            return super().recommend_sampled(users, k, exclude_seen=exclude_seen, return_values=return_values,
                                             tags_any=tags_any, tags_all=tags_all,
                                             sample_temperature=sample_temperature, sample_seed=sample_seed,
                                             return_logprob=return_logprob)
        finally:
            self._serve_ctx = None

    def list_logprob(self, users, context, lists, sample_temperature, exclude_seen=False, tags_any=None, tags_all=None,
                     return_values=False, return_why=False):
        """ShardedHMF.list_logprob over x_test of (users, context): context is [n_input][len(users)], time-major."""
        u = users.cpu().numpy() if isinstance(users, torch.Tensor) else np.asarray(users)
        self._serve_ctx = self._context_array(context, int(u.size), "list_logprob")
        try:
            return super().list_logprob(users, lists, sample_temperature, exclude_seen=exclude_seen, tags_any=tags_any,
                                        tags_all=tags_all, return_values=return_values, return_why=return_why)
        finally:
            self._serve_ctx = None

    def score_items(self, users, context, candidates, k=None):
        """ShardedHMF.score_items over x_test of (users, context): context is [n_input][len(users)], time-major."""
        u = users.cpu().numpy() if isinstance(users, torch.Tensor) else np.asarray(users)
        self._serve_ctx = self._context_array(context, int(u.size), "score_items")
        try:
            return super().score_items(users, candidates, k=k)
        finally:
            self._serve_ctx = None

    def evaluate(self, users, context, items, loss='warp', return_rows=False):
        """ShardedHMF.evaluate over x_test of (users, context): context is [n_input][len(users)], time-major."""
        u = users.cpu().numpy() if isinstance(users, torch.Tensor) else np.asarray(users)
        self._serve_ctx = self._context_array(context, int(u.size), "evaluate")
        try:
            return super().evaluate(users, items, loss=loss, return_rows=return_rows)
        finally:
            self._serve_ctx = None

    def _checkpoint_arrays(self):
        nu, ni = self.n_users, self.n_items
        return [('userembed_cat_0', self.E_user, nu, 'rows'), ('userembed_cat_0/Adagrad', self.A_user, nu, 'rows'),
                ('itemembed_cat_0', self.E_ctx, ni, 'rows'), ('itemembed_cat_0/Adagrad', self.A_ctx, ni, 'rows'),
                ('item_outputembed_cat_0', self.E_item, ni, 'rows'),
                ('item_outputembed_cat_0/Adagrad', self.A_item, ni, 'rows'),
                ('item_output_bias_cat_0', self.b_item, ni, 'rows'),
                ('item_output_bias_cat_0/Adagrad', self.Ab_item, ni, 'rows')]


class ShardedHMFBags(ShardedHMF):
    """ShardedHMF with HET items (comb_attribute.py:151-176): item = mean(id row, bag mean) of an id
    feature and ONE multi-hot attribute -- the id table striped by item as before, the TOKEN table
    striped by token (owner = token % world).  An item's tokens live on several
    ranks, so every rank forms its PARTIAL of every embedding the step needs -- half its own id row
    (zeros where it does not own the item) plus half the bag mean restricted to its own tokens --
    and the partials are summed by the collective that distributes them:

      all_reduce      pool partials [S, d+4]                      -> the S pool embeddings, everywhere
      reduce_scatter  target partials [B, d+4] -> [B_loc, d+4]    -> each rank's own target embeddings
      (local)         logits, WMRB loss, dU, user-shard rows      (as ShardedHMF)
      all_reduce      pool-gradient partials [S, d+4]             -> the pool gradient, everywhere
      all_gather      target-row gradients [B_loc, d+4] -> [B, d+4]
      (local)         one fused one-hot pass (user shard; id shard: pool + ALL B targets, rows of other
                      owners dropped, coefficient 1/2) and one two-stage bag pass over the token shard
                      (tokens of other owners dropped, coefficient 1/2 . 1/len)

    No all_to_all is left on the path; the target ids of the global batch are all-gathered with the
    batch (prepare_route: input data).  The bag index (vals / starts / lens, global item ids, global
    token ids) is replicated; each rank keeps a copy of `vals` in which its own tokens are local rows
    and every other token points at the shard's padding row (forward: adds zeros; backward: out of
    range, dropped by the sort).  Volume per rank and step: 2 x B x (d+4) x 4 bytes through the
    reduce_scatter / all_gather (B = global batch) -- the price of token sharding; the id-only step
    moves 2 x B_loc x (d+4) x 4."""

    def __init__(self, n_users, n_items, d, B_loc, S, learning_rate, rank, world, device, bags, n_tokens,
                 backend=None, group=None, tables=None, seed=0, acc0=0.1, graphs=None, loss='mw'):
        super().__init__(n_users, n_items, d, B_loc, S, learning_rate, rank, world, device, backend=backend,
                         group=group, tables=tables, seed=seed, acc0=acc0, graphs=graphs, loss=loss)
        dev, f32, i32 = self.device, torch.float32, torch.int32
        vals, starts, lens = [np.asarray(a) for a in bags]
        nt = (n_tokens - rank + world - 1) // world
        self.n_tokens, self.nt_loc = n_tokens, nt
        if tables is not None:
            T = np.asarray(tables['token'], dtype=np.float32)[rank::world]
            bT = np.asarray(tables['token_bias'], dtype=np.float32).reshape(-1)[rank::world]
            self.E_tok = torch.zeros((nt + 1, d), dtype=f32, device=dev)
            self.E_tok[:nt].copy_(torch.from_numpy(np.ascontiguousarray(T)))
            self.b_tok = torch.zeros((nt + 1,), dtype=f32, device=dev)
            self.b_tok[:nt].copy_(torch.from_numpy(np.ascontiguousarray(bT)))
        else:
            g = torch.Generator(device=dev)
            g.manual_seed(seed * 2003 + rank)
            lim = float(np.sqrt(6.0 / (n_tokens + d)))
            self.E_tok = torch.empty((nt + 1, d), dtype=f32, device=dev).uniform_(-lim, lim, generator=g)
            self.b_tok = torch.empty((nt + 1,), dtype=f32, device=dev).uniform_(-lim, lim, generator=g)
            self.E_tok[nt].zero_()
            self.b_tok[nt] = 0.0
        self.A_tok = torch.full_like(self.E_tok, acc0)
        self.Ab_tok = torch.full_like(self.b_tok, acc0)
        v = vals.astype(np.int64)
        mine = np.where(v % world == rank, v // world, nt).astype(np.int32)      # other owners -> padding row
        self.bag_vals = torch.from_numpy(np.ascontiguousarray(mine)).to(dev)
        self.bag_starts = torch.from_numpy(np.ascontiguousarray(starts.astype(np.int32))).to(dev)
        self.bag_lens = torch.from_numpy(np.ascontiguousarray(lens.astype(np.int32))).to(dev)
        B, dp = self.B, self.dp
        z = lambda *s_: torch.zeros(s_, dtype=f32, device=dev)
        self.P_part, self.Pb = z(S, dp), z(S)               # pool partials -> (all_reduce) pool embeddings
        self.T_part, self.Tb = z(B, dp), z(B)               # target partials of the GLOBAL batch
        self.pool_fwd = torch.zeros(S, dtype=i32, device=dev)    # id-shard row of every pool slot (padding row: not mine)
        self.pool_bwd = torch.zeros(S, dtype=i32, device=dev)    # ... or KEY_NONE
        self.arena = z(B_loc + S + B, dp)                   # [dU_loc ; pool gradient ; target gradients of the batch]
        self.arena_b = z(B_loc + S + B)

    def _alloc_recv(self, cap):
        return                                              # (no variable-size exchange in this step)

    def set_pool(self, pool_ids):
        super().set_pool(pool_ids)
        self.be.shard_route(self.pool_ids, self.world, self.rank, self.zero_row, self.pool_fwd, self.pool_bwd)

    def prepare_route(self, users, items):
        W = self.world
        dev = self.device
        u = users if isinstance(users, torch.Tensor) else torch.as_tensor(np.asarray(users, dtype=np.int32))
        it = items if isinstance(items, torch.Tensor) else torch.as_tensor(np.asarray(items, dtype=np.int32))
        u, it = u.to(dev, torch.int32), it.to(dev, torch.int32)
        tgt_all = torch.empty(self.B, dtype=torch.int32, device=dev)
        dist.all_gather_into_tensor(tgt_all, it.contiguous(), group=self.group)   # target ids of the global batch
        fwd = torch.zeros(self.B, dtype=torch.int32, device=dev)
        bwd = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.be.shard_route(tgt_all, W, self.rank, self.zero_row, fwd, bwd)
        urows = torch.zeros(self.B_loc, dtype=torch.int32, device=dev)
        self.be.shard_route(u, W, self.rank, 0, urows, None)
        return {'users': u, 'items': it, 'urows': urows, 'tgt_all': tgt_all, 'tgt_fwd': fwd, 'tgt_bwd': bwd}

    def _step_body(self, route):
        """The step as segments between its four collectives (ShardedHMF._run_step drives them).  Every buffer is
        static; what varies from batch to batch are four index vectors (user rows, the global batch's target ids and
        their id-shard rows / keys), fed by the first node of the first segment.  K7's ids-only half (both one-hot
        sorts, the entity and token sorts of the bag pass) runs on a second stream under the forward kernels -- a
        graph of its own between the segments, a branch of the ONE graph at world 1 -- and the scorer is the fused
        bf16-pipe family where its shapes allow (no [B_loc, S] logits), as in ShardedHMF._step_body."""
        be, grp, W = self.be, self.group, self.world
        B, B_loc, S, d = self.B, self.B_loc, self.S, self.d
        dev = self.device
        arena, arena_b = self.arena, self.arena_b
        if getattr(self, 'g_urows', None) is None:
            i32 = torch.int32
            self.g_urows = torch.zeros(B_loc, dtype=i32, device=dev)
            self.g_fwd, self.g_all, self.g_bwd = (torch.zeros(B, dtype=i32, device=dev) for _ in range(3))
        urows, t_fwd, t_all, t_bwd = self.g_urows, self.g_fwd, self.g_all, self.g_bwd
        self.urows = urows
        feed = [(route['urows'], urows), (route['tgt_fwd'], t_fwd), (route['tgt_all'], t_all), (route['tgt_bwd'], t_bwd)]
        key = (arena.data_ptr(), self.pos_ptr.data_ptr(), self.pos_items.data_ptr(), urows.data_ptr())
        bag = (self.bag_vals, self.bag_starts, self.bag_lens)
        dU = arena[:B_loc, :d]
        gP = arena[B_loc:B_loc + S]
        nt = self.nt_loc
        fused = self._fused_scorer()

        def fwd_pool():        # partial embeddings, summed by the collectives
            be.gather_rows(self.E_user, None, urows, self.U_loc, None)
            be.gather_rows(self.E_item, self.b_item, self.pool_fwd, self.P_part[:, :d], self.Pb, scale=0.5)
            be.gather_bags(self.E_tok, self.b_tok, *bag, self.pool_ids, self.P_part[:, :d], self.Pb, scale=0.5,
                           accumulate=True)
            be.copy_strided(self.Pb, self.P_part[:, d])

        def fwd_tgt():
            be.gather_rows(self.E_item, self.b_item, t_fwd, self.T_part[:, :d], self.Tb, scale=0.5)
            be.gather_bags(self.E_tok, self.b_tok, *bag, t_all, self.T_part[:, :d], self.Tb, scale=0.5, accumulate=True)
            be.copy_strided(self.Tb, self.T_part[:, d])

        def score():
            be.copy_strided(self.P_part[:, d], self.b_all)
            if not fused:
                be.gemm(self.U_loc, self.P_part[:, :d], self.logits, transB=True, col_bias=self.b_all)

        def loss():
            self._scorer_loss(fused, self.U_loc, self.P_part[:, :d], urows, self.dT_pack[:, d], dU,
                              self.dT_pack[:, :d])

        def bwd():
            self._scorer_bwd(fused, self.U_loc, self.P_part[:, :d], dU, gP[:, :d], self.gb_all)
            be.copy_strided(self.gb_all, gP[:, d])

        def k7(phase):
            # id shard + user shard: one fused one-hot pass (rows of other owners carry KEY_NONE); token shard: merge
            # per item, then per token -- tokens of other owners are out of range
            be.sparse_adagrad_multi([(self.E_user, self.A_user, None, None),
                                     (self.E_item, self.A_item, self.b_item, self.Ab_item)],
                                    [(0, urows, 0, 1.0), (1, self.pool_bwd, B_loc, 0.5), (1, t_bwd, B_loc + S, 0.5)],
                                    arena[:, :d], arena_b, self.lr, phase=phase)
            be.bags_adagrad(self.E_tok[:nt], self.A_tok[:nt], self.b_tok[:nt], self.Ab_tok[:nt], *bag,
                            [(self.pool_ids, B_loc, 0.5), (t_all, B_loc + S, 0.5)], arena[:, :d], arena_b, self.lr,
                            phase=phase)

        def apply():
            be.copy_strided(arena[B_loc:, d], arena_b[B_loc:])
            k7(_ops.K7_APPLY)

        def body(mode):
            seg = lambda name, fn, feeds=None: self._segment(mode, name, fn, feeds)

            def whole_step():
                fwd_pool()
                sorted_ = self._k7_sorts(mode, k7, False)
                fwd_tgt()
                be.copy_2d(self.T_part, self.T_pack)          # (one rank: the partials ARE the embeddings)
                score()
                loss()
                be.copy_2d(self.dT_pack, arena[B_loc + S:])
                bwd()
                self._k7_join(sorted_)
                apply()

            if W == 1:
                return seg('step', whole_step, feed)
            seg('fwd_pool', fwd_pool, feed)
            sorted_ = self._k7_sorts(mode, k7, True)
            w_pool = dist.all_reduce(self.P_part, op=dist.ReduceOp.SUM, group=grp, async_op=True)
            seg('fwd_tgt', fwd_tgt)                               # target partials under the pool all-reduce
            w_pool.wait()
            w_tgt = dist.reduce_scatter_tensor(self.T_pack, self.T_part, op=dist.ReduceOp.SUM, group=grp, async_op=True)
            seg('score', score)                                   # (unfused scorer: its GEMM under the reduce-scatter)
            w_tgt.wait()
            seg('loss', loss)
            w_dt = dist.all_gather_into_tensor(arena[B_loc + S:], self.dT_pack, group=grp, async_op=True)
            seg('bwd', bwd)                                       # dU, pool gradient under the all-gather
            dist.all_reduce(gP, op=dist.ReduceOp.SUM, group=grp)
            w_dt.wait()
            self._k7_join(sorted_)
            seg('apply', apply)

        return key, body

    def item_view(self, chunk_cols=16384):
        """A serving view of this model (ShardedHetView): recommend / evaluate over its materialised item latents."""
        return ShardedHetView(self, chunk_cols=chunk_cols)

    def recommend(self, users, k, exclude_seen=False, return_values=False):
        """Not on the training class: the item latents are bag means -- item_view() materialises them per shard."""
        raise NotImplementedError("%s.recommend: item latents are bag means -- use item_view().recommend"
                                  % type(self).__name__)

    def recommend_sampled(self, *args, **kwargs):
        """Not on the training class either: item_view().recommend_sampled."""
        raise NotImplementedError("%s.recommend_sampled: item latents are bag means -- use "
                                  "item_view().recommend_sampled" % type(self).__name__)

    def list_logprob(self, *args, **kwargs):
        """Not on the training class either: item_view().list_logprob."""
        raise NotImplementedError("%s.list_logprob: item latents are bag means -- use "
                                  "item_view().list_logprob" % type(self).__name__)

    def similar_items(self, items, k, include_self=False, return_values=False):
        """ShardedHMF.similar_items over the materialised item latents 1/2 (id row + bag mean): through a serving view
        (item_view()) this model keeps for the purpose -- it refreshes when the model has stepped or been restored."""
        if getattr(self, '_sim_view', None) is None:
            self._sim_view = self.item_view()
        return self._sim_view.similar_items(items, k, include_self=include_self, return_values=return_values)

    def score_items(self, users, candidates, k=None):
        """Not on the training class: the item latents are bag means -- item_view() materialises them per shard."""
        raise NotImplementedError("%s.score_items: item latents are bag means -- use item_view().score_items"
                                  % type(self).__name__)

    def evaluate(self, users, items, loss='warp', return_rows=False):
        """Not on the training class: the item latents are bag means -- item_view() materialises them per shard."""
        raise NotImplementedError("%s.evaluate: item latents are bag means -- use item_view().evaluate"
                                  % type(self).__name__)

    def _checkpoint_arrays(self):
        return super()._checkpoint_arrays() + self._token_arrays('rows')


class ShardedHMFRepTokens(ShardedHMF):
    """HET items (comb_attribute.py:151-176: item = mean(id row, bag mean)) with the id table striped by item and
    the TOKEN table REPLICATED on every rank -- round 5, the redesign of ShardedHMFBags for token tables that fit
    beside the id shard (C3: 100 k x 128 x 4 B = 51 MB; past ~64 MB stripe by token: ShardedHMFBags).

    With every token on every rank a bag mean is LOCAL to the owner of the item's id row, so the step is
    ShardedHMF's -- the owner forms the whole item embedding, pool blocks are all-gathered, target rows and their
    gradients travel in two all-to-alls sized by B_loc, the pool gradient in one small all-reduce -- plus ONE
    all-reduce for the token table: every rank merges the token gradients of the lookups it owns (pool block +
    received targets, coefficient 1/2 . 1/len) into a dense gradient table D [n_tokens, d] (the two-stage bag pass
    in its gradient-descent form with a step of -1 onto a zeroed table: the sums themselves), D is summed over the
    ranks, and every replica applies the same Adagrad step to the rows of D that are not all zero (rows without gradient
    would not move: the sparse update of embed_attribute.py:383-400 / hmf_model.py:146-151; arx_adagrad_rows_nonzero,
    which also zeroes D for the next step).  Volume per rank and step on top of
    ShardedHMF: 2 x n_tokens x (d + 1) x 4 B x (N-1)/N through the ring, independent of the batch.  The two
    all-reduces run on the main stream between the 'apply' and 'tok_apply' segments -- NOT overlapped with K7, and
    priced so in roofline_comm_predicted (comm_prediction 'rep_tokens').  The token-striped step moves
    2 x B x (d + 4) x 4 B with B the GLOBAL batch
    (predicted comm / compute 0.35 against 0.57 at N = 8, B_loc = 16384)."""

    def __init__(self, n_users, n_items, d, B_loc, S, learning_rate, rank, world, device, bags, n_tokens,
                 backend=None, group=None, tables=None, seed=0, acc0=0.1, graphs=None, loss='mw'):
        super().__init__(n_users, n_items, d, B_loc, S, learning_rate, rank, world, device, backend=backend,
                         group=group, tables=tables, seed=seed, acc0=acc0, graphs=graphs, loss=loss)
        dev, f32, i32 = self.device, torch.float32, torch.int32
        vals, starts, lens = [np.asarray(a) for a in bags]
        nt = int(n_tokens)
        self.n_tokens = nt
        self.g_gid = None               # received target ids (global), padded with the padding entity: fed per step
        if tables is not None:
            self.E_tok = torch.zeros((nt + 1, d), dtype=f32, device=dev)
            self.E_tok[:nt].copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(tables['token'], dtype=np.float32))))
            self.b_tok = torch.zeros((nt + 1,), dtype=f32, device=dev)
            self.b_tok[:nt].copy_(torch.from_numpy(np.ascontiguousarray(
                np.asarray(tables['token_bias'], dtype=np.float32).reshape(-1))))
        else:
            g = torch.Generator(device=dev)
            g.manual_seed(seed * 2003)                      # (the SAME table on every rank)
            lim = float(np.sqrt(6.0 / (nt + d)))
            self.E_tok = torch.empty((nt + 1, d), dtype=f32, device=dev).uniform_(-lim, lim, generator=g)
            self.b_tok = torch.empty((nt + 1,), dtype=f32, device=dev).uniform_(-lim, lim, generator=g)
            self.E_tok[nt].zero_()
            self.b_tok[nt] = 0.0
        self.A_tok = torch.full_like(self.E_tok, acc0)
        self.Ab_tok = torch.full_like(self.b_tok, acc0)
        # bag index by GLOBAL item id + one padding entity (index n_items): a bag of one padding token (row nt:
        # zeros, dropped by the gradient pass) -- what the padding rows of a pool block / of the receive buffer look up
        n_ent = int(lens.shape[0])
        if n_ent < n_items:
            raise ValueError("bag index shorter than the item table")
        v = np.concatenate([vals.astype(np.int32)[:int(starts[n_ent - 1] + lens[n_ent - 1])], [nt]]).astype(np.int32)
        st = np.concatenate([starts.astype(np.int32)[:n_ent], [len(v) - 1]]).astype(np.int32)
        ln = np.concatenate([lens.astype(np.int32)[:n_ent], [1]]).astype(np.int32)
        self.pad_item = n_ent
        self.bag_vals = torch.from_numpy(v).to(dev)
        self.bag_starts = torch.from_numpy(st).to(dev)
        self.bag_lens = torch.from_numpy(ln).to(dev)
        self.D_tok = torch.zeros((nt, d), dtype=f32, device=dev)      # merged token gradients, summed over the ranks
        self.Db_tok = torch.zeros((nt,), dtype=f32, device=dev)
        self.pool_ext = torch.zeros(S + 1, dtype=i32, device=dev)     # pool ids + the padding entity
        self.block_ids = torch.zeros(S, dtype=i32, device=dev)        # global item id of every row of the owned block
        # global item id (or the padding entity) -> row of the id shard (the shard's zero row where not owned): the
        # map the one-launch HET lookup of the static step takes beside the bag index (both indexed by global id)
        g = np.arange(n_ent + 1, dtype=np.int64)
        lm = np.where((g < n_items) & (g % world == rank), g // world, self.zero_row).astype(np.int32)
        self.lmap = torch.from_numpy(lm).to(dev)

    def set_pool(self, pool_ids):
        super().set_pool(pool_ids)
        be, S = self.be, self.S
        be.copy_i32(self.pool_ids, self.pool_ext[:S])
        be.copy_i32(torch.full((1,), self.pad_item, dtype=torch.int32, device=self.device), self.pool_ext[S:])
        if self.world == 1:
            be.copy_i32(self.pool_ids, self.block_ids)
        else:          # block row -> pool slot (S: padding) -> item id (padding entity)
            be.take_i32(self.pool_ext, self.my_slots, self.block_ids, self.pad_item)

    # ---- what ShardedHMF._step_body takes from this class: HET rows and the replicated token table ----
    def _static_feeds(self, route, cap_r):
        gid = route.get('gid')
        if gid is None or gid.shape[0] != cap_r:
            gid = torch.full((cap_r,), self.pad_item, dtype=torch.int32, device=self.device)
            R = route['R']
            if R > 0:
                gid[:R] = route['recv_ids'][:R]
            route['gid'] = gid
        if self.g_gid is None or self.g_gid.shape[0] != cap_r:
            self.g_gid = torch.empty(cap_r, dtype=torch.int32, device=self.device)
        return [(gid, self.g_gid)]

    def _gather(self, urows, rrows, T_in):
        """users, the owned pool block and the requested target rows in ONE launch (arx_lookup_multi): item rows =
        (id row + bag mean) / 2 with their biases, then the two bias columns of the packed rows."""
        be, d, W, cap, cap_r = self.be, self.d, self.world, self.cap, self.cap_r
        bag = (self.bag_vals, self.bag_starts, self.bag_lens)
        item = (self.E_item, self.b_item, self.lmap, self.E_tok, self.b_tok) + bag
        nt_rows = self.B_loc if W == 1 else cap_r
        if W == 1:
            pool_out, pool_b = self.I_all[:, :d], self.b_all
        else:
            pool_out, pool_b = self.I_pack[:cap, :d], self.b_g[:cap]
        be.lookup_het_multi([(self.E_user, None, None, None, None, None, None, None, urows, self.U_loc, 1.0, None),
                             item + (self.block_ids[:self.S if W == 1 else cap], pool_out, 0.5, pool_b),
                             item + (self.g_gid[:nt_rows], T_in[:nt_rows, :d], 0.5, self.tb_send[:nt_rows])])
        if W > 1:
            be.copy_strided(pool_b, self.I_pack[:cap, d])
        be.copy_strided(self.tb_send[:nt_rows], T_in[:nt_rows, d])

    def _k7(self, phase, urows, rrows):
        be, d, B_loc, Sg, ni, W = self.be, self.d, self.B_loc, self.Sg, self.ni_loc, self.world
        arena, arena_b, cap, cap_r = self.arena, self.arena_b, self.cap, self.cap_r
        nb = self.S if W == 1 else cap
        nt_rows = B_loc if W == 1 else cap_r
        be.sparse_adagrad_multi([(self.E_user, self.A_user, None, None),
                                 (self.E_item[:ni], self.A_item[:ni], self.b_item[:ni], self.Ab_item[:ni])],
                                [(0, urows, 0, 1.0), (1, self.pool_rows[:nb], B_loc, 0.5), (1, rrows, B_loc + Sg, 0.5)],
                                arena[:, :d], arena_b, self.lr, phase=phase)
        # (D_tok / Db_tok are all zero here: allocated so, and the token apply zeroes every row it consumes)
        be.bags_grad_dense(self.D_tok, self.Db_tok, self.bag_vals, self.bag_starts, self.bag_lens,
                           [(self.block_ids[:nb], B_loc, 0.5), (self.g_gid[:nt_rows], B_loc + Sg, 0.5)],
                           arena[:, :d], arena_b, phase=phase)

    def _tok_apply(self):
        """The same Adagrad step on every replica: rows of the summed gradient table that are not all zero (the rest
        would not move), the table zeroed on the way for the next step's accumulation (arx_adagrad_rows_nonzero)."""
        nt = self.n_tokens
        self.be.adagrad_rows_nonzero(self.E_tok[:nt], self.A_tok[:nt], self.b_tok[:nt], self.Ab_tok[:nt], self.D_tok,
                                     self.Db_tok, self.lr)

    def _after_apply(self, seg):
        """The merged token gradients of all ranks (one rank: nothing to sum), then the same dense Adagrad step
        everywhere."""
        if self.world > 1:
            dist.all_reduce(self.D_tok, op=dist.ReduceOp.SUM, group=self.group)
            dist.all_reduce(self.Db_tok, op=dist.ReduceOp.SUM, group=self.group)
        seg('tok_apply', self._tok_apply)

    def _fresh_step(self):
        """The dense token-gradient table must be all zero at step entry (the token apply zeroes the rows it
        consumes).  A step that died between the gradient pass and that apply would leave sums behind that the next
        step counts twice: every step that is NOT a replay (the first eager one, a re-capture, the step after an
        exception -- its graphs are dropped) starts from a cleared table."""
        self.D_tok.zero_()
        self.Db_tok.zero_()

    def item_view(self, chunk_cols=16384):
        """A serving view of this model (ShardedHetView): recommend / evaluate over its materialised item latents."""
        return ShardedHetView(self, chunk_cols=chunk_cols)

    def recommend(self, users, k, exclude_seen=False, return_values=False):
        """Not on the training class: the item latents are bag means -- item_view() materialises them per shard."""
        raise NotImplementedError("%s.recommend: item latents are bag means -- use item_view().recommend"
                                  % type(self).__name__)

    def recommend_sampled(self, *args, **kwargs):
        """Not on the training class either: item_view().recommend_sampled."""
        raise NotImplementedError("%s.recommend_sampled: item latents are bag means -- use "
                                  "item_view().recommend_sampled" % type(self).__name__)

    def list_logprob(self, *args, **kwargs):
        """Not on the training class either: item_view().list_logprob."""
        raise NotImplementedError("%s.list_logprob: item latents are bag means -- use "
                                  "item_view().list_logprob" % type(self).__name__)

    def similar_items(self, items, k, include_self=False, return_values=False):
        """ShardedHMF.similar_items over the materialised item latents 1/2 (id row + bag mean): through a serving view
        (item_view()) this model keeps for the purpose -- it refreshes when the model has stepped or been restored."""
        if getattr(self, '_sim_view', None) is None:
            self._sim_view = self.item_view()
        return self._sim_view.similar_items(items, k, include_self=include_self, return_values=return_values)

    def score_items(self, users, candidates, k=None):
        """Not on the training class: the item latents are bag means -- item_view() materialises them per shard."""
        raise NotImplementedError("%s.score_items: item latents are bag means -- use item_view().score_items"
                                  % type(self).__name__)

    def evaluate(self, users, items, loss='warp', return_rows=False):
        """Not on the training class: the item latents are bag means -- item_view() materialises them per shard."""
        raise NotImplementedError("%s.evaluate: item latents are bag means -- use item_view().evaluate"
                                  % type(self).__name__)

    def _checkpoint_arrays(self):
        return super()._checkpoint_arrays() + self._token_arrays('replicated')


class ShardedHetView(ShardedHMF):
    """Serving view of a sharded HET model (ShardedHMFBags / ShardedHMFRepTokens; model.item_view()): a SNAPSHOT of
    the item latents 1/2 (id row + bag mean) and biases, materialised per shard -- E_item [ni_loc + 1, d] (a zero row
    behind it) and b_item [ni_loc + 1] -- over which ShardedHMF's full-vocabulary recommend and evaluate run as they
    are (prepare_recommend_exclusions, prepare_eval_positives, recommend, evaluate: inherited; collectives, the same
    calling rules).  The snapshot costs the size of the id shard once more (ni_loc x (d + 1) x 4 B per rank); the
    user table is the model's own (by reference).  There are no step buffers: a view does not train.

    refresh() materialises the latents, a collective on the model's stream:
      ShardedHMFRepTokens   every token is local: ONE arx_het_rows_range launch over this rank's columns, straight
                            into E_item / b_item; no communication.
      ShardedHMFBags        an item's tokens live on every rank: per chunk of chunk_cols columns, one launch forms
                            this rank's PARTIAL of every owner's rows (half its own id row where it owns the item,
                            half the bag mean over its own tokens: exactly the partials of the step) in owner-major
                            blocks [W][chunk][d + 4], a reduce-scatter sums them into the owner's [chunk, d + 4], two
                            copies put them in place.  n_items x (d + 4) x 4 B cross the reduce-scatter per refresh
                            and rank.  (World 1: one launch, no collective.)
    The view remembers model.steps and model.n_restores; recommend / evaluate refresh first when the model has stepped
    or been restored from a checkpoint since (step() and model.saver.restore() are collectives, so every rank decides
    alike; a restore counts even where it lands on the step count the view has seen).  Tables written any other way
    (a test poking at the buffers) need an explicit refresh().  A view has no saver: it holds no state of its own.
    The view's buffers are its own: captured step graphs are not disturbed."""

    _TAKEN = ('world', 'rank', 'B_loc', 'B', 'd', 'n_users', 'n_items', 'ni_loc', 'zero_row', 'device', 'group', 'be',
              'use_graphs', '_stream')

    def __init__(self, model, chunk_cols=16384):
        if not isinstance(model, (ShardedHMFBags, ShardedHMFRepTokens)):
            raise TypeError("ShardedHetView: a ShardedHMFBags or ShardedHMFRepTokens model (ShardedHMF serves itself)")
        if int(chunk_cols) < 1:
            raise ValueError("chunk_cols must be positive")
        self.model = model
        for a in self._TAKEN:
            setattr(self, a, getattr(model, a))
        self.E_user = model.E_user
        dev, f32 = self.device, torch.float32
        self.E_item = torch.zeros((self.ni_loc + 1, self.d), dtype=f32, device=dev)
        self.b_item = torch.zeros((self.ni_loc + 1,), dtype=f32, device=dev)
        self.steps = None                                   # model.steps at the last refresh
        self._seen = None                                   # (model.steps, model.n_restores) at the last refresh
        self.n_refresh = 0
        # the token-striped model at N > 1: every rank walks the columns of the LARGEST shard in equal chunks
        self._striped = isinstance(model, ShardedHMFBags) and self.world > 1
        if self._striped:
            self._cols = (self.n_items + self.world - 1) // self.world
            self.chunk = max(1, min(int(chunk_cols), self._cols))
            self._part = torch.zeros((self.world * self.chunk, model.dp), dtype=f32, device=dev)
            self._sum = torch.zeros((self.chunk, model.dp), dtype=f32, device=dev)

    def refresh(self):
        """Materialise the item latents from the model's tables as they are now (a collective; see the class)."""
        with _ops.joined(self._stream if self.use_graphs else None):
            self._refresh()

    def _refresh(self):
        m, be, W, d = self.model, self.be, self.world, self.d
        src = (m.E_item, m.b_item, m.E_tok, m.b_tok, m.bag_vals, m.bag_starts, m.bag_lens, self.n_items, W, self.rank)
        if not self._striped:
            be.het_rows_range(*src, 0, self.ni_loc, self.E_item, bias_out=self.b_item, scale=0.5)
        else:
            for c0 in range(0, self._cols, self.chunk):
                c1 = min(c0 + self.chunk, self._cols)
                n = c1 - c0                                 # (c1 <= ni_loc + 1: a shorter shard's last column is its zero row)
                be.het_rows_range(*src, c0, c1, self._part, all_owners=True, scale=0.5, block_rows=self.chunk)
                _reduce_scatter(self._sum, self._part, group=self.group)
                be.copy_2d(self._sum[:n, :d], self.E_item[c0:c0 + n])
                be.copy_strided(self._sum[:n, d], self.b_item[c0:c0 + n])
        self.steps = m.steps
        self._seen = (m.steps, m.n_restores)
        self.n_refresh += 1

    def _recommend(self, u, k, exclude_seen, tags=None, sample=None):
        if self._seen != (self.model.steps, self.model.n_restores):
            self._refresh()
        return super()._recommend(u, k, exclude_seen, tags=tags, sample=sample)

    def _list_logprob(self, u, lists, k, tau, exclude_seen, tags):
        if self._seen != (self.model.steps, self.model.n_restores):
            self._refresh()
        return super()._list_logprob(u, lists, k, tau, exclude_seen, tags)

    def _evaluate(self, u, it, loss):
        if self._seen != (self.model.steps, self.model.n_restores):
            self._refresh()
        return super()._evaluate(u, it, loss)

    def _similar(self, it, k, include_self):
        if self._seen != (self.model.steps, self.model.n_restores):
            self._refresh()
        return super()._similar(it, k, include_self)

    def _score_items(self, u, cand, k):
        if self._seen != (self.model.steps, self.model.n_restores):
            self._refresh()
        return super()._score_items(u, cand, k)

    def _no_training(self, *a, **k):
        raise TypeError("ShardedHetView: a view does not train (step, pools and positives belong to the model)")

    step = set_pool = prepare_route = set_positives = _no_training


# ---------------------------------------------------------------------------------------------
# Data-parallel sequence model (the LSTM recommender has no table big enough to shard at
# C4's size -- 1 M x 64 x 4 B = 256 MB -- so the replicas split the BATCH).
# ---------------------------------------------------------------------------------------------
class _GIds(object):
    def __init__(self, value):
        self.value = value


class _GNode(object):
    """Stand-in for the lookup node of a gathered site: rows of the gathered gradient arena."""

    def __init__(self, row0, arena, arena_b, node):
        self.row0, self.arena, self.arena_b = row0, arena, arena_b
        self._grad_written = True
        self.bias_grad_used = node.bias_grad_used
        self.with_bias = node.with_bias
        self.shape = node.shape


class _GSite(object):
    """One lookup site of the GLOBAL batch: ids and gradient rows of every replica, rank-major."""

    def __init__(self, s, ids, node, n):
        self.table, self.kind, self.maps, self.max_len, self.coef = s.table, s.kind, s.maps, s.max_len, s.coef
        self.bias_coef = getattr(s, 'bias_coef', 1.0)
        self.col_off, self.key_off = 0, 0
        self.ids_node, self.node = _GIds(ids), node
        self.n = self.cap = n


class SeqDataParallel(object):
    """`world` replicas of a SeqModel (lstm/seqModel.py), one per GPU, each fed 1/world of the
    sequences of a step; one step of the group == the single-process step on the global batch
    (the reference has no multi-device path: SURVEY 8e).  sequence_loss sums over the examples
    (seqModel.py:596), so local gradients simply add.  Per step, between backward and apply:

      all_reduce   dense gradients (lstm_w / lstm_b of every layer, w_input_*), packed in one buffer
      all_reduce   the pool gradients: per-unrolled-step [L, S, d] (+ bias [L, S]) and their sums --
                   tf.gradients yields ONE dense matmul gradient per step for the global batch, and
                   clip_by_global_norm squares them step by step (seqModel.py:179-180)
      all_reduce   one scalar: the squared norms of the batch lookups' IndexedSlices (un-merged in
                   TF's norm, hence additive over replicas)
      all_gather   ids + gradient rows of every batch lookup (inputs, targets, users): every replica
                   then runs the SAME sparse-Adagrad pass over the global lookups -- duplicates
                   across replicas are merged before the one update per row, tables stay identical.

    The pool of sampled negatives must be the same on every replica (draw it with a shared seed or
    broadcast it: broadcast_pool).  One-hot item / user features (config C4); steps run eagerly (the
    collectives are not captured into the hipGraph)."""

    def __init__(self, model, group=None):
        self.model, self.rt, self.group = model, model.rt, group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        if getattr(model, 'output_feat', 1) not in (0, 1):
            raise NotImplementedError("SeqDataParallel: output_feat 0 / 1 only")
        self.rt.dp = self
        self.rt.use_graph = False
        self._plans = {}
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.rt.device)

    # ---- collectives --------------------------------------------------------------------------
    def all_reduce_sum(self, t):
        if self.world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    def _all_reduce_packed(self, tensors):
        """One all-reduce for a list of tensors (bucketed: a ring all-reduce over xGMI is bound by
        its per-link latency at these sizes, not by bytes)."""
        if self.world == 1 or not tensors:
            return
        if not all(t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 for t in tensors):
            # (advisor, round 5: a 4-byte INTEGER tensor packed into the float32 bucket would be summed as float bit
            # patterns -- the word-copy path is for float32 only)
            # (the gloo / CPU rig of the tests, strided views)
            flat = torch.cat([t.reshape(-1) for t in tensors])
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
            off = 0
            for t in tensors:
                n = t.numel()
                t.copy_(flat[off:off + n].view(t.shape))
                off += n
            return
        # round 5: the bucket is a persistent flat buffer, packed and unpacked by arx_copy_words (8 tensors per
        # launch) instead of torch.cat + one copy_ per tensor
        from . import ops
        n_all = sum(t.numel() for t in tensors)
        flat = getattr(self, '_bucket', None)
        if flat is None or flat.numel() < n_all or flat.device != tensors[0].device:
            flat = self._bucket = torch.empty(n_all, dtype=torch.float32, device=tensors[0].device)
        views, off = [], 0
        for t in tensors:
            views.append(flat[off:off + t.numel()])
            off += t.numel()
        ops.copy_words([(t.view(-1), v) for t, v in zip(tensors, views)])
        dist.all_reduce(flat[:n_all], op=dist.ReduceOp.SUM, group=self.group)
        ops.copy_words([(v, t.view(-1)) for t, v in zip(tensors, views)])

    def _all_gather(self, src, dst):
        """dst[w * n : (w + 1) * n] = src of replica w."""
        if self.world == 1:
            dst.copy_(src)
            return
        n = src.shape[0]
        dist.all_gather([dst[w * n:(w + 1) * n] for w in range(self.world)], src.contiguous(), group=self.group)

    def broadcast_pool(self, pool_ids):
        """Replica 0's sampled pool for everyone (int32 device tensor, in place)."""
        if self.world > 1:
            dist.broadcast(pool_ids, src=0, group=self.group)
        return pool_ids

    def global_loss(self, local_loss):
        self._loss.fill_(float(local_loss))
        return float(self.all_reduce_sum(self._loss).item())

    # ---- the exchange -------------------------------------------------------------------------
    def _state(self, plan):
        from . import graph as G
        st = self._plans.get(id(plan))
        if st is not None:
            return st
        rt = self.rt
        # pool lookups: their gradient is a dense [S, d] sum over the batch -> all-reduced, replicated
        pools, preds = set(), []
        for n in plan.order:
            if isinstance(n, G.Prediction) and n.inputs[1].train_tables:
                pools.add(id(n.inputs[1]))
                preds.append(n)
        tables = []
        for table, sites, bufs, total in plan.tables:
            if any(s.kind != 'cat' or s.col_off != 0 for s in sites):
                raise NotImplementedError("SeqDataParallel: one-hot, mean-combined features only")
            width = sites[0].node.shape[1]
            rows = sum(s.n * (1 if id(s.node) in pools else self.world) for s in sites)
            arena = torch.zeros((rows, width), dtype=torch.float32, device=rt.device)
            arena_b = torch.zeros((rows,), dtype=torch.float32, device=rt.device)
            gs, r0 = [], 0
            for s in sites:
                rep = id(s.node) in pools
                n = s.n if rep else s.n * self.world
                ids = s.ids_node.value if rep else torch.empty(n, dtype=torch.int32, device=rt.device)
                gs.append((s, _GSite(s, ids, _GNode(r0, arena, arena_b, s.node), n), rep))
                r0 += n
            gbufs = {'keys': torch.full((rows,), G.KEY_NONE, dtype=torch.int32, device=rt.device),
                     'src': torch.zeros((rows,), dtype=torch.int32, device=rt.device),
                     'coef': torch.zeros((rows,), dtype=torch.float32, device=rt.device),
                     'hot': torch.zeros((rows // 16 + 4,), dtype=torch.int32, device=rt.device)}
            off = 0
            for _, g, _ in gs:
                g.key_off = off
                off += g.cap
            tables.append(G.TableEntry(table, gs, gbufs, rows))
        st = dict(preds=preds, tables=tables)
        self._plans[id(plan)] = st
        return st

    def exchange(self, plan):
        """Called by the plan between backward and the optimiser (graph.py Plan._execute)."""
        rt = self.rt
        st = self._state(plan)
        # dense + pool gradients: one packed all-reduce
        pack = [p.grad for p in rt.dense.values() if getattr(p, 'touched', False)]
        for n in st['preds']:
            if not n._grad_written:
                continue
            pool = n.inputs[1]
            if getattr(n, 'C_steps', None) is not None:
                pack += [n.C_steps, n.rs_steps]
            pack.append(pool.grad)
            if pool.bias_grad_used:
                pack.append(pool.bias_grad)
        self._all_reduce_packed(pack)
        # batch lookups: ids and gradient rows of every replica; pool rows: copied (already global)
        for table, gs, gbufs, rows in st['tables']:
            for s, g, rep in gs:
                node = s.node
                g.node._grad_written = node._grad_written
                g.node.bias_grad_used = node.bias_grad_used
                if not node._grad_written:
                    continue
                a = g.node.arena[g.node.row0:g.node.row0 + g.n]
                ab = g.node.arena_b[g.node.row0:g.node.row0 + g.n]
                src = node.arena[node.row0:node.row0 + s.n]
                src_b = node.arena_b[node.row0:node.row0 + s.n]
                if rep:
                    a.copy_(src)
                    if node.bias_grad_used:
                        ab.copy_(src_b)
                else:
                    self._all_gather(s.ids_node.value, g.ids_node.value)
                    self._all_gather(src, a)
                    if node.bias_grad_used:
                        self._all_gather(src_b, ab)

    def gathered_tables(self, plan):
        """plan.tables with the gathered sites in place of the local ones (the planner's graph.TableEntry)."""
        return [e._replace(sites=[g for _, g, _ in e.sites]) for e in self._state(plan)['tables']]



# ---------------------------------------------------------------------------------------------
# Hybrid sequence model (round 6): embedding tables striped by row, LSTM weights data-parallel.
# north_star: "partition the item-embedding table row-wise ... all-reduce for the dense LSTM weights";
# the reference's only device split is a TF tower list (lstm/run.py:87,221-229, lstm/seqModel.py:87-126).
# ---------------------------------------------------------------------------------------------
class _ShardView(object):
    """A striped table WITHOUT its padding row, as K7 sees it: keys that name the padding row (lookups this rank
    does not own, padded receive slots) are out of range and dropped by the key builders."""

    def __init__(self, t, rows):
        self.name, self.bias_name = t.name, t.bias_name
        self.E, self.acc = t.E[:rows], t.acc[:rows]
        self.bias = None if t.bias is None else t.bias[:rows]
        self.bias_acc = None if t.bias_acc is None else t.bias_acc[:rows]
        self.sites = []
        self.aux_first = self.aux_cnt = None     # (Plan._aux_cnt)


class SeqHybridParallel(SeqDataParallel):
    """SeqModel on `world` ranks with every embedding table striped by ROW (owner = row % world, local row =
    row // world -- ShardedHMF's rule) and the dense parameters (lstm_w / lstm_b of every layer, w_input_*)
    replicated and all-reduced.  One step of the group == the single-process step on the global batch, like
    SeqDataParallel -- but no rank holds a whole table, no rank sorts the GLOBAL lookups, and the lookup traffic is
    all-to-all (rows travel once, to the rank that asked / owns) instead of an all-gather of every replica's rows:

      forward   per batch lookup (inputs, targets, users) and feature: ids -> owners (all_to_all, 4 B per lookup),
                the owner gathers its rows (K2 on its shard), rows + bias -> back (all_to_all, 4 (d + 1) B per
                lookup); the sampled pool: every rank gathers the pool rows it owns (zeros elsewhere), one
                all_reduce of [S, d + 1] makes the pool whole everywhere (S = 1024: 266 KB)
      backward  gradient rows of the batch lookups -> owners (all_to_all); the owner runs K7 over what it RECEIVED
                (keys = local rows) -- every row is updated once, on one rank, duplicates across ranks merged by
                that rank's pass; pool gradient [S, d] (+ bias): all_reduce, every owner applies ITS pool rows;
                per-unrolled-step pool gradients [L, S, d] (+ [L, S]): reduce_scatter -- they are only SQUARED
                (tf.clip_by_global_norm over the un-merged per-step matmul gradients, lstm/seqModel.py:178-182,
                SURVEY A.7): each rank squares its 1/world slice, the squares join the scalar all_reduce that the
                batch lookups' un-merged IndexedSlices norms already need
      dense     lstm_w / lstm_b / w_input_*: one packed all_reduce (128 KB at C4)

    Per rank and step at C4 (L = 50, B_loc = 1024, d = 64, S = 1024): 2 x 2 x 51 200 lookups x 260 B = 53 MB of
    all-to-all + 13.3 MB x (N - 1) / N of reduce_scatter + < 1 MB of small all-reduces -- against SeqDataParallel's
    all_gather of N x 26 MB of rows and a 13.3 MB all_reduce.  Routing (owner of every
    lookup, permutation, split sizes) is host work per batch on the ids the step is fed with: one D2H read of the
    ids per lookup node (data-loader work in a production loop, like ShardedHMF.prepare_route).

    The serving side scores the full vocabulary shard by shard -- no rank ever holds a whole table (B = world *
    B_loc, k = topk_n, n = L * B_loc; DESIGN.md section 7 has the bytes per call):

      model.step_recommend(...)  (step_recommend below; lstm/run.py:550-640, lstm/seqModel.py:326-353,514-517)
        (local)      lookups (fetch) -> LSTM layers -> RowsAt: latents [B_loc, d] at the positions asked for
        all_gather   latents -> [B, d], user indices -> [B]
        (local)      top-k + log-sum-exp over the shard's rows (backend.shard_topk, TopKScan with want_lse), the
                     excluding filter with exclude_seen; local columns -> logit ids (col2logit)
        all_to_all   values, logit ids [B, k], log-sum-exp [B] -> the ranks that own the rows
        (local)      W-way merge + softmax values (arx_topk_softmax_merge_shards)

      model.step(..., forward_only=True)  (step_eval below; the dev loss of lstm/run.py:505-519)
        (local)      lookups (fetch) -> LSTM layers: hs [n, d]
        all_gather   hs, mapped targets, row keys -- in row blocks of at most 16384 global rows
        (local)      target score: the owner's row, every other rank's padding row; all_reduce(SUM)
        (local)      the shard's 'ce' / 'warp' partial per row (backend.shard_eval, the eval positives masked)
        all_to_all   partials -> the ranks that own the rows; arx_eval_merge_shards
        (local)      sum_t loss_t w_t / (sum_t w_t + 1e-12), summed over this rank's sequences

    Per rank, built once on first use (_serving): col2logit [rows] (local table row -> logit index, -1 for the START
    row, items outside the logit vocabulary and the padding of the last stripe), a bias vector that is -inf at those
    rows, and the exclusion lists / eval positives as CSR over this rank's local columns (every rank holds the full
    host-side sets, as the single-process model does: no collective).

    Scope: models whose trained lookups are one-hot, mean-combined features (the restriction SeqDataParallel has;
    C4), output_feat 0 / 1; serving also needs the output side to be ONE one-hot feature whose logit -> row map is
    injective (the id feature).  Steps run eagerly (collectives between the kernels).  No multi-GPU box was in reach
    of the builder: verified with gloo ranks sharing one GPU (tests/test_seq_hybrid_gpu.py,
    tests/test_seq_hybrid_serve_gpu.py) and on CPU for the routing and the serving maps (tests/test_dist_cpu.py,
    tests/test_seq_hybrid_serve_cpu.py)."""

    def __init__(self, model, group=None):
        super().__init__(model, group)
        self._feat = {}            # id(Feature) -> dict(full_h, route)
        self._fetch = {}           # (id(node), k) -> this step's exchange record
        self._hstate = {}
        self._serve_fetch = {}     # (id(node), k) -> receive buffers of the forward-only plans (no gradient arena)
        self._serve = None         # serving state of this rank (_serving)
        self._shard_tables()
        # the wrapped model's Saver would write this rank's stripe, padding row included, under the global name: a
        # runner's model.saver.save / restore go through the sharded saver (collectives) from here on
        from .utils.checkpoint import ShardedSaver
        self.device = self.rt.device
        self.saver = model.saver = ShardedSaver(self)

    # ---- striping -----------------------------------------------------------------------------
    def _shard_tables(self):
        W, r = self.world, self.rank
        for t in self.model.att_emb.tables.values():
            if getattr(t, 'shard', None) is not None:
                continue
            V, d = int(t.E.shape[0]), int(t.E.shape[1])
            rows = (V + W - 1) // W
            E = torch.zeros((rows + 1, d), dtype=torch.float32, device=t.E.device)
            mine = t.E[r::W]
            E[:mine.shape[0]].copy_(mine)
            acc = torch.full_like(E, float(t.acc.flatten()[0].item()) if t.acc.numel() else 0.1)
            acc[:mine.shape[0]].copy_(t.acc[r::W])
            bias = bias_acc = None
            if t.bias is not None:
                bias = torch.zeros((rows + 1,), dtype=torch.float32, device=t.E.device)
                bias[:mine.shape[0]].copy_(t.bias[r::W])
                bias_acc = torch.full_like(bias, 0.1)
                bias_acc[:mine.shape[0]].copy_(t.bias_acc[r::W])
            t.E, t.acc, t.bias, t.bias_acc = E, acc, bias, bias_acc
            t.shard = dict(V=V, rows=rows, zero_row=rows, count=int(mine.shape[0]))
            t.view = _ShardView(t, rows)
            t.aux_first = t.aux_cnt = None

    @staticmethod
    def route_rows(full_rows, world):
        """Host side of one lookup exchange: (order, send_rows, send_counts) for global table rows `full_rows` --
        lookups grouped by owner (stable: the order inside a group is the order of the lookups), rows as LOCAL rows
        of their owner."""
        full_rows = np.asarray(full_rows, dtype=np.int64)
        order, _, counts = owner_order(full_rows, world)
        return order.astype(np.int32), (full_rows[order] // world).astype(np.int32), counts

    def _feature(self, f):
        """The map of a feature re-expressed for a striped table: kept on the host (entity -> global row) for the
        routing, and on the device as entity -> LOCAL row or the padding row (pool-like lookups: every rank looks the
        same ids up and contributes the rows it owns)."""
        st = self._feat.get(id(f))
        if st is None:
            t = f.table
            V = t.shard['V']
            full = f.maps[0]
            full_h = np.arange(V, dtype=np.int64) if full is None else full.cpu().numpy().astype(np.int64)
            if full_h.size and (full_h.min() < 0 or full_h.max() >= V):
                raise ValueError("SeqHybridParallel: feature map of %s leaves the table" % t.name)
            route = np.where(full_h % self.world == self.rank, full_h // self.world, t.shard['zero_row'])
            st = dict(full_h=full_h, route=torch.from_numpy(route.astype(np.int32)).to(t.E.device), f=f)
            self._feat[id(f)] = st
        return st

    def _exchange_counts(self, send_counts):
        W = self.world
        sc = torch.as_tensor(send_counts, dtype=torch.int64)
        rc = torch.empty(W, dtype=torch.int64)
        if W > 1:
            be = dist.get_backend(self.group)
            if be == 'nccl':
                scd, rcd = sc.to(self.rt.device), rc.to(self.rt.device)
                dist.all_to_all_single(rcd, scd, group=self.group)
                rc = rcd.cpu()
            else:
                dist.all_to_all_single(rc, sc, group=self.group)
        else:
            rc.copy_(sc)
        return [int(x) for x in sc.tolist()], [int(x) for x in rc.tolist()]

    def _a2a(self, out, inp, out_splits, in_splits):
        if self.world == 1:
            out.copy_(inp)
            return
        if out.is_cuda and dist.get_backend(self.group) != 'nccl':      # (the gloo rig of the tests: host-staged)
            o, i = torch.empty(out.shape, dtype=out.dtype), inp.cpu()
            dist.all_to_all_single(o, i, out_splits, in_splits, group=self.group)
            out.copy_(o)
            return
        dist.all_to_all_single(out, inp.contiguous(), out_splits, in_splits, group=self.group)

    def _reduce_host_staged(self, t):
        if self.world > 1:
            if t.is_cuda and dist.get_backend(self.group) != 'nccl':
                h = t.cpu()
                dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group)
                t.copy_(h)
            else:
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    # ---- forward: the lookups ---------------------------------------------------------------------
    def _pool_nodes(self, plan):
        from . import graph as G
        pools = set()
        for n in plan.order:
            if isinstance(n, G.Prediction):
                pools.add(id(n.inputs[1]))
        return pools

    def fetch(self, plan):
        """Plan._execute, in front of the lookups: every EntityEmbed node of the plan is served here."""
        from . import graph as G, ops
        if not plan.train:
            return self._fetch_forward(plan)
        pools = self._pool_nodes(plan)
        dev = self.rt.device
        done = set()
        for n in plan.order:
            if not isinstance(n, G.EntityEmbed):
                continue
            if n.concat or any(f.kind != 'cat' for f in n.feats):
                raise NotImplementedError("SeqHybridParallel: one-hot, mean-combined features only")
            n.alloc_value()
            F = len(n.feats)
            if id(n) in pools:
                # every rank: the pool rows it owns (the padding row elsewhere), summed over the ranks
                for k, f in enumerate(n.feats):
                    fs = self._feature(f)
                    t = f.table
                    ops.gather_onehot(t.E, t.bias if n.with_bias else None, fs['route'], n.inputs[0].value, n.value,
                                      scale=n.out_scale / F, accumulate=k > 0,
                                      bias_out=n.bias_value if n.with_bias else None)
                self._reduce_host_staged(n.value)
                if n.with_bias:
                    self._reduce_host_staged(n.bias_value)
                done.add(id(n))
                continue
            ids_h = n.inputs[0].value.cpu().numpy()
            for k, f in enumerate(n.feats):
                fs = self._feature(f)
                t = f.table
                d = int(t.E.shape[1])
                order, send_rows, sc = self.route_rows(fs['full_h'][ids_h], self.world)
                sc, rc = self._exchange_counts(sc)
                R = sum(rc)
                nloc = int(ids_h.shape[0])
                rec = self._fetch.get((id(n), k))
                if rec is None or rec['cap'] < R:
                    cap = max(R, nloc + nloc // 2 + 64) if self.world > 1 else nloc
                    rec = dict(cap=cap, recv_rows=torch.empty(cap, dtype=torch.int32, device=dev),
                               rows=torch.empty((cap, d), dtype=torch.float32, device=dev),
                               rows_b=torch.empty((cap,), dtype=torch.float32, device=dev),
                               got=torch.empty((nloc, d), dtype=torch.float32, device=dev),
                               got_b=torch.empty((nloc,), dtype=torch.float32, device=dev),
                               send=torch.empty((nloc, d), dtype=torch.float32, device=dev),
                               send_b=torch.empty((nloc,), dtype=torch.float32, device=dev),
                               garena=torch.zeros((cap, d), dtype=torch.float32, device=dev),
                               garena_b=torch.zeros((cap,), dtype=torch.float32, device=dev), gen=0)
                    rec['gen'] = (self._fetch[(id(n), k)]['gen'] + 1) if (id(n), k) in self._fetch else 0
                    self._fetch[(id(n), k)] = rec
                    self._hstate.pop(id(plan), None)          # (new buffers: the K7 proxies are rebuilt)
                inv = np.empty_like(order)
                inv[order] = np.arange(order.shape[0], dtype=np.int32)
                rec.update(sc=sc, rc=rc, R=R, order=torch.from_numpy(order).to(dev), inv=torch.from_numpy(inv).to(dev))
                rec['recv_rows'].fill_(t.shard['zero_row'])
                self._a2a(rec['recv_rows'][:R], torch.from_numpy(send_rows).to(dev), rc, sc)      # ids -> owners
                wb = n.with_bias and t.bias is not None
                if R:
                    ops.gather_onehot(t.E, t.bias if wb else None, None, rec['recv_rows'][:R], rec['rows'][:R],
                                      bias_out=rec['rows_b'][:R] if wb else None)
                self._a2a(rec['got'], rec['rows'][:R], sc, rc)                                    # rows -> back
                if wb:
                    self._a2a(rec['got_b'], rec['rows_b'][:R], sc, rc)
                # got is in owner order: lookup i sits at got[inv[i]]
                ops.gather_onehot(rec['got'], rec['got_b'] if wb else None, None, rec['inv'], n.value,
                                  scale=n.out_scale / F, accumulate=k > 0,
                                  bias_out=n.bias_value if n.with_bias else None)
            done.add(id(n))
        return done

    def _fetch_forward(self, plan):
        """fetch() of a forward-only plan (the serving side: step_recommend, step(forward_only=True)): the same id ->
        owner -> rows -> back exchange for every batch lookup, with receive buffers of its own (_serve_fetch) -- no
        gradient arena is allocated, _fetch and _hstate stay as the last training step left them.  A forward-only plan
        that scores a pool (a Prediction node) is refused: the full vocabulary is scored shard by shard, never looked
        up as one pool."""
        from . import graph as G, ops
        dev = self.rt.device
        if any(isinstance(n, G.Prediction) for n in plan.order):
            raise NotImplementedError("SeqHybridParallel: a forward-only plan over striped tables cannot score a pool; "
                                      "use model.step_recommend / model.step(..., forward_only=True)")
        done = set()
        for n in plan.order:
            if not isinstance(n, G.EntityEmbed):
                continue
            if n.concat or any(f.kind != 'cat' for f in n.feats):
                raise NotImplementedError("SeqHybridParallel: one-hot, mean-combined features only")
            n.alloc_value()
            F = len(n.feats)
            ids_h = n.inputs[0].value.cpu().numpy()
            nloc = int(ids_h.shape[0])
            for k, f in enumerate(n.feats):
                fs = self._feature(f)
                t = f.table
                d = int(t.E.shape[1])
                order, send_rows, sc = self.route_rows(fs['full_h'][ids_h], self.world)
                sc, rc = self._exchange_counts(sc)
                R = sum(rc)
                rec = self._serve_fetch.get((id(n), k))
                if rec is None or rec['cap'] < R:
                    cap = max(R, nloc + nloc // 2 + 64) if self.world > 1 else nloc
                    rec = self._serve_fetch[(id(n), k)] = dict(
                        cap=cap, recv_rows=torch.empty(cap, dtype=torch.int32, device=dev),
                        rows=torch.empty((cap, d), dtype=torch.float32, device=dev),
                        rows_b=torch.empty((cap,), dtype=torch.float32, device=dev),
                        got=torch.empty((nloc, d), dtype=torch.float32, device=dev),
                        got_b=torch.empty((nloc,), dtype=torch.float32, device=dev))
                inv = np.empty_like(order)
                inv[order] = np.arange(order.shape[0], dtype=np.int32)
                self._a2a(rec['recv_rows'][:R], torch.from_numpy(send_rows).to(dev), rc, sc)      # ids -> owners
                wb = n.with_bias and t.bias is not None
                if R:
                    ops.gather_onehot(t.E, t.bias if wb else None, None, rec['recv_rows'][:R], rec['rows'][:R],
                                      bias_out=rec['rows_b'][:R] if wb else None)
                self._a2a(rec['got'], rec['rows'][:R], sc, rc)                                    # rows -> back
                if wb:
                    self._a2a(rec['got_b'], rec['rows_b'][:R], sc, rc)
                ops.gather_onehot(rec['got'], rec['got_b'] if wb else None, None, torch.from_numpy(inv).to(dev),
                                  n.value, scale=n.out_scale / F, accumulate=k > 0,
                                  bias_out=n.bias_value if n.with_bias else None)
            done.add(id(n))
        return done

    # ---- serving: the host side (no GPU needed) ------------------------------------------------------
    @staticmethod
    def serve_col2logit(cmap, rows, world, rank):
        """col2logit [rows] int32 of one rank: local table row -> logit index, -1 for the rows outside the logit
        vocabulary (the START row, items filtered out of the vocabulary, the ragged end of the last stripe).  cmap: the
        output feature's logit -> GLOBAL table row map (_pool_embed('full', ...)'s cmap); it must be injective -- one
        one-hot id feature -- or a table row would stand for several logits (NotImplementedError)."""
        cmap = np.asarray(cmap, dtype=np.int64).reshape(-1)
        if cmap.size and (cmap.min() < 0 or cmap.max() >= int(rows) * int(world)):
            raise ValueError("serve_col2logit: the logit -> row map leaves the table")
        if np.unique(cmap).size != cmap.size:
            raise NotImplementedError("SeqHybridParallel serving: the output side must be a single one-hot feature "
                                      "whose logit -> row map is injective (the id feature); this map sends several "
                                      "logits to one table row")
        out = np.full(int(rows), -1, dtype=np.int32)
        mine = np.nonzero(cmap % world == rank)[0]
        out[cmap[mine] // world] = mine.astype(np.int32)
        return out

    @staticmethod
    def serve_shard_csr(ptr, cols, cmap, world, rank):
        """Per-key lists of LOGIT columns (ptr [n_keys + 1], cols: exclusion_csr's form) -> (ptr int32 [n_keys + 1],
        cols int32 [>= 1]) over the LOCAL columns of one rank: the logits whose table row cmap[logit] this rank owns
        (row % world == rank), as row // world, every list sorted ascending without duplicates -- the (ex_ptr, ex_cols)
        that shard_topk and shard_eval take."""
        ptr = np.asarray(ptr, dtype=np.int64).reshape(-1)
        cmap = np.asarray(cmap, dtype=np.int64).reshape(-1)
        n_keys = len(ptr) - 1
        c = np.asarray(cols, dtype=np.int64).reshape(-1)[:ptr[-1]]
        keys = np.repeat(np.arange(n_keys, dtype=np.int64), np.diff(ptr))
        ok = (c >= 0) & (c < len(cmap))
        keys, g = keys[ok], cmap[c[ok]]
        own = g % world == rank
        keys, loc = keys[own], g[own] // world
        o = np.lexsort((loc, keys))
        keys, loc = keys[o], loc[o]
        if len(keys):
            keep = np.ones(len(keys), dtype=bool)
            keep[1:] = (keys[1:] != keys[:-1]) | (loc[1:] != loc[:-1])
            keys, loc = keys[keep], loc[keep]
        out_ptr = np.zeros(n_keys + 1, dtype=np.int64)
        np.cumsum(np.bincount(keys, minlength=n_keys), out=out_ptr[1:])
        if len(loc) == 0:
            loc = np.zeros(1, dtype=np.int64)           # (a valid device pointer; every list is empty)
        return out_ptr.astype(np.int32), loc.astype(np.int32)

    # ---- serving: per-rank state ----------------------------------------------------------------------
    def _serving(self):
        """Built once: the output feature, col2logit, the -inf mask of the out-of-vocabulary rows, the backend."""
        sv = self._serve
        if sv is not None:
            return sv
        model, m, dev = self.model, self.model.att_emb, self.rt.device
        pe = m._pool_embed('full', model.output_feat)
        if len(pe.feats) != 1 or pe.feats[0].kind != 'cat':
            raise NotImplementedError("SeqHybridParallel serving: the output side must be a single one-hot feature "
                                      "(the id feature); got %s" % [f.kind for f in pe.feats])
        f = pe.feats[0]
        fs, t = self._feature(f), f.table
        rows = t.shard['rows']
        c2l = self.serve_col2logit(fs['full_h'], rows, self.world, self.rank)
        neg = np.where(c2l < 0, -np.inf, 0.0).astype(np.float32)
        sv = self._serve = dict(f=f, fs=fs, t=t, rows=rows, col2logit=torch.from_numpy(c2l).to(dev),
                                neg=torch.from_numpy(neg).to(dev),
                                bias=torch.empty(rows, dtype=torch.float32, device=dev),
                                be=HipBackend(dev), ex=None, pos=None, rec={}, ev={})
        return sv

    def _serve_bias(self, sv):
        """The shard's bias over its local rows, -inf where a row is outside the logit vocabulary: such a row never
        wins and adds nothing to a log-sum-exp or a margin sum."""
        from . import ops
        b, t = sv['bias'], sv['t']
        b.copy_(sv['neg'])
        if t.bias is not None:
            ops.axpby(1.0, t.bias[:sv['rows']], 1.0, b)
        return b

    def _serve_lists(self, sv, slot, src, ptr, cols):
        """Device CSR over this rank's local columns of host lists of logit columns; rebuilt when the lists change."""
        if sv[slot] is None or sv[slot][0] is not src:
            p, c = self.serve_shard_csr(ptr, cols, sv['fs']['full_h'], self.world, self.rank)
            dev = self.rt.device
            sv[slot] = (src, torch.from_numpy(p).to(dev), torch.from_numpy(c).to(dev))
        return sv[slot][1], sv[slot][2]

    def _serve_exclusions(self, sv):
        src = getattr(self.model.att_emb, '_ex_host', None)
        if src is None:
            raise ValueError("exclude_seen=True needs prepare_recommend_exclusions() first")
        return self._serve_lists(sv, 'ex', src, src[0], src[1])

    def _serve_positives(self, sv):
        from .attributes.embed_attribute import exclusion_csr
        m = self.model.att_emb
        if not hasattr(m, 'pos_item_set_eval'):
            raise ValueError("the 'warp' dev loss needs prepare_warp() first")
        src = m.pos_item_set_eval
        if sv['pos'] is not None and sv['pos'][0] is src:
            return sv['pos'][1], sv['pos'][2]
        ptr, cols = exclusion_csr(src if src is not None else {}, m.n_users + 1, m._item2logit_np)
        if src is None:
            src = sv                                    # (any stable object: no positives were given)
        return self._serve_lists(sv, 'pos', src, ptr, cols)

    def _gather(self, src, dst):
        """dst[w * n : (w + 1) * n] = src of rank w (host-staged under gloo, like _a2a)."""
        if self.world == 1:
            dst.copy_(src)
            return
        if src.is_cuda and dist.get_backend(self.group) != 'nccl':
            o = torch.empty(dst.shape, dtype=dst.dtype)
            dist.all_gather_into_tensor(o, src.cpu().contiguous(), group=self.group)
            dst.copy_(o)
            return
        dist.all_gather_into_tensor(dst, src.contiguous(), group=self.group)

    # ---- serving: recommend ----------------------------------------------------------------------------
    def step_recommend(self, session, user_input, item_inputs, positions, bucket_id, exclude_seen=False):
        """SeqModel.step_recommend of the striped model (the model dispatches here): same arguments, same return --
        [(uid, values[topk_n], indexes[topk_n])] for this rank's sequences.  A collective: every rank calls it with
        its own batch_size sequences, the same bucket and the same exclude_seen.  B = world * B_loc, k = topk_n:

          (local)      lookups (fetch: ids -> owners, rows back) -> LSTM layers -> RowsAt: latents [B_loc, d]
          all_gather   latents -> [B, d], user indices -> [B]
          (local)      top-k + log-sum-exp of U_all . E[:rows]^T + bias over the shard's rows (backend.shard_topk:
                       TopKScan with want_lse; bias = -inf at rows outside the logit vocabulary); exclude_seen: the
                       excluding filter over this rank's local columns, the log-sum-exp stays over all columns;
                       chunked once more after an overflow, on this rank only; local columns -> logit ids (col2logit)
          all_to_all   values, logit ids [B, k] and log-sum-exp [B] -> the ranks that own the rows: [W][B_loc][k]
          (local)      W-way merge, softmax values exp(v - lse) (arx_topk_softmax_merge_shards)

        Ties among exactly equal scores come out as (score desc, logit id asc) whenever logit ids increase with the
        table rows on each shard (identity maps, C4, the synthetic sets without a logit permutation); otherwise tied
        entries of ONE shard keep that shard's row order.  exclude_seen without prepare_recommend_exclusions raises
        ValueError before any collective; where fewer than topk_n items remain the tail is index -1, value 0."""
        from . import graph as G, ops
        from .lstm.seqModel import RowsAt
        model, rt, W = self.model, self.rt, self.world
        m, dev = model.att_emb, self.rt.device
        sv = self._serving()
        exl = self._serve_exclusions(sv) if exclude_seen else None
        L, Bl = model.buckets[bucket_id], model.batch_size
        B = Bl * W
        k = min(int(model.topk_n), int(m.logit_size))
        if not 1 <= k <= 1024:
            raise ValueError("step_recommend over striped tables: need 1 <= topk_n <= 1024")
        if len(positions) > Bl:
            raise ValueError("step_recommend: at most batch_size positions")
        it = item_inputs
        if not isinstance(it, torch.Tensor):
            it = torch.from_numpy(np.ascontiguousarray(np.asarray(it, dtype=np.int32)[:L].reshape(-1)))
        m.input_all.value[:L * Bl].copy_(it.reshape(-1), non_blocking=True)
        m.add_input({}, user_input, None, forward_only=True, recommend=True, loss=model.loss)
        users = user_input.cpu().numpy() if isinstance(user_input, torch.Tensor) else user_input
        bk = model._bucket(bucket_id)
        if 'serve_rec' not in bk['plans']:
            bk['serve_rows'] = G.IdsInput(rt, Bl, 'serve_rows_%d' % L)
            bk['serve_sel'] = RowsAt(rt, bk['hs'], bk['serve_rows'])
            bk['plans']['serve_rec'] = G.Plan(rt, [bk['serve_sel']], False, [])
        rows_h = np.zeros(Bl, dtype=np.int32)
        rows_h[:len(positions)] = [int(pos) * Bl + i for i, pos in enumerate(positions)]
        bk['serve_rows'].feed(rows_h)
        bk['plans']['serve_rec'].run()
        lat = bk['serve_sel'].value
        d = int(lat.shape[1])
        buf = sv['rec'].get((Bl, k, d))
        if buf is None:
            e = lambda dt, *sh: torch.empty(sh, dtype=dt, device=dev)
            f32, i32 = torch.float32, torch.int32
            buf = sv['rec'][(Bl, k, d)] = (e(f32, B, d), e(i32, B), e(f32, B, k), e(i32, B, k), e(i32, B, k), e(f32, B),
                                           e(f32, W, Bl, k), e(i32, W, Bl, k), e(f32, W, Bl), e(f32, Bl, k),
                                           e(i32, Bl, k), e(f32, Bl))
        U_all, keys_all, out_v, out_c, out_g, lse, recv_v, recv_g, recv_l, po, io, lse_o = buf
        keys_loc = torch.from_numpy(np.asarray(users, dtype=np.int32).reshape(-1)).to(dev)
        self._gather(lat, U_all)
        self._gather(keys_loc, keys_all)
        rows = sv['rows']
        ex = (keys_all, B, exl[0], exl[1]) if exclude_seen else None
        sv['be'].shard_topk(U_all, sv['t'].E[:rows], self._serve_bias(sv), k, ex, out_v, out_c, lse=lse)
        ops.take_i32(sv['col2logit'], out_c.view(-1), out_g.view(-1), fill=-1)
        self._a2a(recv_v.view(B, k), out_v, None, None)
        self._a2a(recv_g.view(B, k), out_g, None, None)
        self._a2a(recv_l.view(B), lse, None, None)
        ops.topk_softmax_merge_shards(recv_v, recv_g, recv_l, po, io, lse_o)
        vals, idx = po.cpu().numpy(), io.cpu().numpy()
        return [(users[i], vals[i], idx[i]) for i in range(len(positions))]

    # ---- serving: the dev loss ---------------------------------------------------------------------------
    EVAL_BLOCK_ROWS = 16384

    def step_eval(self, session, user_input, item_inputs, targets, target_weights, bucket_id):
        """SeqModel.step(..., forward_only=True) of the striped model (the model dispatches here): this rank's summed
        sequence loss over the FULL vocabulary -- 'warp' (each user's eval positives masked) for a model trained with
        'mw', 'ce' for 'mce' (seqModel.py:510) -- so that global_loss(local) is the single-process forward-only loss
        of the global batch.  A collective.  n = L * B_loc rows per rank, in row blocks of at most 16384 global rows:

          (local)      lookups (fetch) -> LSTM layers: hs [n, d]; forward-only plans never drop
          all_gather   hs, the mapped targets (logit indices) and the row keys (the user index of each row)
          (local)      the target score: the owner's row, every other rank's padding row, dot; all_reduce(SUM)
          (local)      this shard's partial per row over E[:rows] (backend.shard_eval 'ce' / 'warp', bias = -inf at
                       rows outside the logit vocabulary, the eval positives as lists of local columns)
          all_to_all   partials -> the ranks that own the rows: [W][rows of the block]
          (local)      the loss per row (arx_eval_merge_shards); after the last block sum_t loss_t w_t /
                       (sum_t w_t + 1e-12) summed over the sequences (seqModel.py:551-567,596: arx_seq_weights,
                       arx_dot_scaled)

        Rows of weight 0 (positions past a sequence's end) are scored like any other and weigh nothing."""
        from . import graph as G, ops
        from .attributes.embed_attribute import EVAL_LOSS_OF
        from .lstm.seqModel import SeqWeights
        model, rt, W, r = self.model, self.rt, self.world, self.rank
        m, dev = model.att_emb, self.rt.device
        kind = EVAL_LOSS_OF.get(model.loss)
        if kind is None:
            raise NotImplementedError("SeqHybridParallel: the dev loss of models trained with 'mw' / 'mce' only "
                                      "(full-vocabulary training losses are not striped)")
        sv = self._serving()
        pos = self._serve_positives(sv) if kind == 'warp' else None
        L, Bl = model.buckets[bucket_id], model.batch_size
        n = L * Bl
        tg_h = targets.cpu().numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets, dtype=np.int64)[:L]
        lg_h = m._item2logit_np[tg_h.reshape(-1).astype(np.int64)]
        if (lg_h < 0).any():
            raise KeyError(int(tg_h.reshape(-1)[np.argmax(lg_h < 0)]))         # (target_mapping's error)
        model._feed(user_input, item_inputs, targets, target_weights, L, None, None, True)
        users = user_input.cpu().numpy() if isinstance(user_input, torch.Tensor) else user_input
        bk = model._bucket(bucket_id)
        if 'serve_eval' not in bk['plans']:
            bk['serve_wn'] = SeqWeights(rt, bk['eval'].inputs[1].inputs[0], L, Bl)
            bk['plans']['serve_eval'] = G.Plan(rt, [bk['hs'], bk['serve_wn']], False, [])
        bk['plans']['serve_eval'].run()
        hs, wn = bk['hs'].value, bk['serve_wn'].value
        tg = model.targets_all.value[:n]
        d = int(hs.shape[1])
        nb = max(1, min(n, self.EVAL_BLOCK_ROWS // W))
        buf = sv['ev'].get((n, nb, d))
        if buf is None:
            e = lambda dt, *sh: torch.empty(sh, dtype=dt, device=dev)
            f32, i32 = torch.float32, torch.int32
            N = W * nb
            # gathered hs / targets / keys; target rows, bias (zeros without a bias table), score, local column; the
            # shard's partials (+ unused counts), the received [W][c]; this rank's row losses; the weighted sum
            buf = sv['ev'][(n, nb, d)] = (e(f32, N, d), e(i32, N), e(i32, N), e(f32, N, d),
                                          torch.zeros(N, dtype=f32, device=dev), e(f32, N), e(i32, N), e(f32, N),
                                          e(i32, N), e(f32, N), e(f32, n), e(f32, 1))
        H_all, T_all, K_all, Tg, tb, t, tcol, part, cnt, recv, loss_rows, out = buf
        keys = torch.from_numpy(np.tile(np.asarray(users, dtype=np.int32).reshape(-1), L)).to(dev)
        tab, rows, route = sv['t'], sv['rows'], sv['fs']['route']
        E, bias = tab.E[:rows], self._serve_bias(sv)
        for a in range(0, n, nb):
            b = min(n, a + nb)
            c = b - a
            N = W * c
            self._gather(hs[a:b], H_all[:N])
            self._gather(tg[a:b], T_all[:N])
            self._gather(keys[a:b], K_all[:N])
            # the target logit: the owner's row, every other rank's padding row -- one non-zero summand per row
            ops.gather_onehot(tab.E, tab.bias, route, T_all[:N], Tg[:N],
                              bias_out=tb[:N] if tab.bias is not None else None)
            ops.take_i32(route, T_all[:N], tcol[:N], fill=rows)          # (the padding row: "not on this shard")
            ops.dot_score(H_all[:N], Tg[:N], tb[:N], t[:N])
            self._reduce_host_staged(t[:N])
            ex = (K_all[:N], N, pos[0], pos[1]) if kind == 'warp' else None
            sv['be'].shard_eval(H_all[:N], E, bias, t[:N], tcol[:N], kind, ex, part[:N], cnt[:N])
            self._a2a(recv[:N], part[:N], None, None)
            sv['be'].eval_merge_shards(kind, recv[:N].view(W, c), None, t[r * c:(r + 1) * c], loss_rows[a:b], None)
        ops.dot_scaled(loss_rows, wn, 1.0, out)
        return float(out.item())

    # ---- backward: gradients to the owners ----------------------------------------------------------
    def _state(self, plan):
        from . import graph as G
        st = self._hstate.get(id(plan))
        if st is not None:
            return st
        rt = self.rt
        dev = rt.device
        pools, preds = set(), []
        for n in plan.order:
            if isinstance(n, G.Prediction) and n.inputs[1].train_tables:
                pools.add(id(n.inputs[1]))
                preds.append(n)
        tables = []
        for table, sites, bufs, total in plan.tables:
            if any(s.kind != 'cat' or s.col_off != 0 for s in sites):
                raise NotImplementedError("SeqHybridParallel: one-hot, mean-combined features only")
            width = sites[0].node.shape[1]
            gs, rows = [], 0
            for s in sites:
                k = next(i for i, f in enumerate(s.node.feats) if f.table is s.table)
                if id(s.node) in pools:
                    n_ = s.n
                    route = self._feature(s.node.feats[k])['route']
                    gs.append((s, n_, 'pool', route, None))
                else:
                    rec = self._fetch[(id(s.node), k)]
                    gs.append((s, rec['cap'], 'batch', None, rec))
                rows += gs[-1][1]
            arena = torch.zeros((rows, width), dtype=torch.float32, device=dev)
            arena_b = torch.zeros((rows,), dtype=torch.float32, device=dev)
            out, r0 = [], 0
            for s, n_, kind, route, rec in gs:
                if kind == 'pool':
                    g = _GSite(s, s.ids_node.value, _GNode(r0, arena, arena_b, s.node), n_)
                    g.maps = (route,)
                else:
                    g = _GSite(s, rec['recv_rows'], _GNode(r0, arena, arena_b, s.node), n_)
                    g.maps = (None,)
                g.table = table.view
                out.append((s, g, kind, rec))
                r0 += n_
            gbufs = {'keys': torch.full((rows,), G.KEY_NONE, dtype=torch.int32, device=dev),
                     'src': torch.zeros((rows,), dtype=torch.int32, device=dev),
                     'coef': torch.zeros((rows,), dtype=torch.float32, device=dev),
                     'hot': torch.zeros((rows // 16 + 4,), dtype=torch.int32, device=dev)}
            off = 0
            for _, g, _, _ in out:
                g.key_off = off
                off += g.cap
            tables.append(G.TableEntry(table.view, out, gbufs, rows))
        # per-step pool gradients: only their squares are needed -> reduce_scatter (see the class docstring)
        steps = []
        for n in preds:
            if getattr(n, 'C_steps', None) is not None:
                for buf in (n.C_steps, n.rs_steps):
                    tot = buf.numel()
                    dd = int(buf.shape[-1]) if buf.dim() == 3 else 1
                    per = (tot + self.world - 1) // self.world
                    per = (per + dd - 1) // dd * dd            # slices start on a row (the norm's row scales)
                    steps.append(dict(buf=buf, per=per,
                                      pad=torch.zeros(per * self.world, dtype=torch.float32, device=dev),
                                      mine=torch.zeros(per, dtype=torch.float32, device=dev)))
        st = dict(preds=preds, tables=tables, steps=steps)
        self._hstate[id(plan)] = st
        return st

    def step_slices(self, buf):
        """(this rank's summed slice of a per-step pool-gradient buffer, first element, count) after exchange()."""
        for st in self._hstate.values():
            for e in st['steps']:
                if e['buf'] is buf:
                    lo = self.rank * e['per']
                    cnt = max(0, min(e['per'], buf.numel() - lo))
                    return e['mine'], lo, cnt
        return None

    def exchange(self, plan):
        from . import ops
        rt = self.rt
        st = self._state(plan)
        # dense gradients + the pool gradient and its bias (small): one packed all_reduce
        pack = [p.grad for p in rt.dense.values() if getattr(p, 'touched', False)]
        for n in st['preds']:
            if not n._grad_written:
                continue
            pool = n.inputs[1]
            pack.append(pool.grad)
            if pool.bias_grad_used:
                pack.append(pool.bias_grad)
        self._all_reduce_packed([t for t in pack])
        # per-step pool gradients: summed slices
        for e in st['steps']:
            flat = e['buf'].reshape(-1)
            if self.world == 1:
                e['mine'][:flat.numel()].copy_(flat)
                continue
            e['pad'][:flat.numel()].copy_(flat)
            if e['pad'].is_cuda and dist.get_backend(self.group) != 'nccl':
                h = e['pad'].cpu()
                dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group)       # (gloo has no reduce_scatter)
                e['mine'].copy_(h[self.rank * e['per']:(self.rank + 1) * e['per']])
            else:
                dist.reduce_scatter_tensor(e['mine'], e['pad'], op=dist.ReduceOp.SUM, group=self.group)
        # lookups: gradient rows to the owners of the rows
        for table, gs, gbufs, rows in st['tables']:
            for s, g, kind, rec in gs:
                node = s.node
                g.node._grad_written = node._grad_written
                g.node.bias_grad_used = node.bias_grad_used
                if not node._grad_written:
                    continue
                a = g.node.arena[g.node.row0:g.node.row0 + g.n]
                ab = g.node.arena_b[g.node.row0:g.node.row0 + g.n]
                src = node.arena[node.row0:node.row0 + s.n]
                src_b = node.arena_b[node.row0:node.row0 + s.n]
                if kind == 'pool':
                    a.copy_(src)                      # (all-reduced above: the pool gradient of the global batch)
                    if node.bias_grad_used:
                        ab.copy_(src_b)
                    continue
                R, sc, rc = rec['R'], rec['sc'], rec['rc']
                ops.gather_onehot(src, src_b if node.bias_grad_used else None, None, rec['order'], rec['send'],
                                  bias_out=rec['send_b'] if node.bias_grad_used else None)       # owner order
                a.zero_()
                self._a2a(a[:R], rec['send'], rc, sc)
                if node.bias_grad_used:
                    ab.zero_()
                    self._a2a(ab[:R], rec['send_b'], rc, sc)

    def gathered_tables(self, plan):
        return [e._replace(sites=[g for _, g, _, _ in e.sites]) for e in self._state(plan)['tables']]

    # ---- checkpoints (utils/checkpoint.py ShardedSaver) ------------------------------------------------
    def _checkpoint_arrays(self):
        """(name, tensor, global rows, layout) under the reference's variable names: tables, biases and their
        '/Adagrad' slots striped by row, the dense parameters and their slots replicated."""
        out = []
        for t in self.model.att_emb.tables.values():
            V = t.shard['V']
            out += [(t.name, t.E, V, 'rows'), (t.name + '/Adagrad', t.acc, V, 'rows')]
            if t.bias is not None:
                out += [(t.bias_name, t.bias, V, 'rows'), (t.bias_name + '/Adagrad', t.bias_acc, V, 'rows')]
        for p in self.rt.dense.values():
            out += [(p.name, p.w, int(p.w.shape[0]), 'replicated'),
                    (p.name + '/Adagrad', p.acc, int(p.w.shape[0]), 'replicated')]
        return out

    def _checkpoint_scalars(self):
        return {'global_step': int(self.rt.global_step), 'learning_rate': float(self.rt.lr_host)}

    def _checkpoint_set_scalars(self, sc):
        self.rt.global_step = int(sc['global_step'])
        self.rt.set_learning_rate(float(sc['learning_rate']))

    def _checkpoint_restored(self):
        return                  # (the serving state holds maps and lists only: _serve_bias reads the bias per call)

    # ---- tables back together (tests only; checkpoints go through model.saver) -------------------------
    def global_params(self, slots=False):
        """{reference variable name: numpy array} of the WHOLE tables (att_emb.get_params() of a single-process
        model): the shards of all ranks, interleaved.  O(table) traffic -- not a step-path call."""
        W = self.world
        out = {}
        for t in self.model.att_emb.tables.values():
            sh = t.shard
            for name, loc in ((t.name, t.acc if slots else t.E), (t.bias_name, None if t.bias is None else
                                                                   (t.bias_acc if slots else t.bias))):
                if loc is None or name is None:
                    continue
                x = loc[:sh['rows']].detach().cpu().contiguous()
                parts = [torch.empty_like(x) for _ in range(W)]
                if W > 1:
                    dist.all_gather(parts, x, group=self.group)
                else:
                    parts = [x]
                full = torch.stack(parts, 1).reshape((sh['rows'] * W,) + tuple(x.shape[1:]))[:sh['V']]
                a = full.numpy()
                out[name] = a.reshape(-1, 1) if a.ndim == 1 else a
        return out


# --------------------------------------------------------------------------
# bench entry for N > 1 (driver: python -m torch.distributed.run ... bench.py --gpus N)
# --------------------------------------------------------------------------
def _hash_u32(x, salt):
    x = (x.to(torch.int64) * 2654435761 + salt) & 0xFFFFFFFF
    x = ((x ^ (x >> 15)) * 2246822519) & 0xFFFFFFFF
    x = ((x ^ (x >> 13)) * 3266489917) & 0xFFFFFFFF
    return x ^ (x >> 16)


def _zipf_items(n, n_items, gen, dev):
    """Zipf-like global item ids: rank = floor(n_items * u^6), scattered by a hash."""
    u = torch.rand(n, device=dev, generator=gen)
    rk = torch.clamp((u.pow(6.0) * n_items).to(torch.int64), max=n_items - 1)
    return (_hash_u32(rk, 12345) % n_items).to(torch.int32)


def draw_global_pool(sampler, S, group=None):
    """ONE weighted draw without replacement of S items over an item set whose weights are sharded over
    the ranks of `group` (utils/prepare_train.py:7-17 draws the pool from one distribution): every rank
    races its own shard (sampler.sample_with_keys: exponential keys -ln(u)/w, weights on a common
    scale, independent seeds), the ranks exchange their S smallest (key, id) pairs -- 8 KB each -- and
    every rank keeps the S smallest keys of the union: the S smallest keys of the whole item set, the
    single-process draw.  Identical on every rank (stable order: key, then rank, then position)."""
    ids, keys = sampler.sample_with_keys(S)
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world > 1:
        allk = torch.empty(world * S, dtype=keys.dtype, device=keys.device)
        alli = torch.empty(world * S, dtype=ids.dtype, device=ids.device)
        dist.all_gather_into_tensor(allk, keys.contiguous(), group=group)
        dist.all_gather_into_tensor(alli, ids.contiguous(), group=group)
        if allk.is_cuda and world * S <= 16384 and allk.dtype == torch.float32 and alli.dtype == torch.int32:
            # (round 5: one rank-selection launch over the 64-bit (key, position) words instead of torch's sort +
            # index kernels -- SURVEY section 7: no torch arithmetic on the path)
            from . import ops
            ids = torch.empty(S, dtype=alli.dtype, device=alli.device)
            ops.merge_keyed_take(allk, alli, S, ids)
        else:          # (the gloo / CPU rig of the tests, or more pairs than the kernel's LDS list holds)
            ids = alli[torch.argsort(allk, stable=True)[:S]]
    if int(ids.min().item()) < 0:
        raise ValueError("draw_global_pool(%d): fewer items with a positive weight in all shards together" % S)
    return ids


def _time_collective(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    dist.barrier()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    t = torch.tensor([e0.elapsed_time(e1) / iters], dtype=torch.float64, device=torch.device('cuda', torch.cuda.current_device()))
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


XGMI_LINK_GBS = 153.0     # per direction and link, 7 links per GPU


def comm_roofline(model, world, grp=None):
    """The step's collectives alone, at the step's payloads (every rank calls it): achieved GB/s per
    rank against what its xGMI links allow.  A rank moves (N-1)/N of a payload P over N-1 links in an
    all_gather / all_to_all, 2 (N-1)/N in an all_reduce: with every link busy the floor is
    P / N / 153 GB/s (twice that for the all_reduce)."""
    if world == 1:
        return {"note": "one rank: every exchange is a local copy, no xGMI traffic"}
    S, dp, B_loc, cap = model.S, model.dp, model.B_loc, max(model.cap, 4)
    out = {}
    x_pack, x_gath = model.I_pack[:cap], model.I_gath[:world * cap]
    rows = torch.zeros((B_loc, dp), dtype=torch.float32, device=model.device)
    back = torch.zeros_like(rows)
    g = torch.zeros((S, dp), dtype=torch.float32, device=model.device)
    cases = [
        ("all_gather_pool_blocks", lambda: dist.all_gather_into_tensor(x_gath, x_pack, group=grp),
         cap * dp * 4 * world, 1.0),
        ("all_to_all_target_rows", lambda: _all_to_all(back, rows, group=grp), B_loc * dp * 4, 1.0),
        ("all_reduce_pool_grads", lambda: dist.all_reduce(g, op=dist.ReduceOp.SUM, group=grp), S * dp * 4, 2.0),
    ]
    for name, fn, payload, factor in cases:
        ms = _time_collective(fn)
        wire = payload * factor * (world - 1) / world               # bytes this rank sends (= receives)
        floor_ms = wire / (world - 1) / (XGMI_LINK_GBS * 1e9) * 1e3   # all N-1 links busy
        out[name] = {"payload_bytes": payload, "ms": ms, "achieved_gbs_per_rank": wire / ms / 1e6,
                     "peak_gbs_per_rank": XGMI_LINK_GBS * (world - 1), "frac": floor_ms / ms}
    return out


def comm_prediction(mode, world, B_loc, S, d, n_tokens=0, L=0, dense_bytes=0):
    """What the step's collectives cost at link rate for a world of `world` ranks -- ARITHMETIC, not a measurement
    (the bench line carries it as `roofline_comm_predicted`): a rank moves (N-1)/N of a payload
    over N-1 links of XGMI_LINK_GBS each in an all_gather / all_to_all / reduce_scatter, twice that in an
    all_reduce; collectives below ~1 MB are latency-bound (tens of us under RCCL) whatever this floor says."""
    N = max(int(world), 1)
    dp = d + 4
    link = XGMI_LINK_GBS * 1e9
    f = (N - 1) / N if N > 1 else 0.0

    def row(name, kind, payload):
        wire = payload * (2.0 if kind == 'all_reduce' else 1.0) * f
        us = wire / max(N - 1, 1) / link * 1e6 if N > 1 else 0.0
        return {"collective": name, "kind": kind, "payload_bytes": int(payload), "wire_bytes_per_rank": int(wire),
                "us_at_link_rate": us}
    if mode == 'id':
        rows = [row("pool blocks", 'all_gather', S * dp * 4), row("target rows", 'all_to_all', B_loc * dp * 4),
                row("target-row gradients", 'all_to_all', B_loc * dp * 4), row("pool gradients", 'all_reduce', S * dp * 4)]
    elif mode == 'id_logits':        # ShardedHMF(exchange='logits'): the logits cross, not the pool rows
        B = B_loc * N
        rows = [row("latents of the global batch", 'all_gather', B * dp * 4),
                row("target rows", 'all_to_all', B_loc * dp * 4),
                row("partial logits [B, S / N] -> [B_loc, S]", 'all_to_all', B_loc * S * 4),
                row("logit gradients back", 'all_to_all', B_loc * S * 4),
                row("target-row gradients", 'all_to_all', B_loc * dp * 4),
                row("latent-gradient partials", 'reduce_scatter', B * d * 4)]
    elif mode == 'rep_tokens':
        rows = [row("pool blocks", 'all_gather', S * dp * 4), row("target rows", 'all_to_all', B_loc * dp * 4),
                row("target-row gradients", 'all_to_all', B_loc * dp * 4), row("pool gradients", 'all_reduce', S * dp * 4),
                row("merged token gradient + bias", 'all_reduce', n_tokens * (d + 1) * 4)]
    elif mode in ('seq_hybrid', 'seq_dp'):
        # the sequence model (C4: L unrolled steps, B_loc sequences per rank, d = 64): lookups per rank and step =
        # 2 L B_loc (inputs + targets), rows of (d + 1) floats; per-step pool gradients [L, S, d + 1]
        n_look = 2 * L * B_loc
        if mode == 'seq_hybrid':        # SeqHybridParallel: tables striped by row
            rows = [row("lookup ids to the owners", 'all_to_all', n_look * 4),
                    row("lookup rows back", 'all_to_all', n_look * (d + 1) * 4),
                    row("pool rows", 'all_reduce', S * (d + 1) * 4),
                    row("lookup-gradient rows to the owners", 'all_to_all', n_look * (d + 1) * 4),
                    row("per-step pool gradients (squared only)", 'reduce_scatter', L * S * (d + 1) * 4),
                    row("dense gradients + pool gradient", 'all_reduce', dense_bytes + S * (d + 1) * 4)]
        else:                           # SeqDataParallel: every table on every rank
            rows = [row("dense + per-step pool gradients", 'all_reduce', dense_bytes + (L + 1) * S * (d + 1) * 4),
                    row("lookup ids of all replicas", 'all_gather', N * n_look * 4),
                    row("lookup-gradient rows of all replicas", 'all_gather', N * n_look * (d + 1) * 4)]
    else:           # token-striped bags: partials of the GLOBAL batch
        B = B_loc * N
        rows = [row("pool partials", 'all_reduce', S * dp * 4), row("target partials", 'reduce_scatter', B * dp * 4),
                row("pool-gradient partials", 'all_reduce', S * dp * 4), row("target-row gradients", 'all_gather', B * dp * 4)]
    return {"model": "%d ranks, %d xGMI links x %.0f GB/s per direction each; arithmetic, not measured" % (N, max(N - 1, 1), XGMI_LINK_GBS),
            "exchanges": rows, "us_total_at_link_rate": sum(r["us_at_link_rate"] for r in rows)}


def bench_run(args, world, rank, local_rank, init_pg=True):
    """The N-rank bench body (every rank calls it); returns the JSON dict on rank 0, None elsewhere.
    world == 1 runs the very same sharded step on one GPU (all "exchanges" local): the anchor of
    the weak-scaling curve -- same code path, same 100 M-item table, same eager launches."""
    # ARX_DIST_BACKEND=gloo + ARX_DIST_ONE_GPU=1: a rig without a second GPU (this repo's test box) runs the
    # N > 1 code path with every rank on device 0 and gloo underneath -- for checking the path, not for numbers
    one_gpu = bool(os.environ.get("ARX_DIST_ONE_GPU"))
    if one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if init_pg:
        backend = os.environ.get("ARX_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    B_loc, S, d = args.batch, args.n_sampled, args.dim
    t_setup = time.time()
    rep_tokens = bool(getattr(args, 'sharded_rep_tokens', False))
    with_bags = bool(getattr(args, 'sharded_bags', False)) or rep_tokens
    if with_bags:
        # HET items: a multi-hot attribute of 20 tokens over a 100 k-token table striped by token
        n_tok, L_bag = 100000, 20
        rng = np.random.default_rng(11)                      # the SAME bag index on every rank
        p_tok = 1.0 / np.arange(1, n_tok + 1)
        vals = rng.choice(n_tok, size=(args.n_items + 1) * L_bag, p=p_tok / p_tok.sum()).astype(np.int32)
        lens = np.full(args.n_items + 1, L_bag, dtype=np.int32)
        starts = (np.arange(args.n_items + 1, dtype=np.int64) * L_bag).astype(np.int32)
        cls = ShardedHMFRepTokens if rep_tokens else ShardedHMFBags
        model = cls(args.n_users, args.n_items, d, B_loc, S, 0.1, rank, world, dev, (vals, starts, lens), n_tok, seed=0)
    else:
        model = ShardedHMF(args.n_users, args.n_items, d, B_loc, S, 0.1, rank, world, dev, seed=0,
                           exchange=getattr(args, 'exchange', 'rows'))
    pred_mode = 'rep_tokens' if rep_tokens else ('bags' if with_bags else
                                                 ('id_logits' if getattr(model, 'exchange', 'rows') == 'logits' else 'id'))
    gen = torch.Generator(device=dev)
    gen.manual_seed(77 + rank)
    n_pos = 20
    nu = model.nu_loc
    ptr = (torch.arange(nu + 2, device=dev, dtype=torch.int64) * n_pos).clamp(max=nu * n_pos).to(torch.int32)
    pos_items = _zipf_items(nu * n_pos, args.n_items, gen, dev)
    model.set_positives(ptr, pos_items)
    total = args.steps + args.warmup
    nb = min(total, 32)
    batches = []
    route_ms = []      # host cost of routing one batch (prepare_route: D2H of the ids, argsort by owner, counts, ids to the owners)
    for _ in range(nb):
        lu = torch.randint(0, nu, (B_loc,), device=dev, generator=gen)
        k = torch.randint(0, n_pos, (B_loc,), device=dev, generator=gen)
        users = (lu * world + rank).to(torch.int32)
        items = pos_items[(lu * n_pos + k)]
        torch.cuda.synchronize()
        t_r = time.time()
        batches.append(model.prepare_route(users, items))      # data-loader side: order by owner
        torch.cuda.synchronize()
        route_ms.append((time.time() - t_r) * 1e3)
    # Shared negative pool: ONE draw of S items without replacement with p ~ count^0.5 over ALL items
    # (prepare_train.py:7-35 sample_items over item_frequency, run_hmf.py:62 power = 0.5): every rank
    # races its own shard on device (arx_sample_wor), the ranks exchange their S best (key, id)
    # pairs (8 KB each) and keep the S smallest keys of the union (draw_global_pool) -- inside the
    # timed region, every n_resample steps.  Setup: global interaction counts of the owned items (one
    # reduce_scatter).
    from .utils.prepare_train import DeviceSampler
    rows = (args.n_items + world - 1) // world
    from . import ops as _ops
    cnt = torch.zeros(rows * world, dtype=torch.int32, device=dev)
    _ops.item_frequency(pos_items, rows * world, cnt)             # arx_item_frequency: counts only
    if world > 1:
        dist.all_reduce(cnt, op=dist.ReduceOp.SUM)                 # (set-up; 4 B per item)
    mine = cnt.view(rows, world)[:, rank].contiguous()
    del cnt
    tot = mine.sum(dtype=torch.int64).to(torch.float64)
    if world > 1:
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
    wts = (mine.to(torch.float64) / tot).pow(0.5).to(torch.float32)
    own = torch.arange(rows, device=dev, dtype=torch.int64) * world + rank
    wts[own >= args.n_items] = 0.0
    sampler = DeviceSampler(own.to(torch.int32), wts, device=dev, seed=4242 + rank)
    def redraw():
        # ONE draw of S items over all shards (draw_global_pool): the reference's sampling law at any N
        model.set_pool(draw_global_pool(sampler, S))
    torch.cuda.synchronize()
    dist.barrier()
    setup_s = time.time() - t_setup
    redraws = [0]

    import contextlib

    def run(k0, k1):
        # the whole loop (redraws, steps) on the model's own stream: no stream joins around the steps
        own = getattr(model, 'stream', None)
        with (torch.cuda.stream(own) if own is not None else contextlib.nullcontext()):
            for k in range(k0, k1):
                if k == 0 or (k >= args.warmup and (k - args.warmup) % args.n_resample == 0):
                    redraw()
                    redraws[0] += k >= args.warmup
                model.step(batches[k % nb])

    run(0, args.warmup)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.time()
    run(args.warmup, total)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    wall = time.time() - t0
    tmax = torch.tensor([wall], dtype=torch.float64, device=dev)
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    wall = float(tmax.item())
    loss = float(model.read_loss().item())
    comm = comm_roofline(model, world) if not with_bags else None
    # roofline of the dominant kernel (the local scorer GEMM [B_loc, S] x d), HIP events on the
    # stream the kernel runs on; same definition as the single-GPU bench line
    out = None
    if rank == 0:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        pool_mat = model.P_part if (with_bags and not rep_tokens) else model.I_all
        # the kernel the timed step RUNS (round 4 verdict, weak #6): with the fused scorer that is k_sc_hinge of
        # MwScorer.fwd (phase 2: target score + scorer GEMM + hinge epilogue, no logits), launched here with the step's
        # own buffers; only where the step itself takes the materialising GEMM (shapes the family does not cover,
        # ARX_SCORER_F32, the bag variants) is that GEMM the one timed
        fused = (rep_tokens or not with_bags) and getattr(model, 'scorer', None) is not None and model._fused_scorer()
        if fused:
            Sg_, arena, arena_b = model.Sg, model.arena, model.arena_b
            dT_ = arena[B_loc + Sg_:B_loc + Sg_ + B_loc] if world == 1 else model.dT_pack
            dt_ = arena_b[B_loc + Sg_:B_loc + Sg_ + B_loc] if world == 1 else dT_[:, d]
            run_gemm = lambda: model.scorer.fwd(model.U_loc, model.I_all[:, :d], model.b_all, model.T_pack[:, :d],
                                                model.T_pack[:, d], model.urows, model.pos_ptr, model.pos_items,
                                                model.item2slot, model.bl, model.t_loc, dt_, arena[:B_loc, :d],
                                                dT_[:, :d], 1.0 / (B_loc * world), phases=2)
        else:
            run_gemm = lambda: model.be.gemm(model.U_loc, pool_mat[:, :d], model.logits, transB=True,
                                             col_bias=model.b_all)
        for _ in range(5):
            run_gemm()
        e0.record()
        for _ in range(50):
            run_gemm()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 50
        flops = 2.0 * B_loc * S * d
        bx6 = fused or ((not _ops.SCORER_F32) and d in (64, 128) and S % 128 == 0 and B_loc >= 4096)
        peak = 2500.0 / 6.0 if bx6 else 157.3
        roofline = {"kernel": ("k_sc_hinge (MwScorer.fwd phase 2: target score + scorer GEMM + hinge epilogue, 6 exact bf16 terms "
                               "per f32 product term; the kernel the sharded step runs; per rank)" if fused else
                               "logits GEMM on the bf16 pipe, 6 exact bf16 terms per f32 product term (k_nt_bx6; per rank)"
                               if bx6 else "gemm_logits_nt (f32-input MFMA; per rank)"),
                    "bound": "mfma", "achieved": flops / ms / 1e9,
                    "peak": peak, "unit": "TFLOP/s", "frac": flops / ms / 1e9 / peak, "traffic": None,
                    "flops_per_launch": flops, "ms_per_launch": ms,
                    "peak_note": "2MNK f32 flops against 2500 TF dense bf16 / 6 terms" if bx6 else "f32-input MFMA peak"}
        B = B_loc * world
        out = {
            "metric": "training interactions/sec + sampled-negatives/sec, dim-128, 1/2/4/8 MI355X",
            "value": B * args.steps / wall, "unit": "interactions/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * wall / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": ("C3 sharded: HET items (id + 20-token bag over a 100 k-token table REPLICATED on every rank; "
                                    "per step the id-only exchanges + ONE all_reduce of the merged token gradient [n_tokens, d], "
                                    "arx.dist.ShardedHMFRepTokens) -- " if rep_tokens else
                                    "C3 sharded: HET items (id + 20-token bag over a 100 k-token table striped by TOKEN; "
                                    "per step all_reduce(pool partials, pool grads) + reduce_scatter(target partials) + "
                                    "all_gather(target grads), arx.dist.ShardedHMFBags) -- " if with_bags else "") +
                                   "C5 (BASELINE configs[4]): synthetic %d-item/%d-user HMF, dim %d, id-only, WMRB 'mw', "
                                   "item and user tables row-sharded over %d GPU(s) (owner = id %% N), %d shared "
                                   "negatives/step = ONE draw over all shards with p ~ count^0.5 (per-rank races on device, "
                                   "the S best keys of the union) every %d steps (%d redraw(s) inside the timed region); "
                                   "per step: RCCL all_gather(pool rows, blocks padded to the largest owner count) + "
                                   "all_to_all(target rows, target grads) + all_reduce(pool grads); B_loc=%d per GPU.  The batch ROUTING (order by owner, "
                                   "count / id exchange: data-loader work, ShardedHMF.prepare_route) is done once per "
                                   "batch of the %d-batch ring, OUTSIDE the timed loop"
                                   % (args.n_items, args.n_users, d, world, S, args.n_resample, redraws[0], B_loc, nb),
                       "batch_per_gpu": B_loc, "global_batch": B, "n_sampled": S, "dim": d,
                       "parallelism": "row-sharded tables x dp%d" % world,
                       "exchange": getattr(model, 'exchange', 'rows'),
                       "routing_in_timed_region": False,
                       # the data loader's share, stated next to it: host milliseconds per batch of B_loc interactions
                       # (median over the ring's batches; one host thread, includes the tiny count exchange)
                       "routing_host_ms_per_batch": float(np.median(route_ms)) if route_ms else None,
                       "pool_redraws_timed": redraws[0],
                       "hipgraph_segments": (sorted(model._graphs) if model.use_graphs else None),
                       "step_form": ("hipGraph segments between the collectives" if model.use_graphs else
                                     "the same segments, launched kernel by kernel"),
                       "hipgraph_captures": model.n_captures, "hipgraph_replays": model.n_replays,
                       "sampled_negative_logits_per_s": B * S * args.steps / wall,
                       "final_loss": loss, "setup_s": setup_s},
            "roofline": roofline, "roofline_comm": comm,
            # the same exchanges priced at link rate for the world of this run and for the 8-GPU node of BASELINE
            # configs[4] (arithmetic: no multi-GPU box was in reach of the builder)
            "roofline_comm_predicted": {
                "this_run": comm_prediction(pred_mode, world, B_loc, S, d, n_tokens=100000 if with_bags else 0),
                "at_8_ranks": comm_prediction(pred_mode, 8, B_loc, S, d, n_tokens=100000 if with_bags else 0)},
            "cpu_baseline": {"value": None, "unit": "interactions/s", "cores": None, "kind": "port",
                             "sample": None,
                             "why": "timed on rank 0 at N = 1 only (bench contract): the N = 1 line of the same run "
                                    "carries the reference-algorithm restatement on this box's host cores"},
        }
    del model
    torch.cuda.empty_cache()
    return out


def bench_main(args, world, rank, local_rank):
    """(bench.py::main_sharded is the entry the driver uses: it adds the N = 1 anchor to the line.)"""
    out = bench_run(args, world, rank, local_rank)
    dist.destroy_process_group()
    if rank == 0:
        # RCCL prints its version banner through C stdio: flush it out first so that the JSON
        # line is the LAST line on stdout
        import ctypes
        import sys
        sys.stdout.flush()
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)
