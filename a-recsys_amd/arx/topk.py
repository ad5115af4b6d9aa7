"""Full-vocabulary top-k: the nodes (TopK, StreamTopK on TopKScan) and the serving rules every model shares --
when the [rows, V] logits are too big to materialise (ARX_STREAM_TOPK_BYTES), which node recommends, the excluding
twin of a node, and the chunked re-run after the fused candidate lists overflowed.  Depends on graph and ops only.
Item tags (recommend within "only this category / in stock / this market"): every logit column carries one 32-bit tag
word, every request row two words (any, all); column c is eligible for row r iff
(any[r] == 0 or tags[c] & any[r]) and tags[c] & all[r] == all[r] -- the nodes take tags= beside exclude=, the rule
itself lives in the kernels (arx_tags.h: arx_topk_tags_fill, arx_gemm_nt_topk_filter_tags).
Sampled recommend: the nodes take sample= beside tags= -- (tau [tau_rows] float32, tau_rows, seed_words int32 [2]) on
the device, or a callable giving it -- and return k DISTINCT columns drawn with probability proportional to
exp(score / tau), one after the other without replacement (Plackett-Luce), in SELECTION order: the top-k of the keys
fmaf(tau, g, score), g the Gumbel noise of arx_sample.h, a pure function of (seed, row % tau_rows, column), so the dense,
the chunked and the fused path draw the same sample.  The values are the winners' SCORES again (arx_topk_gumbel_strip),
not monotone along a row.  What a temperature and a seed may be: sample_params.
The propensity of a GIVEN ordered list under that policy (arx_list_logp.h): TopKScan.list_logp / dense_list_logp, the
node ListLogp and the body of the models' list_logprob (check_lists, list_taus, list_logp_key, list_logprob).
scan_dtype='bf16' (arx_topk_bf16.h): the fused scan's FILTER multiplies on the bf16 matrix pipe, widened by a proven
bound of the rounding error (bf16_margin_coeff), and what passes is re-scored in f32 -- ids and values stay those of the
f32 scores (TopKScan.run(scan_bf16=True); check_scan_dtype, no_scan_dtype: where the option may stand).
"""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch

from . import graph as G
from . import ops


def stream_min_bytes():
    """[rows, V] f32 logits above this many bytes are streamed, not materialised (read at every call: the
    variable may change between two model constructions)."""
    return int(os.environ.get('ARX_STREAM_TOPK_BYTES', str(1 << 30)))


def logits_too_big(rows, V):
    return rows * V * 4 > stream_min_bytes()


def streams_topk(rows, V, k, d, plain_prediction):
    """The HMF / LinearSeq rule: stream where the logits (a plain G.Prediction of a width-d latent) are too big, and
    past 65 536 items wherever the fused form applies -- it beats the materialising one at every batch size
    (V = 1 M: 1.0 against 8.1 ms at mb = 64, 3.3 against 13.8 at 1 024).  (SeqModel's rule is its own: _bucket.)"""
    fused_ok = V > 65536 and d in (32, 64, 128)
    return bool(plain_prediction and k <= 1024 and (logits_too_big(rows, V) or fused_ok))


class TopK(G.Node):
    """hmf_model.py:154 tf.nn.top_k(logits, top_N_items, sorted=True).
    exclude (optional): a callable giving (row_keys, key_rows, ex_ptr, ex_cols) (EmbeddingAttribute.exclusion_args):
    each row's excluded columns are set to -inf IN the logits before the select (nothing after this node may read
    them), and winners of value -inf (rows with fewer than k eligible columns) get index -1.
    tags (optional): a callable giving (col_tags, want_any, want_all, want_rows) (EmbeddingAttribute.tag_args), or
    that tuple: the columns ineligible for a row by their tag words are set to -inf the same way; a column must pass
    both.
    sample (optional): a callable giving (tau, tau_rows, seed_words) (EmbeddingAttribute.sample_args), or that tuple:
    the eligible logits become Gumbel keys before the select (k draws without replacement from softmax(logits / tau),
    in selection order) and the winners' values are turned back into logits after it."""

    def __init__(self, rt, logits, k, exclude=None, tags=None, sample=None, logp=False):
        super().__init__(rt, (logits.shape[0], k), (logits,))
        self.k = k
        self.exclude = exclude
        self.tags = tags
        self.sample = sample
        self.indices = torch.empty((logits.shape[0], k), dtype=torch.int32, device=rt.device)
        # logp (with sample): self.logp [rows, k], the log-probability of every draw (arx_sample_logp.h).  The keys
        # then go into a buffer of their own: the logits stay scores for the mass pass, and the values are those scores
        self.logp = self._keys = None
        if logp:
            if sample is None:
                raise ValueError("TopK: logp goes with sample")
            self.logp = torch.empty((logits.shape[0], k), dtype=torch.float32, device=rt.device)
            self._keys = torch.empty(tuple(logits.shape), dtype=torch.float32, device=rt.device)
            self._lp = LogpBuffers(logits.shape[0], k, rt.device)

    def forward(self, train):
        x = self.inputs[0].value
        if self.exclude is not None:
            ops.topk_exclude_fill(x, 0, self.exclude())
        if self.tags is not None:
            ops.topk_tags_fill(x, 0, self.tags() if callable(self.tags) else self.tags)
        sample = self.sample() if callable(self.sample) else self.sample
        keys = x
        if sample is not None:
            if self.logp is not None:
                keys = self._keys
                keys.copy_(x)
            ops.topk_gumbel_add(keys, 0, sample)
        ops.topk(keys, self.k, self.alloc_value(), self.indices)
        if self.exclude is not None or self.tags is not None or self.logp is not None:
            ops.topk_mark_empty(self.value, self.indices)     # (logp: a -inf pick is not eligible, filters or not)
        if sample is not None and self.logp is not None:
            lp = self._lp
            ops.sample_logp_sort(self.indices, lp.pk_cols, lp.pk_slot)
            ops.rest_mass_chunk(x, 0, sample, lp.picks, True, lp.m_run, lp.s_run, lp.pick_score)
            ops.sample_logp_finish(self.indices, lp.pick_score, lp.m_run, lp.s_run, 1, sample, self.logp, self.value)
        elif sample is not None:
            ops.topk_gumbel_strip(self.value, self.indices, sample)

    def list_logp(self, lists, sample, logp, values, why):
        """The log-probability of GIVEN lists int32 [rows, k] (any k in [1, 1024]) under this node's policy -- its
        logits as they stand, its exclusion lists and tags, the temperatures of `sample` (dense_list_logp,
        arx_list_logp.h).  The logits are filled with -inf at the ineligible columns, as forward() fills them."""
        own = self.__dict__.setdefault('_llb', {})
        k = int(lists.shape[1])
        if k not in own:
            own[k] = ListLogpBuffers(self.inputs[0].shape[0], k, self.rt.device)
        dense_list_logp(self.inputs[0].value, lists, self.exclude() if self.exclude is not None else None,
                        self.tags() if callable(self.tags) else self.tags, sample, own[k], logp, values, why)


class LogpBuffers(object):
    """What the mass pass of the sampled recommend's propensities keeps per request row (arx_sample_logp.h): the picks
    sorted by column with their slots, the picks' scores, the running REST pair of the materialised form and -- made
    by parts() at first use -- REST's pairs per column range of the streaming form."""

    def __init__(self, B, k, device):
        i32, f32 = torch.int32, torch.float32
        self.pk_cols = torch.empty((B, k), dtype=i32, device=device)
        self.pk_slot = torch.empty((B, k), dtype=i32, device=device)
        self.picks = (self.pk_cols, self.pk_slot)
        self.pick_score = torch.empty((B, k), dtype=f32, device=device)
        self.m_run = torch.empty(B, dtype=f32, device=device)
        self.s_run = torch.empty(B, dtype=f32, device=device)
        self._parts = None

    def parts(self, P):
        if self._parts is None or self._parts[0].shape[1] != P:
            B, dev = self.pk_cols.shape[0], self.pk_cols.device
            self._parts = (torch.empty((B, P), dtype=torch.float32, device=dev),
                           torch.empty((B, P), dtype=torch.float32, device=dev))
        return self._parts


class ListLogpBuffers(LogpBuffers):
    """LogpBuffers of a GIVEN list (arx_list_logp.h): also `clean` [B, k], the list with the entries the policy could
    not draw taken out -- what the mass pass and the finish read as the picks."""

    def __init__(self, B, k, device):
        super().__init__(B, k, device)
        self.clean = torch.empty((B, k), dtype=torch.int32, device=device)


def dense_list_logp(x, lists, ex, tags, sample, lb, logp, values, why):
    """TopKScan.list_logp over materialised logits x [B, V]: the excluded and the tag-ineligible columns are set to -inf
    IN x (nothing after this may read them as scores), then prepare, one rest_mass_chunk over [0, V), the unchanged
    finish and stamp.  lb: the ListLogpBuffers of (B, k)."""
    if ex is not None:
        ops.topk_exclude_fill(x, 0, ex)
    if tags is not None:
        ops.topk_tags_fill(x, 0, tags)
    ops.list_logp_prepare(lists, x.shape[1], ex, tags, lb.clean, why, lb.pk_cols, lb.pk_slot)
    ops.rest_mass_chunk(x, 0, sample, lb.picks, True, lb.m_run, lb.s_run, lb.pick_score)
    ops.sample_logp_finish(lb.clean, lb.pick_score, lb.m_run, lb.s_run, 1, sample, logp, values)
    ops.list_logp_stamp(lb.clean, lb.pick_score, why, logp, values)


class TopKScan(object):
    """The streaming full-vocabulary top-k of StreamTopK without a Runtime: its buffers and its algorithm on plain
    tensors, run(latent, pool, bias, ...) -- StreamTopK runs on it, and so does the per-shard stage of the row-sharded
    recommend (arx.dist.ShardedHMF.recommend), whose tables are no graph nodes.  B rows, V pool rows of width d."""

    def __init__(self, B, V, d, k, device, chunk=65536, want_lse=False, share=None):
        self.k, self.chunk = k, max(int(chunk), k)
        self._rows, self._dev = B, device
        # want_lse: also self.lse [B] = log sum exp over ALL the row's logits (seqModel.py:514-517 reports the winners'
        # softmax values exp(v - lse)): per column range out of the fused GEMM / per chunk, combined at the end
        self.want_lse = bool(want_lse)
        self.lse = torch.empty(B, dtype=torch.float32, device=device) if want_lse else None
        self._lse_parts = None
        dev = device
        f32, i32 = torch.float32, torch.int32
        self.indices = torch.empty((B, k), dtype=i32, device=dev)
        if share is not None and tuple(share._buf.shape) == (B, min(self.chunk, V)):
            self._buf = share._buf
        else:
            self._buf = torch.empty((B, min(self.chunk, V)), dtype=f32, device=dev)
        self._cv, self._ci = torch.empty((B, k), dtype=f32, device=dev), torch.empty((B, k), dtype=i32, device=dev)
        self._ov, self._oi = torch.empty((B, k), dtype=f32, device=dev), torch.empty((B, k), dtype=i32, device=dev)
        tail = V % self.chunk                       # a last chunk narrower than k keeps only `tail` entries
        kt = tail if 0 < tail < k else k
        self._tv, self._ti = torch.empty((B, kt), dtype=f32, device=dev), torch.empty((B, kt), dtype=i32, device=dev)
        self.fused = os.environ.get('ARX_TOPK_FUSED', '1') != '0' and d in (32, 64, 128)
        self.overflow = torch.zeros(1, dtype=i32, device=dev)
        self.slack, self.min_capp = 4.0, 32          # candidate segment = slack x the expected survivors, >= min_capp
        self._cand = None
        self._bf16 = None

    def _bf16_bufs(self, n, d):
        """The scratch of the bf16 scan, owned by this scan and made at the first call that asks for it: the bf16 image
        [n, d] of the pool rows past the first chunk (rows of 2 d bytes, 16-byte aligned) and their norms [n] --
        256 MB + 4 MB at 1 M x 128.  Rewritten by every run: never stale."""
        if self._bf16 is None or tuple(self._bf16[0].shape) != (n, d):
            self._bf16 = (torch.empty((n, d), dtype=torch.bfloat16, device=self._dev),
                          torch.empty(n, dtype=torch.float32, device=self._dev))
        return self._bf16

    def _cand_bufs(self, n0, V):
        """Candidate rows [B, parts * capp]: a column range's expected survivors are k (V - n0) / n0 / parts (scores in
        no particular order along the vocabulary); four times that, at least 32."""
        key = (n0, V, self.slack, self.min_capp)
        if self._cand is None or self._cand[0] != key:
            B, k, dev = self._rows, self.k, self._dev
            parts = ops.gemm_nt_topk_parts(B, V - n0)
            expect = k * (V - n0) / float(n0) / parts
            capp = self.min_capp
            while capp < self.slack * expect + self.min_capp:
                capp *= 2
            while parts * capp < k:
                capp *= 2
            cap = parts * capp
            self._cand = (key, capp, torch.empty((B, cap), dtype=torch.float32, device=dev),
                          torch.zeros((B, cap), dtype=torch.int32, device=dev),
                          torch.empty((B, k), dtype=torch.int32, device=dev), parts)
        return self._cand[1:]

    def _lse_buf(self, ncols):
        if self._lse_parts is None or self._lse_parts.shape[1] != ncols:
            B, dev = self._rows, self._dev
            self._lse_parts = torch.empty((B, ncols), dtype=torch.float32, device=dev)
            self._lse0 = torch.empty(B, dtype=torch.float32, device=dev)
        return self._lse_parts

    def overflowed(self):
        """True when the last fused run dropped candidates (device -> host read)."""
        return bool(self.fused and int(self.overflow.item()) != 0)

    @contextlib.contextmanager
    def chunked(self):
        """Inside: run() takes the chunked path; the fused setting comes back on exit, also when the body raises."""
        was, self.fused = self.fused, False
        try:
            yield self
        finally:
            self.fused = was

    def run(self, latent, pool, bias, ws, values, indices, ex=None, col_scale=None, self_col=None, tags=None,
            sample=None, logp=None, strip=True, scan_bf16=False):
        """values / indices [B, k] = the top-k of latent . pool^T + bias (bias may be None) over all V >= k pool rows;
        ex: exclusion lists (row_keys, key_rows, ex_ptr, ex_cols) or None.  ws: the GEMM workspace.
        col_scale [V] (None: every launch is the one above): the scores are (latent . pool^T) * col_scale[column] --
        cosines, with unit rows in latent and the pool's inverse row norms (similar_scan) -- and self_col [B] int32
        (optional) names the column each row leaves out (any value outside [0, V): none); a row with fewer than k
        columns left ends in (-inf, -1).  No bias, no exclusion lists and no log-sum-exp in that form.
        tags: (col_tags [V] int32, want_any, want_all, want_rows) or None -- only the columns eligible for a row by
        their tag words enter its result (composes with ex; the log-sum-exp stays over ALL the columns).  A tag too
        rare to give k eligible columns in the first chunk leaves the threshold at -inf: the fused lists may then
        overflow, and run_complete re-runs the request on the chunked path.
        sample: (tau [tau_rows], tau_rows, seed_words) or None -- the sampled recommend: per chunk the order is GEMM,
        log-sum-exp, exclusion fill, tags fill, gumbel_add, select; the fused rest goes through
        gemm_nt_topk_filter_sample (threshold and candidates are keys); after the merge and mark_empty, gumbel_strip
        turns the winners' keys back into scores.  Not with col_scale.
        logp (with sample): float32 [B, k] -- the log-probability of every draw (arx_sample_logp.h).  After the selection
        is complete (the merge and mark_empty) the mass pass runs INSTEAD of gumbel_strip: one streaming launch over
        [0, V) where the fused form applies, a second sweep of chunks otherwise (chunked() forces it, as it does for
        the selection); `values` are then the picks' exact scores.
        A keyed sample -- three more entries (col_mul, col_add, noise_rows), ops.sample_keyed -- feeds the noise other
        rows and columns (arx_sample_shard.h: shard s of W passes (W, s, the rows' user ids)); strip=False returns the
        winners' KEYS (what a merge across shards compares); not with logp.
        scan_bf16 (arx_topk_bf16.h): inside the fused form the pool rows past the first chunk are rounded to bf16
        (rows_bf16_norm, at every run: the pool may be a graph node recomputed per call), the filter runs on the bf16
        matrix pipe with its test widened by bf16_margin_coeff(d) |latent[r]| |pool[c]| -- no column whose f32 score
        beats the threshold is lost -- and cand_rescore overwrites every survivor's value with its exact f32 score in
        slate_scores' arithmetic; select, merge and mark_empty run unchanged.  indices / values: the top-k by (score
        desc, column asc) of the f32 scores -- the first chunk's from the f32 GEMM, the others' from the re-score.
        Composes with ex and tags; not with sample, col_scale or want_lse.  Outside the fused form (a width the
        kernels do not take, misaligned rows, chunked()) the run is the f32 one."""
        if scan_bf16 and (sample is not None or col_scale is not None or self.want_lse):
            raise ValueError("TopKScan.run: scan_bf16 goes with no sample, no col_scale and no log-sum-exp")
        if logp is not None and not strip:
            raise ValueError("TopKScan.run: strip=False (the keys) does not go with logp")
        V, k = pool.shape[0], self.k
        cos = col_scale is not None
        if logp is not None and sample is None:
            raise ValueError("TopKScan.run: logp goes with sample")
        if cos and sample is not None:
            raise ValueError("TopKScan.run: col_scale (the cosine form) takes no sample")
        if cos and tags is not None:
            raise ValueError("TopKScan.run: col_scale (the cosine form) takes no item tags")
        if tags is not None and int(tags[0].shape[0]) != V:
            raise ValueError("TopKScan.run: %d tag words for %d pool rows" % (int(tags[0].shape[0]), V))
        # (logp: a pick of score -inf -- a row with fewer than k finite scores -- is not eligible and becomes -1, filters
        # or not: ELIGIBLE of arx_sample_logp.h)
        empties = ex is not None or self_col is not None or tags is not None or logp is not None
        if cos and (self.want_lse or bias is not None or ex is not None):
            raise ValueError("TopKScan.run: col_scale goes with no bias, no exclusion lists and no log-sum-exp")
        if self_col is not None and not cos:
            raise ValueError("TopKScan.run: self_col belongs to the col_scale form")
        run_v, run_i = values, indices
        out_v, out_i = self._ov, self._oi
        if self.fused and V > self.chunk and pool.stride(0) % 4 == 0 and latent.stride(0) % 4 == 0:
            n0 = self.chunk
            lg = self._buf[:, :n0]
            ops.gemm(latent, pool[:n0], lg, ws, transB=True, col_bias=bias[:n0] if bias is not None else None)
            if cos:
                ops.cos_chunk_finish(lg, 0, col_scale, self_col)
            capp, cand_v, cand_i, cpos, parts = self._cand_bufs(n0, V)
            lp = None
            if self.want_lse:
                lp = self._lse_buf(parts + 1)
                ops.row_logsumexp(lg, self._lse0)               # (over the whole chunk: before the exclusion fill)
                lp[:, parts].copy_(self._lse0)
            if ex is not None:
                ops.topk_exclude_fill(lg, 0, ex)                # threshold = the k-th best ELIGIBLE column
            if tags is not None:
                ops.topk_tags_fill(lg, 0, tags)
            if sample is not None:
                ops.topk_gumbel_add(lg, 0, sample)              # threshold = the k-th best KEY
            ops.topk_chunk(lg, k, 0, run_v, run_i)
            ops.fill_f32(cand_v.view(-1), float('-inf'))
            ops.fill_i32(self.overflow, 0)
            if scan_bf16:
                img, coln = self._bf16_bufs(V - n0, int(pool.shape[1]))
                ops.rows_bf16_norm(pool[n0:], img, coln)
                ops.gemm_nt_topk_filter_bf16(latent, img, coln, bias[n0:] if bias is not None else None,
                                             run_v[:, k - 1], n0, cand_v, cand_i, capp, self.overflow,
                                             bf16_margin_coeff_f32(int(pool.shape[1])),
                                             tags=(tags[0][n0:],) + tuple(tags[1:]) if tags is not None else None, ex=ex)
                ops.cand_rescore(latent, pool, bias, cand_v, cand_i)
            elif cos:
                ops.gemm_nt_topk_filter_cos(latent, pool[n0:], col_scale[n0:], self_col, run_v[:, k - 1], n0, cand_v,
                                            cand_i, capp, self.overflow)
            elif sample is not None:
                ops.gemm_nt_topk_filter_sample(latent, pool[n0:], bias[n0:] if bias is not None else None,
                                               run_v[:, k - 1], n0, cand_v, cand_i, capp, self.overflow, sample,
                                               tags=(tags[0][n0:],) + tuple(tags[1:]) if tags is not None else None,
                                               ex=ex, lse_part=lp)
            elif tags is not None:
                ops.gemm_nt_topk_filter_tags(latent, pool[n0:], bias[n0:] if bias is not None else None,
                                             run_v[:, k - 1], n0, cand_v, cand_i, capp, self.overflow,
                                             (tags[0][n0:],) + tuple(tags[1:]), ex=ex, lse_part=lp)
            elif ex is not None:
                ops.gemm_nt_topk_filter_excl(latent, pool[n0:], bias[n0:] if bias is not None else None,
                                             run_v[:, k - 1], n0, cand_v, cand_i, capp, self.overflow, ex,
                                             lse_part=lp)
            else:
                ops.gemm_nt_topk_filter(latent, pool[n0:], bias[n0:] if bias is not None else None,
                                        run_v[:, k - 1], n0, cand_v, cand_i, capp, self.overflow, lse_part=lp)
            if self.want_lse:
                ops.row_logsumexp(lp, self.lse)
            ops.topk_chunk(cand_v, k, 0, self._cv, cpos)
            ops.take_rows_i32(cand_i, cpos, self._ci)
            ops.topk_merge(run_v, run_i, self._cv, self._ci, k, out_v, out_i)
            values.copy_(out_v)
            indices.copy_(out_i)
            if empties:
                ops.topk_mark_empty(values, indices)
            if logp is not None:
                self._logp_pass(latent, pool, bias, ws, values, indices, ex, tags, sample, logp, True)
            elif sample is not None and strip:
                ops.topk_gumbel_strip(values, indices, sample)
            return
        nch = (V + self.chunk - 1) // self.chunk
        lp = self._lse_buf(nch) if self.want_lse else None
        for c0 in range(0, V, self.chunk):
            c1 = min(V, c0 + self.chunk)
            kc = min(k, c1 - c0)
            lg = self._buf[:, :c1 - c0]
            ops.gemm(latent, pool[c0:c1], lg, ws, transB=True, col_bias=bias[c0:c1] if bias is not None else None)
            if self.want_lse:
                ops.row_logsumexp(lg, self._lse0)
                lp[:, c0 // self.chunk].copy_(self._lse0)
            if ex is not None:
                ops.topk_exclude_fill(lg, c0, ex)
            if tags is not None:
                ops.topk_tags_fill(lg, c0, tags)
            if sample is not None:
                ops.topk_gumbel_add(lg, c0, sample)
            if cos:
                ops.cos_chunk_finish(lg, c0, col_scale, self_col)
            if c0 == 0:                              # chunk >= k and V >= k: the first chunk fills all k
                ops.topk_chunk(lg, k, 0, run_v, run_i)
                continue
            cv, ci = (self._cv, self._ci) if kc == k else (self._tv, self._ti)
            ops.topk_chunk(lg, kc, c0, cv, ci)
            ops.topk_merge(run_v, run_i, cv, ci, k, out_v, out_i)
            run_v, out_v = out_v, run_v
            run_i, out_i = out_i, run_i
        if run_v.data_ptr() != values.data_ptr():
            values.copy_(run_v)
            indices.copy_(run_i)
        if empties:
            ops.topk_mark_empty(values, indices)
        if logp is not None:
            self._logp_pass(latent, pool, bias, ws, values, indices, ex, tags, sample, logp, False)
        elif sample is not None and strip:
            ops.topk_gumbel_strip(values, indices, sample)
        if self.want_lse:
            ops.row_logsumexp(lp, self.lse)

    def _logp_pass(self, latent, pool, bias, ws, values, indices, ex, tags, sample, logp, streaming):
        """The mass pass and the finish of run(logp=) over the complete selection (mass_pass), then logp and the exact
        values."""
        lb = getattr(self, '_lp', None)
        if lb is None:
            lb = self._lp = LogpBuffers(self._rows, self.k, self._dev)
        m_part, s_part, P = self.mass_pass(latent, pool, bias, ws, indices, ex, tags, sample, streaming, lb)
        ops.sample_logp_finish(indices, lb.pick_score, m_part, s_part, P, sample, logp, values)

    def mass_pass(self, latent, pool, bias, ws, cols, ex, tags, sample, streaming, lb, presorted=False):
        """REST's mass per row -- the eligible columns that are not among the row's picks `cols` [B, k] (columns of
        this pool, -1: none) -- from one streaming scan, or chunk by chunk through the logits buffer (GEMM, exclusion
        fill, tags fill, rest_mass_chunk); the picks' scores go to lb.pick_score on the way.  lb: the LogpBuffers of
        (B, k).  presorted: lb.pk_cols / lb.pk_slot already hold the picks sorted (ops.list_logp_prepare wrote them):
        no sort launch.  Returns (m_part, s_part, P): [B, P] parts, or the running pairs [B] with P = 1."""
        V = pool.shape[0]
        if not presorted:
            ops.sample_logp_sort(cols, lb.pk_cols, lb.pk_slot)
        if streaming:
            P = ops.gemm_nt_topk_parts(self._rows, V)
            m_part, s_part = lb.parts(P)
            ops.gemm_nt_rest_mass(latent, pool, bias, 0, sample, lb.picks, m_part, s_part, lb.pick_score, tags=tags,
                                  ex=ex)
            return m_part, s_part, P
        for c0 in range(0, V, self.chunk):
            c1 = min(V, c0 + self.chunk)
            lg = self._buf[:, :c1 - c0]
            ops.gemm(latent, pool[c0:c1], lg, ws, transB=True, col_bias=bias[c0:c1] if bias is not None else None)
            if ex is not None:
                ops.topk_exclude_fill(lg, c0, ex)
            if tags is not None:
                ops.topk_tags_fill(lg, c0, tags)
            ops.rest_mass_chunk(lg, c0, sample, lb.picks, c0 == 0, lb.m_run, lb.s_run, lb.pick_score)
        return lb.m_run, lb.s_run, 1

    def mass_streams(self, latent, pool):
        """Whether mass_pass over this pool may take the streaming form: where run() takes the fused one."""
        return bool(self.fused and pool.shape[0] > self.chunk and pool.stride(0) % 4 == 0
                    and latent.stride(0) % 4 == 0)

    def list_logp(self, latent, pool, bias, ws, lists, ex, tags, sample, logp, values, why, lb=None):
        """The log-probability of GIVEN lists under the sampling policy (arx_list_logp.h): lists int32 [B, k] of
        columns of this pool -- any k in [1, 1024], not tied to self.k; -1 an empty slot; anything else may stand
        there.  prepare (the entries the policy could not draw are taken out and coded in `why`), the mass pass over
        what is left (streaming where mass_streams says so, chunk by chunk otherwise; chunked() forces that), the
        unchanged finish, stamp.  logp / values float32 and why int32 [B, k]: logp 0 at -1, -inf at the codes 2-6;
        values the scores of the drawable entries, -inf elsewhere (may be None).  sample: (tau [tau_rows], tau_rows,
        ...), every tau > 0 (the callers check it on the host).  lb: the ListLogpBuffers of (B, k) (None: this scan's
        own, kept per k)."""
        k = int(lists.shape[1])
        if tags is not None and int(tags[0].shape[0]) != pool.shape[0]:
            raise ValueError("TopKScan.list_logp: %d tag words for %d pool rows" % (int(tags[0].shape[0]), pool.shape[0]))
        if lb is None:
            own = self.__dict__.setdefault('_llb', {})
            lb = own.get(k)
            if lb is None:
                lb = own[k] = ListLogpBuffers(self._rows, k, self._dev)
        ops.list_logp_prepare(lists, pool.shape[0], ex, tags, lb.clean, why, lb.pk_cols, lb.pk_slot)
        m_part, s_part, P = self.mass_pass(latent, pool, bias, ws, lb.clean, ex, tags, sample,
                                           self.mass_streams(latent, pool), lb, presorted=True)
        ops.sample_logp_finish(lb.clean, lb.pick_score, m_part, s_part, P, sample, logp, values)
        ops.list_logp_stamp(lb.clean, lb.pick_score, why, logp, values)


class StreamTopK(G.Node, TopKScan):
    """top_k over the FULL vocabulary without the [mb, V] logits -- same indices / values as
    TopK(Prediction), tf.nn.top_k's tie rule included.
    fused (round 5, the default where the scorer GEMM's small-K kernel applies): the first chunk of the pool gives
    every row its k best (GEMM -> radix select); the scorer GEMM over ALL the other columns then writes no logits --
    arx_gemm_nt_topk_filter keeps only what beats the row's k-th best so far, as short candidate lists in column order;
    one select over the lists and one merge finish.  A candidate list that overflows (scores rising along the
    vocabulary) sets a flag: overflowed() -- run_complete runs the request once more on the chunked path.
    chunked: the GEMM runs over chunks of the pool rows, every chunk keeps its k best per row (radix select) and a
    merge folds them into the running result.
    exclude (optional): a callable giving (row_keys, key_rows, ex_ptr, ex_cols) (EmbeddingAttribute.exclusion_args):
    each row's excluded columns never enter the result (the first chunk and every chunked-path chunk are filled with
    -inf at them, the fused GEMM's candidates skip them); winners of value -inf get index -1.  The log-sum-exp
    (want_lse) stays over ALL the columns.  tags (optional): a callable giving (col_tags, want_any, want_all,
    want_rows) (EmbeddingAttribute.tag_args), or that tuple: the columns ineligible for a row by their tag words never enter its
    result either (the same two places: -inf fills and the fused GEMM's survivor test).  share: another StreamTopK over the same shapes whose logits chunk buffer
    this one re-uses (plans run one after the other on one stream).  sample (optional): a callable giving (tau,
    tau_rows, seed_words) (EmbeddingAttribute.sample_args), or that tuple: the sampled recommend (TopKScan.run).
    scan_bf16: the fused scan filters on the bf16 matrix pipe and re-scores in f32 (TopKScan.run(scan_bf16=True)); not
    with sample or want_lse.  The algorithm and its buffers: TopKScan."""

    def __init__(self, rt, latent, pool, k, chunk=65536, want_lse=False, exclude=None, share=None, tags=None,
                 sample=None, logp=False, scan_bf16=False):
        G.Node.__init__(self, rt, (latent.shape[0], k), (latent, pool))
        TopKScan.__init__(self, latent.shape[0], pool.shape[0], latent.shape[1], k, rt.device, chunk=chunk,
                          want_lse=want_lse, share=share)
        self.exclude = exclude
        self.tags = tags
        self.sample = sample
        if scan_bf16 and (sample is not None or want_lse):
            raise ValueError("StreamTopK: scan_bf16 goes with no sample and no log-sum-exp")
        self.scan_bf16 = bool(scan_bf16)
        self.fused = self.fused and pool.shape[1] == latent.shape[1]
        # logp (with sample): self.logp [rows, k], the log-probability of every draw (TopKScan.run(logp=))
        if logp and sample is None:
            raise ValueError("StreamTopK: logp goes with sample")
        self.logp = torch.empty((latent.shape[0], k), dtype=torch.float32, device=rt.device) if logp else None

    def forward(self, train):
        latent, pool = self.inputs
        ex = self.exclude() if self.exclude is not None else None
        tags = self.tags() if callable(self.tags) else self.tags
        sample = self.sample() if callable(self.sample) else self.sample
        self.run(latent.value, pool.value, pool.bias_value, self.rt.ws, self.alloc_value(), self.indices, ex, tags=tags,
                 sample=sample, logp=self.logp, scan_bf16=self.scan_bf16)


def recommend_node(rt, logits, k, rows):
    """The recommend node over `logits` [rows, V]: streaming scorer + top-k (streams_topk) or tf.nn.top_k of the
    materialised logits (hmf_model.py:154)."""
    plain = isinstance(logits, G.Prediction)
    if streams_topk(rows, logits.shape[1], k, logits.inputs[0].shape[1] if plain else 0, plain):
        return StreamTopK(rt, logits.inputs[0], logits.inputs[1], k)
    return TopK(rt, logits, k)


def excluding_twin(rt, node, exclusion_args=None, tag_args=None, sample_args=None, logp=False, scan_bf16=False):
    """The twin of a recommend node that leaves columns out -- by the exclusion lists, by the item tags, or by both
    (the plain node and its plan stay as they are); a streaming twin shares the plain node's chunk buffer.
    sample_args: the SAMPLED twin (alone, or on top of either filter); logp: that twin also gives node.logp, the
    log-probability of every draw.  scan_bf16: the twin of a STREAMING node whose fused scan filters in bf16 (alone --
    the plain recommend on the bf16 pipe -- or on top of either filter; not with sample_args)."""
    if scan_bf16 and (sample_args is not None or not isinstance(node, StreamTopK)):
        raise ValueError("excluding_twin: scan_bf16 goes with a streaming node and no sample_args")
    if exclusion_args is None and tag_args is None and sample_args is None and not scan_bf16:
        raise ValueError("excluding_twin: exclusion lists, item tags or both")
    if logp and sample_args is None:
        raise ValueError("excluding_twin: logp goes with sample_args")
    if logp and not isinstance(node, StreamTopK) and type(node) is not TopK:
        raise NotImplementedError("excluding_twin: no log-probabilities for a %s node" % type(node).__name__)
    if isinstance(node, StreamTopK):
        more = {} if sample_args is None else {'sample': sample_args}
        if logp:
            more['logp'] = True
        if scan_bf16:
            more['scan_bf16'] = True
        return StreamTopK(rt, node.inputs[0], node.inputs[1], node.k, chunk=node.chunk, want_lse=node.want_lse,
                          exclude=exclusion_args, share=node, tags=tag_args, **more)
    if logp:
        return TopK(rt, node.inputs[0], node.k, exclude=exclusion_args, tags=tag_args, sample=sample_args, logp=True)
    if sample_args is not None:
        return type(node)(rt, node.inputs[0], node.k, exclude=exclusion_args, tags=tag_args, sample=sample_args)
    if tag_args is None:
        return type(node)(rt, node.inputs[0], node.k, exclude=exclusion_args)
    return type(node)(rt, node.inputs[0], node.k, exclude=exclusion_args, tags=tag_args)


def recommend_key(exclude_seen, tagged, sampled=False, logp=False, bf16=False):
    """The plan of a recommend call: 'recommend', 'recommend_ex', 'recommend_tags' or 'recommend_ex_tags'; the sampled
    twins end in '_sample', those that also give the draws' log-probabilities in '_sample_logp'; the twins whose scan
    filters in bf16 (scan_dtype='bf16') end in '_bf16' -- a plan of their own beside the f32 plan of the same filters."""
    if logp and not sampled:
        raise ValueError("recommend_key: log-probabilities belong to the sampled recommend")
    if bf16 and sampled:
        raise ValueError("recommend_key: the bf16 scan does not go with the sampled recommend")
    return 'recommend' + ('_ex' if exclude_seen else '') + ('_tags' if tagged else '') + \
        ('_sample' if sampled else '') + ('_logp' if logp else '') + ('_bf16' if bf16 else '')


def list_logp_key(exclude_seen, tagged):
    """The plans of list_logprob, beside recommend_key's: 'list_logp', 'list_logp_ex', 'list_logp_tags' or
    'list_logp_ex_tags' -- a model keeps one per (that name, k)."""
    return 'list_logp' + ('_ex' if exclude_seen else '') + ('_tags' if tagged else '')


MAX_LIST_PLANS = 8      # (list_logp_key, k) plans a model keeps; the oldest goes first


class ListLogp(G.Node):
    """value = logp float32 [rows, k]: the log-probability of the GIVEN lists under the sampling policy of the
    recommend node `source` (arx_list_logp.h) -- with self.values float32 (the scores of the drawable entries, -inf
    elsewhere) and self.why int32 (the reason codes).  source: a StreamTopK (this node scores its latent against its
    pool through the scan's mass pass: TopKScan.list_logp, the chunk buffer is the scan's) or a TopK (over its
    materialised logits: dense_list_logp).  The node owns the list placeholder self.lists (rows * k ids, row-major),
    its ListLogpBuffers and its outputs; exclude / tags / sample: callables giving the device arguments
    (EmbeddingAttribute.exclusion_args / tag_args / sample_args) or None.  tau, the tag words and the lists are
    placeholders read by the kernels: a captured plan replays with new values."""

    def __init__(self, rt, source, k, exclude=None, tags=None, sample=None):
        rows = int(source.shape[0])
        k = int(k)
        if not 1 <= k <= 1024:
            raise ValueError("ListLogp: need 1 <= k <= 1024, got %d" % k)
        if sample is None:
            raise ValueError("ListLogp: needs sample (the temperatures)")
        self.scan = source if isinstance(source, StreamTopK) else None
        if self.scan is None and type(source) is not TopK:
            raise NotImplementedError("ListLogp: no list log-probabilities for a %s node" % type(source).__name__)
        self.lists = G.IdsInput(rt, rows * k, 'list_logp_%d' % k)
        super().__init__(rt, (rows, k), tuple(source.inputs) + (self.lists,))
        self.k, self.exclude, self.tags, self.sample = k, exclude, tags, sample
        self.values = torch.empty((rows, k), dtype=torch.float32, device=rt.device)
        self.why = torch.empty((rows, k), dtype=torch.int32, device=rt.device)
        self._lb = ListLogpBuffers(rows, k, rt.device)
        self.own_nodes = (self.lists, self)

    def forward(self, train):
        lists = self.lists.value.view(self.shape)
        ex = self.exclude() if self.exclude is not None else None
        tags = self.tags() if self.tags is not None else None
        sample = self.sample()
        logp = self.alloc_value()
        if self.scan is None:
            dense_list_logp(self.inputs[0].value, lists, ex, tags, sample, self._lb, logp, self.values, self.why)
        else:
            latent, pool = self.inputs[0], self.inputs[1]
            self.scan.list_logp(latent.value, pool.value, pool.bias_value, self.rt.ws, lists, ex, tags, sample, logp,
                                self.values, self.why, lb=self._lb)


def check_lists(lists, rows, what='list_logprob'):
    """lists -> ([rows, k] int32 on the host, or a contiguous int32 device tensor), k.  Accepts a list, an integer
    array or an integer tensor [rows, k] with 1 <= k <= 1024; an id that does not fit int32 is clamped to the nearest
    int32 (it stays out of range: the kernel codes it RANGE).  ValueError for floats, bools, a wrong rank, a wrong
    row count or a k outside [1, 1024]."""
    lo, hi = -2 ** 31, 2 ** 31 - 1
    if isinstance(lists, torch.Tensor):
        if lists.dtype in (torch.bool,) or lists.is_floating_point() or lists.is_complex():
            raise ValueError("%s: lists must hold integers, got %s" % (what, lists.dtype))
        shape = tuple(lists.shape)
        a = lists
    else:
        a = np.asarray(lists)
        if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("%s: lists must hold integers, got %s" % (what, a.dtype))
        shape = tuple(a.shape)
    if len(shape) != 2 or shape[0] != rows:
        raise ValueError("%s: lists must be [%d, k], got shape %s" % (what, rows, shape))
    k = int(shape[1])
    if not 1 <= k <= 1024:
        raise ValueError("%s: need 1 <= k <= 1024 entries per list, got %d" % (what, k))
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.int32:
            a = a.clamp(lo, hi).to(torch.int32)
        return a.contiguous(), k
    if a.dtype != np.int32:
        a = np.clip(a, lo, hi) if a.dtype.kind == 'i' else np.minimum(a, hi)
    return np.ascontiguousarray(a.astype(np.int32)), k


def list_taus(temperature, rows, what='list_logprob'):
    """The temperatures of one list_logprob call as float32 [rows]: a number or one per row (sample_params' checks),
    every one > 0 as float32 -- ValueError naming the first row of temperature 0: a deterministic policy has no
    propensities (compare the list with recommend() instead)."""
    tau, _ = sample_params(temperature, 0, rows)
    zero = np.nonzero(tau <= 0)[0]
    if len(zero):
        raise ValueError("%s: sample_temperature must be > 0 (row %d has %r): a deterministic policy has no "
                         "propensities -- compare the list with recommend() instead" % (what, int(zero[0]),
                                                                                       float(tau[zero[0]])))
    return tau


def drop_list_logp_plans(model, part):
    """Drop the list_logprob plans of `model` whose key names `part` ('_ex' / '_tags'): they captured the arrays a
    prepare_recommend_exclusions / prepare_item_tags call is about to replace."""
    for key in [q for q in model._plans if isinstance(q, tuple) and str(q[0]).startswith('list_logp') and part in q[0]]:
        _drop_list_plan(model, key)


def _drop_list_plan(model, key):
    for n in model._plans.pop(key).fetch[0].own_nodes:
        model.rt.nodes.remove(n)


def list_logprob(model, feed, lists, sample_temperature, exclude_seen=False, tags_any=None, tags_all=None,
                 return_values=False, return_why=False):
    """The body of LatentProductModel.list_logprob / LinearSeq.list_logprob.  model: has rt, _plans, output (the
    full-vocabulary logits node), topk (its recommend node), att_emb, batch_size; feed(): feeds the request's user
    (and context) placeholders as a recommend step does.  Every check runs before any feed.  One plan per
    (list_logp_key, k), at most MAX_LIST_PLANS of them; tau, the tag words and the lists are fed per call.  Returns
    logprob float32 [mb, k] numpy, or the tuple (logprob[, values][, why])."""
    what = 'list_logprob'
    if type(model.output) is not G.Prediction:
        raise NotImplementedError("list_logprob: output_feat 2 / 3 pool the token SCORES of an item -- there is no "
                                  "item latent pool to take the lists' propensities against")
    rows = model.batch_size
    a, k = check_lists(lists, rows, what)
    tau = list_taus(sample_temperature, rows, what)
    m = model.att_emb
    if exclude_seen:
        m.exclusion_args()                     # ValueError when nothing was prepared
    tagged = tags_any is not None or tags_all is not None
    if tagged:
        m.tag_args()
        tag_words(tags_any, tags_all, rows, what)
    key = (list_logp_key(exclude_seen, tagged), k)
    entry = model._plans.get(key)
    if entry is None:
        mine = [q for q in model._plans if isinstance(q, tuple) and str(q[0]).startswith('list_logp')]
        for old in mine[:max(0, len(mine) - (MAX_LIST_PLANS - 1))]:
            _drop_list_plan(model, old)
        node = ListLogp(model.rt, model.topk, k, m.exclusion_args if exclude_seen else None,
                        m.tag_args if tagged else None, m.sample_args)
        entry = model._plans[key] = G.Plan(model.rt, [node], False, [])
    node = entry.fetch[0]
    feed()
    if tagged:
        m.feed_tag_words(tags_any, tags_all, what)
    m.sample_args()
    m._sample_tau.feed(tau)
    node.lists.feed(a.reshape(-1))
    entry.run()
    out = [node.value.cpu().numpy()]
    if return_values:
        out.append(node.values.cpu().numpy())
    if return_why:
        out.append(node.why.cpu().numpy())
    return out[0] if len(out) == 1 else tuple(out)


def check_return_logprob(return_logprob, recommend, sample_temperature):
    """The one rule of return_logprob on the models: the log-probabilities are those of the sampled recommend --
    ValueError (before any feed) without recommend or without sample_temperature."""
    if return_logprob and not recommend:
        raise ValueError("return_logprob=True goes with recommend=True")
    if return_logprob and sample_temperature is None:
        raise ValueError("return_logprob=True needs sample_temperature (the propensity of a sampled recommend)")


def no_return_logprob(what, return_logprob):
    """The entries that do not give the draws' log-probabilities (SeqModel.step_recommend: its rows are [L * B] and its
    values are softmax at temperature 1; every similar_items): NotImplementedError where one is asked."""
    if return_logprob:
        raise NotImplementedError("%s: return_logprob is not implemented (LatentProductModel.step and LinearSeq.step "
                                  "give the propensities of recommend(sample_temperature=))" % what)


def bf16_margin_coeff(K):
    """c(K) of the bf16 filter scan (arx_topk_bf16.h; proved in DESIGN.md section 4 item 20): for finite u, p of width
    K well inside float32's range, with u~, p~ their round-to-nearest-even bf16 images,
        |(u~ . p~ accumulated in float32) - (u . p computed in float32, slate_scores' order)| <= c(K) |u|_2 |p|_2
    -- 2^-7 + 2^-16 for the two roundings of every product, (K + 8) 2^-22 for the float32 accumulation of both sums
    (twice what round-to-nearest needs: an accumulator that truncates is covered) and the slack the norms' and the
    comparison's own roundings are paid from.  The ONE definition: the device takes it as an argument."""
    return 2.0 ** -7 * (1.0 + 2.0 ** -9) + (int(K) + 8) * 2.0 ** -22


def bf16_margin_coeff_f32(K):
    """bf16_margin_coeff(K) as the float32 the kernel takes, rounded UP."""
    c = bf16_margin_coeff(K)
    f = np.float32(c)
    if float(f) < c:
        f = np.nextafter(f, np.float32(np.inf))
    return float(f)


SCAN_DTYPES = (None, 'f32', 'bf16')


def check_scan_dtype(scan_dtype, recommend, sample_temperature, return_logprob):
    """The one rule of scan_dtype on the models -> True for the bf16 scan.  None / 'f32': the scan as it always was.
    'bf16' (with recommend=True) filters the vocabulary past the first chunk on the bf16 matrix pipe and re-scores
    what passes in f32 -- the same ids, f32 values.  ValueError (before any feed) for another word or without
    recommend; NotImplementedError naming the option it does not go with: the Gumbel keys of sample_temperature and
    the rest-mass pass of return_logprob stay f32."""
    if scan_dtype not in SCAN_DTYPES:
        raise ValueError("scan_dtype must be None, 'f32' or 'bf16', got %r" % (scan_dtype,))
    if scan_dtype != 'bf16':
        return False
    if not recommend:
        raise ValueError("scan_dtype='bf16' goes with recommend=True")
    if return_logprob:
        raise NotImplementedError("scan_dtype='bf16' is not implemented with return_logprob: the rest-mass pass of the "
                                  "propensities stays f32")
    if sample_temperature is not None:
        raise NotImplementedError("scan_dtype='bf16' is not implemented with sample_temperature: the Gumbel keys of "
                                  "the sampled recommend stay f32")
    return True


def no_scan_dtype(what, scan_dtype):
    """The entries without the bf16 scan (SeqModel.step_recommend: its log-sum-exp must stay exact over ALL the columns;
    every similar_items: the cosine form): NotImplementedError where it is asked."""
    if scan_dtype not in SCAN_DTYPES:
        raise ValueError("scan_dtype must be None, 'f32' or 'bf16', got %r" % (scan_dtype,))
    if scan_dtype == 'bf16':
        raise NotImplementedError("%s: scan_dtype='bf16' is not implemented (LatentProductModel.step and "
                                  "LinearSeq.step take it with recommend=True)" % what)


def sample_params(temperature, seed, rows):
    """The temperatures and the seed of one sampled recommend call as what the device placeholders hold: float32
    [rows] and the two int32 seed words (low, high).  temperature: one number for every row or one per row, finite
    and >= 0 (0: that row is the plain top-k); seed: an int in [0, 2^63).  ValueError for a negative, NaN or infinite
    temperature, a bool, a non-number, a wrong length, or a seed outside the range."""
    t = temperature.cpu().numpy() if isinstance(temperature, torch.Tensor) else temperature
    a = np.asarray(t)
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError("sample_temperature must be a number or %d numbers, one per row" % rows)
    if a.ndim > 1 or (a.ndim == 1 and len(a) != rows):
        raise ValueError("sample_temperature must be one number or %d numbers, one per row" % rows)
    a = a.astype(np.float64)
    if not np.all(np.isfinite(a)) or np.any(a < 0):
        raise ValueError("sample_temperature must be finite and >= 0")
    with np.errstate(over='ignore'):
        tau = np.ascontiguousarray(np.broadcast_to(a, (rows,)).astype(np.float32))
    if not np.all(np.isfinite(tau)):
        raise ValueError("sample_temperature must be finite in float32")
    if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 63:
        raise ValueError("sample_seed must be an int in [0, 2^63)")
    seed = int(seed)
    words = np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint32).view(np.int32)
    return tau, words


def tag_words(tags_any, tags_all, rows, what='recommend'):
    """The two request words per row as int32 BIT PATTERNS [rows] (what the device placeholders hold).  Each of
    tags_any / tags_all: None (0: no constraint), an int (one word for every row) or a length-`rows` integer array;
    ValueError for a word outside [0, 2^32), a non-integer or a wrong length."""
    out = []
    for name, w in (('tags_any', tags_any), ('tags_all', tags_all)):
        if isinstance(w, torch.Tensor):
            w = w.cpu().numpy()
        a = np.asarray(0 if w is None else w)
        if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
            if a.dtype != object or not all(isinstance(x, (int, np.integer)) for x in a.reshape(-1)):
                raise ValueError("%s: %s must hold integers (32-bit tag words)" % (what, name))
        if a.ndim > 1 or (a.ndim == 1 and len(a) != rows):
            raise ValueError("%s: %s must be one word or %d words, one per row" % (what, name, rows))
        flat = a.reshape(-1)
        if len(flat) and (min(flat) < 0 or max(flat) >= 2 ** 32):      # (one word for no rows is checked too)
            raise ValueError("%s: %s words must lie in [0, 2^32)" % (what, name))
        if a.ndim == 0:
            a = np.full(rows, a.item(), dtype=object if a.dtype == object else a.dtype)
        out.append(np.ascontiguousarray(a.astype(np.uint32)).view(np.int32))
    return out[0], out[1]


def run_complete(scan, run, forget=None):
    """run(); where the fused candidate lists of `scan` overflowed, once more on the chunked path.  forget() drops
    a captured plan: one captured with the fused launch sequence must not replay the chunked one, nor the other way
    round.  A node without overflowed() (a dense top-k) runs once.  Returns what the last run() returned."""
    forget = forget or (lambda: None)
    out = run()
    if getattr(scan, 'overflowed', lambda: False)():
        forget()
        try:
            with scan.chunked():
                out = run()
        finally:
            forget()
    return out


def similar_scan(scan, table, query_rows, values, indices, ws, include_self, self_cols=None):
    """Cosine nearest neighbours of table rows over the whole table -- the one place the rules of similar_items live
    (EmbeddingAttribute.similar_items, arx.dist HipBackend.shard_similar).  scan: a TopKScan(B, V, d, k) without
    want_lse; table [V, d]; query_rows [B] int32: the rows asked about (< 0: a zero query).  In order: the inverse row
    norms of the table (one streaming read, recomputed at every call: no cache to go stale), the queries as unit rows
    (arx_gather_rows_unit), the scan -- once more on the chunked path where the fused candidate lists overflowed.
    values / indices [B, k]: (cosine desc, row asc); include_self False leaves each query's own row out; (-inf, -1)
    where fewer than k rows are left.  A zero row has cosine 0 with everything, also as a query.
    The sharded caller's queries come from their owners as unit rows already: query_rows is then that float32 [B, d]
    tensor (nothing is gathered here) and self_cols [B] int32 names the LOCAL column each row leaves out (anything
    outside [0, V): none; ignored with include_self)."""
    V = int(table.shape[0])
    inv = getattr(scan, '_inv_norm', None)
    if inv is None or int(inv.shape[0]) != V:
        inv = scan._inv_norm = torch.empty(V, dtype=torch.float32, device=table.device)
    ops.rows_inv_norm(table, inv)
    if query_rows.dtype == torch.float32:
        q = query_rows
    else:
        q = getattr(scan, '_unit_rows', None)
        if q is None or tuple(q.shape) != (int(query_rows.shape[0]), int(table.shape[1])):
            q = scan._unit_rows = torch.empty((int(query_rows.shape[0]), int(table.shape[1])), dtype=torch.float32,
                                              device=table.device)
        ops.gather_rows_unit(table, query_rows, q)
        if self_cols is None:
            self_cols = query_rows
    sc = None if include_self else self_cols
    if sc is None and not include_self:
        raise ValueError("similar_scan: unit-row queries need self_cols to leave their own rows out")
    run_complete(scan, lambda: scan.run(q, table, None, ws, values, indices, col_scale=inv, self_col=sc))
