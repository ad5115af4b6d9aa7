"""score_items: what the model thinks of THESE items for THIS row -- a per-row candidate slate scored against the item
latent pool recommend scores against (arx_slate.h), optionally ordered.  The one owner of the slate rules: what a
slate may hold (check_slate), which k is legal (check_k), the scoring node (SlateScore), the order of a scored slate
(slate_order: score desc, slot asc; (-1, -inf) past the live slots) and the plan cache of the single-process models
(score_items).  Also the diversified order of a scored slate (arx_diverse.h): what lambda and a per-group cap may be
(check_diversify, check_max_per_group), the item groups by logit column (item_group_ids, prepare_item_groups) and the
re-rank node (SlateDiverse).  And the sampled slate (arx_slate_sample.h): k draws from softmax(score / tau) over the
row's distinct candidates with their log-probabilities (SlateSample; what a temperature and a seed may be is
topk.sample_params, the placeholders are the sampled recommend's).  Depends on graph, ops and topk only.
Build-defined: the reference has no such call.
"""
from __future__ import annotations

import numpy as np
import torch

from . import graph as G
from . import ops
from .topk import sample_params

MAX_PLANS = 8           # ('score_items', C, k[, 'mmr', capped | 'sample']) plans a model keeps; the oldest goes first


def check_slate(candidates, rows, V, what='score_items'):
    """candidates -> contiguous int32 array [rows, C], C >= 1, every entry -1 (an empty slot) or in [0, V).
    Accepts an integer array or tensor; ValueError for anything else (wrong rank or rows, floats, bools, an id
    outside the range)."""
    if isinstance(candidates, torch.Tensor):
        candidates = candidates.detach().cpu().numpy()
    a = np.asarray(candidates)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s: candidates must hold integers, got %s" % (what, a.dtype))
    if a.ndim != 2 or a.shape[0] != rows:
        raise ValueError("%s: candidates must be [%d, C], got shape %s" % (what, rows, tuple(a.shape)))
    if a.shape[1] < 1:
        raise ValueError("%s: a slate needs at least one slot (C >= 1)" % what)
    if a.size and (a.min() < -1 or a.max() >= V):
        raise ValueError("%s: every candidate must be -1 (an empty slot) or in [0, %d)" % (what, V))
    return np.ascontiguousarray(a.astype(np.int32))


def check_k(k, C, what='score_items'):
    """None (scores only) or an int in [1, min(1024, C)] (arx_topk's limit); ValueError otherwise."""
    if k is None:
        return None
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= min(1024, C):
        raise ValueError("%s: need 1 <= k <= min(1024, %d), got %r" % (what, C, k))
    return int(k)


def slate_order(scores, cand, k, values, pos, ids):
    """values / ids [rows, k] = the k best slots of scores [rows, C] by (score desc, slot asc) and the candidate ids
    cand [rows, C] int32 they hold; (-inf, -1) where a row has fewer than k slots above -inf.  pos [rows, k] int32 is
    scratch (the winning slot positions).  arx_take_rows_i32 has no guard for a negative position: take first, mark
    afterwards."""
    ops.topk(scores, k, values, pos)
    ops.take_rows_i32(cand, pos, ids)
    ops.topk_mark_empty(values, ids)


def _per_row(x, rows, name, what):
    """x, a real scalar or one value per row (no bools) -> a 1-D numpy array of `rows` entries, dtype untouched."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
        raise ValueError("%s: %s must be a number or one number per row, got %r" % (what, name, x))
    if a.ndim == 0:
        a = np.full(rows, a[()])
    if a.ndim != 1 or a.shape[0] != rows:
        raise ValueError("%s: %s needs one value or %d (one per row), got shape %s" % (what, name, rows, tuple(a.shape)))
    return a


def check_diversify(lam, rows, what='score_items'):
    """lambda of the MMR objective, a scalar or one per row -> float32 [rows]; ValueError for a value outside [0, 1],
    a NaN, a bool or a wrong length.  1 is the plain order by score, 0 looks at the distance to the picks only."""
    a = _per_row(lam, rows, 'diversify', what)
    if not np.issubdtype(a.dtype, np.floating):
        a = a.astype(np.float64)
    if a.size and not ((a >= 0) & (a <= 1)).all():             # (a NaN compares false)
        raise ValueError("%s: diversify must lie in [0, 1], got %r" % (what, lam))
    return np.ascontiguousarray(a.astype(np.float32))


def check_max_per_group(m, rows, what='score_items'):
    """The cap on the picks of one group, a scalar or one per row -> int32 [rows]; ValueError for a value below 1, a
    non-integer, a bool or a wrong length."""
    a = _per_row(m, rows, 'max_per_group', what)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s: max_per_group must hold integers, got %s" % (what, a.dtype))
    if a.size and a.min() < 1:
        raise ValueError("%s: max_per_group must be >= 1, got %r" % (what, m))
    return np.ascontiguousarray(np.minimum(a, 2 ** 31 - 1).astype(np.int32))


def item_group_ids(groups, item2logit, n_logits):
    """One group id per LOGIT column, int32 [n_logits], for max_per_group (arx_diverse.h).  groups, per ITEM index: an
    integer array [n_items] or {item_index: group}; a negative group is 'no group' (never capped).  Items go through
    item2logit (a numpy array, -1 where an item has no logit) the way item_tag_words takes them: an item without a
    logit is skipped, a column without an item gets -1; where two items share a column the later item's group holds."""
    item2logit = np.asarray(item2logit)
    if isinstance(groups, dict):
        items = np.fromiter(groups.keys(), dtype=np.int64, count=len(groups))
        vals = np.asarray(list(groups.values()))
        if len(items) and items.min() < 0:
            raise ValueError("item groups: negative item index")
        if not len(items):
            vals = np.zeros(0, dtype=np.int64)
    else:
        vals = groups.cpu().numpy() if isinstance(groups, torch.Tensor) else np.asarray(groups)
        items = np.arange(len(vals), dtype=np.int64) if vals.ndim == 1 else None
    if vals.ndim != 1 or vals.dtype == np.bool_ or not np.issubdtype(vals.dtype, np.integer):
        raise ValueError("item groups: an integer array [n_items] or a {item_index: group} dict")
    if len(vals) and (vals.min() < -2 ** 31 or vals.max() >= 2 ** 31):
        raise ValueError("item groups: ids must fit int32")
    ok = items < len(item2logit)
    items, vals = items[ok], vals[ok]
    cols = item2logit[items].astype(np.int64)
    ok = (cols >= 0) & (cols < n_logits)
    out = np.full(n_logits, -1, dtype=np.int32)
    out[cols[ok]] = vals[ok].astype(np.int32)
    return out


def prepare_item_groups(model, groups):
    """The body of model.prepare_item_groups: map through the model's item_ind2logit_ind, upload once, and drop the
    capped plans (they hold the old array)."""
    att = model.att_emb
    if att._item2logit_np is None:
        raise ValueError("item groups need item_ind2logit_ind")
    ids = item_group_ids(groups, att._item2logit_np, att.logit_size)
    for key in [q for q in model._plans if isinstance(q, tuple) and q[0] == 'score_items' and len(q) == 5 and q[4]]:
        _drop_plan(model, key)
    model._item_groups = model.rt.upload(ids, torch.int32)


def _drop_plan(model, key):
    for n in model._plans.pop(key).fetch[0].own_nodes:
        model.rt.nodes.remove(n)


class SlateScore(G.Node):
    """value [rows, C] = latent_r . pool[c] + bias[c] for the candidates c of row r (-inf at an empty slot).
    inputs: the latent node [rows, d], the pool EntityEmbed [V, d] (with its bias) and an IdsInput of rows * C
    candidates (row-major).  With k also top_values / top_ids [rows, k] (slate_order).  Every buffer is static: a
    G.Plan over this node captures and replays like the recommend plans."""

    def __init__(self, rt, latent, pool, cand_ids, k=None):
        rows = int(latent.shape[0])
        n = int(cand_ids.shape[0])
        if rows < 1 or n < rows or n % rows:
            raise ValueError("SlateScore: %d candidates for %d rows" % (n, rows))
        if int(latent.shape[1]) != int(pool.shape[1]):
            raise ValueError("SlateScore: latent width %d against pool width %d" % (latent.shape[1], pool.shape[1]))
        C = n // rows
        super().__init__(rt, (rows, C), (latent, pool, cand_ids))
        self.k = check_k(k, C, 'SlateScore')
        self.top_values = self.top_ids = self._pos = None
        if self.k is not None:
            self.top_values = torch.empty((rows, self.k), dtype=torch.float32, device=rt.device)
            self.top_ids = torch.empty((rows, self.k), dtype=torch.int32, device=rt.device)
            self._pos = torch.empty((rows, self.k), dtype=torch.int32, device=rt.device)

    def forward(self, train):
        latent, pool, ids = self.inputs
        cand = ids.value.view(self.shape)
        ops.slate_scores(latent.value, pool.value, pool.bias_value, cand, self.alloc_value())
        if self.k is not None:
            slate_order(self.value, cand, self.k, self.top_values, self._pos, self.top_ids)


class SlateDiverse(G.Node):
    """top_ids / top_values / pos [rows, k] = the greedy MMR order of the slate a SlateScore node scored
    (arx_slate_mmr): pick t maximises lam * rel - (1 - lam) * (largest cosine to picks 0 .. t - 1), cosines between
    the rows of the pool EntityEmbed; (-1, -inf, -1) past the last pick.  groups: int32 [V] on the device (one id per
    pool row) -> at most cap[r] picks of one group in row r.  lam (FloatInput [rows]) and cap (IdsInput [rows]) are
    placeholders read by the kernel: a captured plan replays with new values.  Every buffer is static."""

    def __init__(self, rt, slate_score_node, pool, k, groups=None):
        rows, C = slate_score_node.shape
        k = check_k(k, C, 'SlateDiverse')
        if k is None:
            raise ValueError("SlateDiverse: k is required")
        if not ops.slate_mmr_supported(C, int(pool.shape[1])):
            raise ValueError("SlateDiverse: arx_slate_mmr_supported refuses C=%d, d=%d" % (C, pool.shape[1]))
        self.lam = G.FloatInput(rt, (rows,), 'mmr_lam_%d' % C)
        self.cap = G.IdsInput(rt, rows, 'mmr_cap_%d' % C) if groups is not None else None
        super().__init__(rt, (rows, k), (slate_score_node, pool, self.lam) + (() if self.cap is None else (self.cap,)))
        self.k, self.groups = k, groups
        self.top_values = torch.empty((rows, k), dtype=torch.float32, device=rt.device)
        self.top_ids = torch.empty((rows, k), dtype=torch.int32, device=rt.device)
        self.pos = torch.empty((rows, k), dtype=torch.int32, device=rt.device)

    def forward(self, train):
        sl, pool = self.inputs[0], self.inputs[1]
        cand = sl.inputs[2].value.view(sl.shape)
        ops.slate_mmr(pool.value, cand, sl.value, self.lam.value, self.groups,
                      self.cap.value if self.cap is not None else None, self.k, self.top_ids, self.top_values,
                      self.pos)


class SlateSample(G.Node):
    """top_ids / top_values / pos / logp [rows, k] = k draws without replacement from softmax(score / tau) over the
    distinct live candidates of the slate a SlateScore node scored, in selection order (arx_slate_sample): the top-k of
    the keys fmaf(tau, g, score), g the noise of the sampled recommend, a function of (seed, row, item) -- the draw
    does not depend on the order of the slate; values are the scores themselves; logp[t] is the log-probability of pick
    t given picks 0 .. t - 1 (0 on a tau == 0 row); (-1, -inf, -1, 0) past the last competitor.  sample: a callable
    giving (tau [tau_rows], tau_rows, seed_words int32 [2]) on the device (EmbeddingAttribute.sample_args), or that
    tuple: placeholders read by the kernel, a captured plan replays with new values.  Every buffer is static."""

    def __init__(self, rt, slate_score_node, k, sample):
        rows, C = slate_score_node.shape
        k = check_k(k, C, 'SlateSample')
        if k is None:
            raise ValueError("SlateSample: k is required")
        if not ops.slate_sample_supported(C):
            raise ValueError("SlateSample: arx_slate_sample_supported refuses C=%d" % C)
        super().__init__(rt, (rows, k), (slate_score_node,))
        self.k, self.sample = k, sample
        self.top_values = torch.empty((rows, k), dtype=torch.float32, device=rt.device)
        self.top_ids = torch.empty((rows, k), dtype=torch.int32, device=rt.device)
        self.pos = torch.empty((rows, k), dtype=torch.int32, device=rt.device)
        self.logp = torch.empty((rows, k), dtype=torch.float32, device=rt.device)

    def forward(self, train):
        sl = self.inputs[0]
        cand = sl.inputs[2].value.view(sl.shape)
        sample = self.sample() if callable(self.sample) else self.sample
        ops.slate_sample(cand, sl.value, sample, self.k, self.top_ids, self.top_values, self.pos, self.logp)


def score_items(model, feed, candidates, k=None, diversify=None, max_per_group=None, sample_temperature=None,
                sample_seed=None, return_logprob=False):
    """The body of LatentProductModel.score_items / LinearSeq.score_items.  model: has rt, _plans, output (the
    full-vocabulary logits node), batch_size; feed(): feeds the request's user (and context) placeholders as a
    recommend step does.  candidates [batch_size, C] logit indices, -1 an empty slot.  Returns float32 [mb, C] on
    the device (k None) or (ids int32 [mb, k], values float32 [mb, k]).  The plan of a (C, k) pair is cached in
    model._plans under ('score_items', C, k), at most MAX_PLANS of them.
    diversify (lambda in [0, 1], a scalar or one per row) and / or max_per_group (a cap >= 1 on the picks of one item
    group, after model.prepare_item_groups): k is required and (ids, values) come in SELECTION order of the greedy MMR
    re-rank (SlateDiverse); a cap alone means lambda = 1, the best k by score under the cap.  Those plans are keyed
    ('score_items', C, k, 'mmr', capped) and count toward MAX_PLANS; lambda and the cap are fed per call.
    sample_temperature (topk.sample_params: a number >= 0 or one per row): k is required and (ids, values) are k draws
    without replacement from softmax(score / tau) over the row's distinct live candidates, in selection order
    (SlateSample); return_logprob adds logprob float32 [mb, k], the log-probability of each draw given those before it.
    sample_seed: an int in [0, 2^63), None takes model.att_emb's draw counter (next_sample_seed: a refused call does not
    move it).  One plan per (C, k), keyed ('score_items', C, k, 'sample') -- four entries: prepare_item_groups tells the
    capped plans by their five; the temperature and the seed are the placeholders of att_emb.sample_args, fed per
    call.  ValueError, before any feed: a temperature without k or together with diversify / max_per_group, a seed or
    return_logprob without a temperature, a C outside arx_slate_sample_supported."""
    out = model.output
    if type(out) is not G.Prediction:
        raise NotImplementedError("score_items: output_feat 2 / 3 pool the token SCORES of an item -- there is no "
                                  "item latent pool to score a slate against")
    latent, pool = out.inputs[0], out.inputs[1]
    cand = check_slate(candidates, model.batch_size, int(pool.shape[0]))
    C = int(cand.shape[1])
    k = check_k(k, C)
    mmr = diversify is not None or max_per_group is not None
    sampled = sample_temperature is not None
    if not sampled and (sample_seed is not None or return_logprob):
        raise ValueError("score_items: sample_seed / return_logprob need sample_temperature")
    if sampled:
        if k is None:
            raise ValueError("score_items: sample_temperature needs k")
        if mmr:
            raise ValueError("score_items: sample_temperature does not combine with diversify / max_per_group")
        if not ops.slate_sample_supported(C):
            raise ValueError("score_items: sample_temperature over C=%d slots: outside the envelope of "
                             "arx_slate_sample_supported" % C)
        sample_params(sample_temperature, 0 if sample_seed is None else sample_seed, model.batch_size)
    lam = cap = groups = None
    if mmr:
        if k is None:
            raise ValueError("score_items: diversify / max_per_group need k")
        lam = check_diversify(1.0 if diversify is None else diversify, model.batch_size)
        if max_per_group is not None:
            cap = check_max_per_group(max_per_group, model.batch_size)
            groups = getattr(model, '_item_groups', None)
            if groups is None:
                raise ValueError("score_items: max_per_group needs prepare_item_groups() first")
        if not ops.slate_mmr_supported(C, int(pool.shape[1])):
            raise ValueError("score_items: diversify / max_per_group over C=%d slots of d=%d: outside the envelope of "
                             "arx_slate_mmr_supported" % (C, pool.shape[1]))
    key = ('score_items', C, k, 'mmr', cap is not None) if mmr else \
        ('score_items', C, k, 'sample') if sampled else ('score_items', C, k)
    entry = model._plans.get(key)
    if entry is None:
        mine = [q for q in model._plans if isinstance(q, tuple) and q[0] == 'score_items']   # (insertion order)
        for old in mine[:max(0, len(mine) - (MAX_PLANS - 1))]:
            _drop_plan(model, old)
        ids = G.IdsInput(model.rt, model.batch_size * C, 'slate_%d' % C)
        if mmr:
            sl = SlateScore(model.rt, latent, pool, ids, None)
            node = SlateDiverse(model.rt, sl, pool, k, groups)
            node.own_nodes = (ids, sl, node.lam) + ((node.cap,) if node.cap is not None else ()) + (node,)
        elif sampled:
            sl = SlateScore(model.rt, latent, pool, ids, None)
            node = SlateSample(model.rt, sl, k, model.att_emb.sample_args)
            node.own_nodes = (ids, sl, node)                   # (the placeholders are att_emb's, shared with recommend)
        else:
            node = SlateScore(model.rt, latent, pool, ids, k)
            node.own_nodes = (ids, node)
        entry = model._plans[key] = G.Plan(model.rt, [node], False, [])
    node = entry.fetch[0]
    feed()
    if sampled:
        model.att_emb.feed_sample(sample_temperature, sample_seed)
        node.inputs[0].inputs[2].feed(cand.reshape(-1))
    elif mmr:
        node.inputs[0].inputs[2].feed(cand.reshape(-1))
        node.lam.feed(lam)
        if cap is not None:
            node.cap.feed(cap)
    else:
        node.inputs[2].feed(cand.reshape(-1))
    entry.run()
    if k is None:
        return node.value.clone()
    if return_logprob:
        return node.top_ids.clone(), node.top_values.clone(), node.logp.clone()
    return node.top_ids.clone(), node.top_values.clone()
