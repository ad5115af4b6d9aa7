"""score_items: what the model thinks of THESE items for THIS row -- a per-row candidate slate scored against the item
latent pool recommend scores against (arx_slate.h), optionally ordered.  The one owner of the slate rules: what a
slate may hold (check_slate), which k is legal (check_k), the scoring node (SlateScore), the order of a scored slate
(slate_order: score desc, slot asc; (-1, -inf) past the live slots) and the plan cache of the single-process models
(score_items).  Depends on graph and ops only.  Build-defined: the reference has no such call.
"""
from __future__ import annotations

import numpy as np
import torch

from . import graph as G
from . import ops

MAX_PLANS = 8           # ('score_items', C, k) plans a model keeps; the oldest goes first


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


def score_items(model, feed, candidates, k=None):
    """The body of LatentProductModel.score_items / LinearSeq.score_items.  model: has rt, _plans, output (the
    full-vocabulary logits node), batch_size; feed(): feeds the request's user (and context) placeholders as a
    recommend step does.  candidates [batch_size, C] logit indices, -1 an empty slot.  Returns float32 [mb, C] on
    the device (k None) or (ids int32 [mb, k], values float32 [mb, k]).  The plan of a (C, k) pair is cached in
    model._plans under ('score_items', C, k), at most MAX_PLANS of them."""
    out = model.output
    if type(out) is not G.Prediction:
        raise NotImplementedError("score_items: output_feat 2 / 3 pool the token SCORES of an item -- there is no "
                                  "item latent pool to score a slate against")
    latent, pool = out.inputs[0], out.inputs[1]
    cand = check_slate(candidates, model.batch_size, int(pool.shape[0]))
    C = int(cand.shape[1])
    k = check_k(k, C)
    key = ('score_items', C, k)
    entry = model._plans.get(key)
    if entry is None:
        mine = [q for q in model._plans if isinstance(q, tuple) and q[0] == 'score_items']   # (insertion order)
        for old in mine[:max(0, len(mine) - (MAX_PLANS - 1))]:
            for n in model._plans.pop(old).fetch[0].own_nodes:
                model.rt.nodes.remove(n)
        ids = G.IdsInput(model.rt, model.batch_size * C, 'slate_%d' % C)
        node = SlateScore(model.rt, latent, pool, ids, k)
        node.own_nodes = (ids, node)
        entry = model._plans[key] = G.Plan(model.rt, [node], False, [])
    node = entry.fetch[0]
    feed()
    node.inputs[2].feed(cand.reshape(-1))
    entry.run()
    if k is None:
        return node.value.clone()
    return node.top_ids.clone(), node.top_values.clone()
