"""explain_items: WHY did this item get this score for this row -- the score of score_items taken apart into the
contributions of the item's output features (its own id row, its genre, the bag of its title) and of the single tokens
of its bags (arx_explain.h).  An item's latent is the mean over its F output features of an id row or a bag mean, so

    score(r, c) = 1/F * sum_f s_f(r, c)
       cat feature f:     s_f = u_r . E_f[m_f(c)] + b_f[m_f(c)]
       mulhot feature f:  s_f = 1/len_f(c) * sum_t ( u_r . E_f[v_{f,c,t}] + b_f[v_{f,c,t}] )

is an exact sum: the explanation is a decomposition of what the model computes, not a heuristic laid over it.  The one
owner of the rules: which `top` is legal (check_top), the node (ExplainSlate), the result (Explanation) and the plan
cache of the single-process models (explain_items).  Depends on graph, ops and slate only.  Build-defined: the
reference has no such call.  Out of scope: SeqModel; the sharded models (their tables are striped); a "most negative"
or absolute-value order of the tokens; merging the repeats of a token.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import graph as G
from . import ops
from .slate import SlateScore, check_slate

MAX_PLANS = 4           # ('explain_items', C, top) plans a model keeps; the oldest goes first

Explanation = collections.namedtuple(
    'Explanation', ['score', 'feature', 'bias', 'token_value', 'token_id', 'token_feature', 'features'])
Explanation.__doc__ = """What explain_items returns; device tensors, cloned.
score [mb, C] float32: score_items' score, bit for bit (-inf at an empty slot).
feature [mb, C, F] float32: the contribution 1/F * s_f of output feature f, bias included; the sum over f is the score
    (up to float32 rounding); 0 at an empty slot.
bias [mb, C] float32: the bias part of the score, 1/F * sum_f of the bias terms -- the pool bias of the item; score
    minus this is the personalised part.
token_value / token_id / token_feature [mb, C, top]: the `top` largest token contributions
    1/(F * len) * (u . E_f[v] + b_f[v]) over all bag positions of all mulhot features of the item, by (value desc,
    feature asc, bag position asc); token_id is the row of the feature's table, token_feature the column of `feature`;
    (-inf, -1, -1) past the last position and at an empty slot.  None with top = 0.
features: ((kind, table_name), ...) in the column order of `feature`."""


def check_top(top, what='explain_items'):
    """An int in [0, 16] (arx_explain.h's limit), no bools; ValueError otherwise."""
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 0 <= int(top) <= ops.EXPLAIN_MAX_TOP:
        raise ValueError("%s: need an int 0 <= top <= %d, got %r" % (what, ops.EXPLAIN_MAX_TOP, top))
    return int(top)


class ExplainSlate(G.Node):
    """feature [rows, C, F], bias [rows, C] and token_value / token_id / token_feature [rows, C, top] (None with
    top = 0) of the candidates of every row (arx_explain_slate).  inputs: the latent node [rows, d], the pool
    EntityEmbed (mean-combined, out_scale 1: its feats and with_bias give the feature descriptors) and an IdsInput of
    rows * C candidates (row-major).  Every buffer is static: a G.Plan over this node captures and replays."""

    def __init__(self, rt, latent, pool, cand_ids, top):
        rows = int(latent.shape[0])
        n = int(cand_ids.shape[0])
        if rows < 1 or n < rows or n % rows:
            raise ValueError("ExplainSlate: %d candidates for %d rows" % (n, rows))
        if int(latent.shape[1]) != int(pool.shape[1]):
            raise ValueError("ExplainSlate: latent width %d against pool width %d" % (latent.shape[1], pool.shape[1]))
        if getattr(pool, 'concat', False) or getattr(pool, 'out_scale', 1.0) != 1.0 or not hasattr(pool, 'feats'):
            raise NotImplementedError("ExplainSlate: the pool must be a mean-combined EntityEmbed with out_scale 1")
        C = n // rows
        F = len(pool.feats)
        super().__init__(rt, (rows, C, F), (latent, pool, cand_ids))
        self.top = check_top(top, 'ExplainSlate')
        self.es = ops.ExplainSet(pool.feats, int(pool.shape[0]), with_bias=bool(pool.with_bias))
        self.features = tuple((f.kind, f.table.name) for f in pool.feats)
        dev = rt.device
        self.bias = torch.empty((rows, C), dtype=torch.float32, device=dev)
        self.token_value = self.token_id = self.token_feature = None
        if self.top:
            self.token_value = torch.empty((rows, C, self.top), dtype=torch.float32, device=dev)
            self.token_id = torch.empty((rows, C, self.top), dtype=torch.int32, device=dev)
            self.token_feature = torch.empty((rows, C, self.top), dtype=torch.int32, device=dev)

    def forward(self, train):
        latent, _, ids = self.inputs
        cand = ids.value.view(self.shape[:2])
        ops.explain_slate(latent.value, cand, self.es, self.top, self.alloc_value(), self.bias, self.token_value,
                          self.token_id, self.token_feature)


def _drop_plan(model, key):
    for n in model._plans.pop(key).fetch[0].own_nodes:
        model.rt.nodes.remove(n)


def explain_items(model, feed, items, top=3):
    """The body of LatentProductModel.explain_items / LinearSeq.explain_items.  model: has rt, _plans, output (the
    full-vocabulary logits node), batch_size; feed(): feeds the request's user (and context) placeholders as a
    recommend step does.  items [batch_size, C] logit indices, -1 an empty slot (slate.check_slate).  Returns an
    Explanation.  One plan per (C, top), cached in model._plans under ('explain_items', C, top), at most MAX_PLANS of
    them; it holds an ExplainSlate and a SlateScore node over the same ids, so `score` is score_items' score bit for
    bit.  Every check runs before any feed."""
    out = model.output
    if type(out) is not G.Prediction:
        raise NotImplementedError("explain_items: output_feat 2 / 3 pool the token SCORES of an item -- there is no "
                                  "item latent pool to score a slate against")
    latent, pool = out.inputs[0], out.inputs[1]
    cand = check_slate(items, model.batch_size, int(pool.shape[0]), 'explain_items')
    C = int(cand.shape[1])
    top = check_top(top)
    key = ('explain_items', C, top)
    entry = model._plans.get(key)
    if entry is None:
        mine = [q for q in model._plans if isinstance(q, tuple) and q[0] == 'explain_items']   # (insertion order)
        for old in mine[:max(0, len(mine) - (MAX_PLANS - 1))]:
            _drop_plan(model, old)
        ids = G.IdsInput(model.rt, model.batch_size * C, 'explain_%d' % C)
        ex = ExplainSlate(model.rt, latent, pool, ids, top)
        sl = SlateScore(model.rt, latent, pool, ids, None)
        ex.own_nodes = (ids, ex, sl)
        entry = model._plans[key] = G.Plan(model.rt, [ex, sl], False, [])
    ex, sl = entry.fetch
    feed()
    ex.inputs[2].feed(cand.reshape(-1))
    entry.run()
    tok = (None, None, None) if not top else (ex.token_value.clone(), ex.token_id.clone(), ex.token_feature.clone())
    return Explanation(sl.value.clone(), ex.value.clone(), ex.bias.clone(), tok[0], tok[1], tok[2], ex.features)
