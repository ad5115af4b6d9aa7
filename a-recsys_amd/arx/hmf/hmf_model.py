"""LatentProductModel -- the reference's HMF model (hmf/hmf_model.py:19-274) on MI355X.

Constructor / step / get_batch / get_permuted_batch keep the reference's
signatures; `session`, `GPU`, `run_op`, `run_meta` are accepted and ignored.
State (tables, Adagrad slots, mask, sampled pool) lives on the device and is
owned by the model.  step() is forward + backward + Adagrad as ONE captured
hipGraph replay of libarx.so kernels.
"""
from __future__ import annotations

import random

import numpy as np
import torch

from .. import explain
from .. import graph as G
from .. import ops
from .. import slate
from .. import topk as _topk
from ..attributes import embed_attribute
from ..topk import (StreamTopK, TopK, TopKScan, check_return_logprob, check_scan_dtype,       # noqa: F401
                    excluding_twin, recommend_key, recommend_node, run_complete)                   # (re-exported)
from ..utils.checkpoint import Saver


class _Var(object):
    """Stand-in for the tf.Variable handles the runners read with .eval()."""

    def __init__(self, getter):
        self._getter = getter

    def eval(self, session=None):
        return self._getter()


class _Op(object):
    def __init__(self, fn):
        self._fn = fn

    def run(self, session=None):
        return self._fn()

    __call__ = run


class MLP(G.Node):
    """hmf_model.py:80-94: drop(act(drop(act(drop(act(u)) . W1 + b1)) . W2 + b2)) -- tf.nn.dropout
    after every activation with the model's keep probability (identity in forward-only plans
    and when rt.keep_prob == 1).  The three keep masks stay readable in `keeps` (parity tests
    replay them through the oracle)."""

    requires_grad = True
    uses_dropout = True

    def __init__(self, rt, x, params, kind):
        self.w1, self.b1, self.w2, self.b2 = params
        super().__init__(rt, (x.shape[0], self.w2.w.shape[1]), (x,))
        self.kind = 0 if kind == 'relu' else 1
        n, hdim = x.shape[0], self.w1.w.shape[1]
        dev = rt.device
        f32 = torch.float32
        self.h0 = torch.empty(x.shape, dtype=f32, device=dev)          # act(u)
        self.h1 = torch.empty((n, hdim), dtype=f32, device=dev)        # act(z1)
        self.h2 = torch.empty(self.shape, dtype=f32, device=dev)       # act(z2)
        self.h0d, self.h1d = torch.empty_like(self.h0), torch.empty_like(self.h1)   # after dropout
        self.d1 = torch.empty((n, hdim), dtype=f32, device=dev)
        self.d0 = torch.empty(x.shape, dtype=f32, device=dev)
        self.keeps = [torch.empty(t.numel(), dtype=torch.uint8, device=dev) for t in (self.h0, self.h1, self.h2)]
        self.sids = []
        for _ in range(3):
            rt.dropout_calls += 1
            self.sids.append(rt.dropout_calls)
        self.kp_used = 1.0

    def _drop(self, k, src, dst, kp):
        ops.dropout_fwd_step(src, kp, self.rt.seed * 1000003 + self.sids[k], self.rt.step_dev, dst, self.keeps[k])

    def forward(self, train):
        x = self.inputs[0]
        rt = self.rt
        out = self.alloc_value()
        kp = rt.keep_prob if train else 1.0
        self.kp_used = kp
        drop = kp < 1.0
        ops.act_fwd(x.value, self.kind, self.h0)
        a0 = self.h0
        if drop:
            self._drop(0, self.h0, self.h0d, kp)
            a0 = self.h0d
        ops.gemm(a0, self.w1.w, self.h1, rt.ws, col_bias=self.b1.w)
        ops.act_fwd(self.h1, self.kind, self.h1)
        a1 = self.h1
        if drop:
            self._drop(1, self.h1, self.h1d, kp)
            a1 = self.h1d
        h2 = self.h2 if drop else out
        ops.gemm(a1, self.w2.w, h2, rt.ws, col_bias=self.b2.w)
        ops.act_fwd(h2, self.kind, h2)
        if drop:
            self._drop(2, self.h2, out, kp)

    def backward(self):
        x = self.inputs[0]
        rt = self.rt
        kp = self.kp_used
        drop = kp < 1.0
        dz2 = self.grad
        if drop:
            ops.dropout_bwd(dz2, self.keeps[2], kp, dz2)
        ops.act_bwd(self.h2 if drop else self.value, dz2, self.kind, dz2)      # through act(z2)
        a1 = self.h1d if drop else self.h1
        a0 = self.h0d if drop else self.h0
        ops.gemm(a1, dz2, self.w2.grad, rt.ws, transA=True)
        ops.col_sum(dz2, self.b2.grad, rt.ws)
        ops.gemm(dz2, self.w2.w, self.d1, rt.ws, transB=True)
        if drop:
            ops.dropout_bwd(self.d1, self.keeps[1], kp, self.d1)
        ops.act_bwd(self.h1, self.d1, self.kind, self.d1)
        ops.gemm(a0, self.d1, self.w1.grad, rt.ws, transA=True)
        ops.col_sum(self.d1, self.b1.grad, rt.ws)
        ops.gemm(self.d1, self.w1.w, self.d0, rt.ws, transB=True)
        if drop:
            ops.dropout_bwd(self.d0, self.keeps[0], kp, self.d0)
        ops.act_bwd(self.h0, self.d0, self.kind, self.d0)
        g = x.alloc_grad()
        ops.add_rows_bcast(1.0, self.d0, x.grad_beta(), g)
        for p in (self.w1, self.b1, self.w2, self.b2):
            p.touched = True


class LatentProductModel(object):
    def __init__(self, user_size, item_size, size, num_layers, batch_size, learning_rate,
                 learning_rate_decay_factor, user_attributes=None, item_attributes=None,
                 item_ind2logit_ind=None, logit_ind2item_ind=None, loss_function='ce', GPU=None,
                 logit_size_test=None, nonlinear=None, dropout=1.0, n_sampled=None,
                 indices_item=None, dtype='float32', top_N_items=100, hidden_size=500,
                 loss_func='log', loss_exp_p=1.005, params=None, use_graph=True, seed=0,
                 mw_eval_unmasked=True):
        self.user_size = user_size
        self.item_size = item_size
        self.top_N_items = top_N_items
        # 'mw' models evaluate with the full-vocabulary 'warp' loss (:130,144).  The reference's
        # step() only runs set_mask['mw'] (:209-210), so ITS eval loss sees an all-True warp mask
        # (the target column itself adds relu(0 + 1) = 1 inside the log).  That is the default
        # (run_hmf.py selects checkpoints, patience and learning-rate decay on this number);
        # mw_eval_unmasked=False masks the user's eval positives instead (what the masks are for).
        self.mw_eval_unmasked = bool(mw_eval_unmasked)
        if user_attributes is not None:
            user_attributes.set_model_size(size)             # hmf_model.py:34-36
            self.user_attributes = user_attributes
        if item_attributes is not None:
            item_attributes.set_model_size(size)
            self.item_attributes = item_attributes
        self.item_ind2logit_ind = item_ind2logit_ind
        self.logit_ind2item_ind = logit_ind2item_ind
        if logit_ind2item_ind is not None:
            self.logit_size = len(logit_ind2item_ind)
        self.indices_item = indices_item if indices_item is not None else range(self.logit_size)
        self.logit_size_test = logit_size_test
        self.nonlinear = nonlinear
        self.loss_function = loss_function
        self.n_sampled = n_sampled
        self.batch_size = batch_size
        self.dropout = dropout
        self.dtype = dtype
        self.data_length = None
        self.train_permutation = None
        self.start_index = None
        self.loss_func, self.loss_exp_p = loss_func, loss_exp_p

        self.rt = rt = G.Runtime(learning_rate=learning_rate, use_graph=use_graph)
        self._lr_decay = learning_rate_decay_factor
        self.learning_rate = _Var(lambda: rt.lr_host)
        self.learning_rate_decay_op = _Op(lambda: rt.set_learning_rate(rt.lr_host * self._lr_decay))
        self.global_step = _Var(lambda: rt.global_step)

        mb = batch_size
        # mapped item target (logit index) and raw item id target (hmf_model.py:69-70)
        self.item_id_target = G.IdsInput(rt, mb, 'item_id')
        self.item_target = None      # built below: the in-plan mapping of item_id_target (needs att_emb)

        m = embed_attribute.EmbeddingAttribute(user_attributes, item_attributes, mb, self.n_sampled,
                                               0, False, item_ind2logit_ind, logit_ind2item_ind,
                                               params=params, runtime=rt, seed=seed)
        self.att_emb = m
        self.item_target = embed_attribute.TargetMapping(rt, self.item_id_target, m, 'item')    # :69,173
        embedded_user, _ = m.get_batch_user(float(dropout), False)          # :78
        if self.nonlinear in ('relu', 'tanh'):
            ps = []
            for name, shape in (('w1', (size, hidden_size)), ('b1', (hidden_size,)),
                                ('w2', (hidden_size, size)), ('b2', (size,))):
                w = m._new_var(name, shape, params or {})
                p = G.DenseParam(name, w)
                rt.dense[name] = p
                ps.append(p)
            embedded_user, _ = m.get_batch_user(1.0, False)                  # :87
            rt.keep_prob = float(dropout)                                    # :88-94 dropout inside the MLP
            embedded_user = MLP(rt, embedded_user, ps, self.nonlinear)
        self.embedded_user = embedded_user

        loss = self.loss_function
        self._plans = {}
        self.set_mask, self.reset_mask = {}, {}
        self.pos_score = self.neg_score = self.auc = None
        neg_pos = None
        if loss in ('bpr', 'bpr-hinge'):
            # :96-107.  Built for the pair losses only: no other loss reads the 'pos' / 'neg' placeholders, and the
            # reference never fed them (embed_attribute.py:704-706 is commented out there)
            pos_embs_item, _pos_item_b = m.get_batch_item('pos', mb)
            neg_embs_item, _neg_item_b = m.get_batch_item('neg', mb)
            neg_pos = embed_attribute.NegPos(embedded_user, embed_attribute.reduce_mean(pos_embs_item, 0),
                                             embed_attribute.reduce_mean(neg_embs_item, 0))
        sampled_logits = target_score = None
        if self.n_sampled is not None:
            sampled_logits = m.get_prediction(embedded_user, 'sampled')       # :112
            target_score = m.get_target_score(embedded_user, self.item_id_target)  # :115
        logits = m.get_prediction(embedded_user)                              # :118
        self.output = logits
        batch_loss_eval = None
        if loss in ('warp', 'ce', 'rs', 'rs-sig', 'rs-sig2', 'bbpr'):            # :121-122
            batch_loss = m.compute_loss(logits, self.item_target, loss, loss_func=self.loss_func,
                                        exp_p=self.loss_exp_p)
        elif loss == 'warp_eval':
            batch_loss, _ = m.compute_loss(logits, self.item_target, loss)
        elif loss in ('mw', 'mce'):
            # 'mce': build-defined sampled softmax (the reference has no arithmetic for it, see arx.h): trains like
            # 'mw' on the sampled pool; evaluates with the full softmax 'ce', the loss run_hmf.py:255,304 groups it with
            batch_loss = m.compute_loss(sampled_logits, target_score, loss)
            batch_loss_eval = m.sampled_eval_loss(loss, embedded_user, logits, self.item_target, batch_size,  # :130
                                                  batch_size, m._pool_embed('full', 1),
                                                  masked=not self.mw_eval_unmasked)
        elif loss in ('bpr', 'bpr-hinge'):                                       # :132-133
            # one launch forms both scores, the loss and every gradient; no [mb, V] logits in training
            batch_loss = m.compute_loss(neg_pos, self.item_target, loss)
            self.pos_score = G.PairOutput(rt, batch_loss, 'pos')                 # :104
            self.neg_score = G.PairOutput(rt, batch_loss, 'neg')                 # :105
            self.auc = G.PairOutput(rt, batch_loss, 'auc')                       # :107
        else:
            raise NotImplementedError("not implemented!")
        if loss in ('warp', 'warp_eval', 'mw', 'mce', 'rs', 'rs-sig', 'rs-sig2', 'bbpr'):   # :137
            self.set_mask, self.reset_mask = m.get_warp_mask()
        self.batch_loss = batch_loss
        self.loss = G.MeanLoss(rt, batch_loss)                                # :140
        self.loss.lazy = True
        self.loss_eval = G.MeanLoss(rt, batch_loss_eval) if loss in ('mw', 'mce') else self.loss  # :144
        self.topk = recommend_node(rt, logits, min(self.top_N_items, self.logit_size), batch_size)
        self.indices = self.topk
        self.saver = Saver(self)

    # ------------------------------------------------------------------
    def prepare_warp(self, pos_item_set, pos_item_set_eval):
        self.att_emb.prepare_warp(pos_item_set, pos_item_set_eval)

    def prepare_recommend_exclusions(self, item_sets):
        """The items recommend(exclude_seen=True) leaves out per user -- typically the training history:
        {user_index: items} or a (ptr, items) CSR pair in item-index space (EmbeddingAttribute.
        prepare_recommend_exclusions).  A second call replaces the lists (the captured plan is dropped)."""
        for key in ('recommend_ex', 'recommend_ex_sample', 'recommend_ex_tags_sample', 'recommend_ex_sample_logp',
                    'recommend_ex_tags_sample_logp', 'recommend_ex_bf16', 'recommend_ex_tags_bf16'):
            self._plans.pop(key, None)
        _topk.drop_list_logp_plans(self, '_ex')
        self.att_emb.prepare_recommend_exclusions(item_sets)

    def prepare_item_tags(self, tags):
        """The items' 32-bit tag words for recommend(tags_any=, tags_all=): an integer array [n_items] or
        {item_index: bit numbers 0..31} (EmbeddingAttribute.prepare_item_tags).  A second call replaces the words
        (the captured plans that read them are dropped)."""
        for key in ('recommend_tags', 'recommend_ex_tags', 'recommend_tags_sample', 'recommend_ex_tags_sample',
                    'recommend_tags_sample_logp', 'recommend_ex_tags_sample_logp', 'recommend_tags_bf16',
                    'recommend_ex_tags_bf16'):
            self._plans.pop(key, None)
        _topk.drop_list_logp_plans(self, '_tags')
        self.att_emb.prepare_item_tags(tags)

    def _scan_bf16(self, scan_dtype, recommend, sample_temperature, return_logprob):
        """topk.check_scan_dtype; True only where the recommend node streams (a dense top-k has no scan to speed up)."""
        return check_scan_dtype(scan_dtype, recommend, sample_temperature, return_logprob) and \
            isinstance(self.topk, StreamTopK)

    def _recommend_node(self, key):
        if key.endswith('_bf16'):
            return getattr(self, '_bf16_nodes', {}).get(key)
        if key.endswith('_sample') or key.endswith('_sample_logp'):
            return getattr(self, '_sample_nodes', {}).get(key)
        return {'recommend': self.topk, 'recommend_ex': getattr(self, 'topk_ex', None),
                'recommend_tags': getattr(self, 'topk_tags', None),
                'recommend_ex_tags': getattr(self, 'topk_ex_tags', None)}[key]

    def similar_items(self, logit_ids, k, include_self=False, return_values=False, chunk=65536,
                      return_logprob=False, scan_dtype=None):
        """Cosine nearest neighbours of items (logit indices) over the full vocabulary, in the item latent space
        recommend scores against: EmbeddingAttribute.similar_items."""
        return self.att_emb.similar_items(logit_ids, k, include_self=include_self, return_values=return_values,
                                          return_logprob=return_logprob, scan_dtype=scan_dtype,
                                          chunk=chunk)

    def prepare_item_groups(self, groups):
        """The items' groups (category / brand / seller) for score_items(max_per_group=): an integer array [n_items] or
        {item_index: group} in item-index space, a negative id for 'no group'.  Mapped through item_ind2logit_ind to
        one int32 per logit column, -1 for a column without an item (arx.slate.item_group_ids).  A second call
        replaces the array (the capped plans are dropped)."""
        slate.prepare_item_groups(self, groups)

    def score_items(self, user_input, candidates, k=None, diversify=None, max_per_group=None, sample_temperature=None,
                    sample_seed=None, return_logprob=False):
        """What the model thinks of THESE items for THIS user: row r of one full batch of users (the rules of
        step(recommend=True)) against its own slate candidates[r] -- [batch_size, C] logit indices, the space
        recommend returns and similar_items takes; -1 marks an empty slot.  The latent and the item pool are
        recommend's, dropout off.  k None: float32 [mb, C] scores on the device, -inf at empty slots.
        1 <= k <= min(1024, C): (ids int32 [mb, k], values float32 [mb, k]) by (score desc, slot asc) -- duplicates
        and ties keep slate order --, (-1, -inf) where a row has fewer than k live slots (an item switched off by a
        -inf bias is not live, as in recommend).  ValueError for any other k or a malformed slate.  Build-defined
        (arx.slate): one plan per (C, k), at most eight kept.
        diversify = lambda in [0, 1] (a scalar or one per row): "the best k, but spread out" -- a greedy MMR re-rank on
        the device (arx_diverse.h).  Pick t maximises lambda * rel - (1 - lambda) * (largest cosine between the item's
        latent and those of picks 0 .. t - 1), rel the score scaled to [0, 1] over the row's live slots; ties go to
        the higher score, then the lower slot.  max_per_group = m >= 1 (a scalar or one per row): at most m picks of
        one group, after prepare_item_groups(); alone it means lambda = 1, the best k by score under the cap.  With
        either, k is required and (ids, values) -- values the model's scores -- come in SELECTION order, (-1, -inf)
        once no slot qualifies.  ValueError for a lambda outside [0, 1], a cap below 1 or without groups, and a (C, d)
        outside arx_slate_mmr_supported (C <= 512, d <= 128, C * d <= 32768).  The usual composition: over-fetch with a
        model built with top_N_items = C, then re-rank to k (the -1 tails of recommend are empty slots already):
            cands = model.step(None, users, None, recommend=True)
            ids, values = model.score_items(users, cands, k, diversify=0.7)
        sample_temperature = tau (a number >= 0 or one per row; None: the calls above, untouched): "explore among the
        best C, and log how likely the draw was" -- k is required and (ids, values) are k DISTINCT items drawn with
        probability proportional to exp(score / tau), one after the other without replacement (Plackett-Luce), in
        SELECTION order; values are the model's scores, not monotone along a row.  An item that fills several slots
        competes once (its lowest slot), -1 and -inf slots never; tau = 0 rows are the plain order; (-1, -inf) past the
        last distinct live item.  The noise is the sampled recommend's, a function of (seed, row, item): the draw is
        that call's draw restricted to the slate and does not depend on the slate's order.  sample_seed: an int in
        [0, 2^63) -- the same seed gives the same draw; None takes the model's draw counter (att_emb.sample_draws, shared
        with recommend: starts at 0, one up per such call).  return_logprob=True: (ids, values, logprob), logprob
        float32 [mb, k] the log-probability of each draw given the draws before it (arx_slate_sample.h) -- the row sum
        is the log-propensity of the returned list; 0 on a tau = 0 row and in the (-1, -inf) columns.  ValueError for
        a temperature without k or together with diversify / max_per_group, a seed or return_logprob without a
        temperature, a bad temperature or seed (topk.sample_params) and a C outside arx_slate_sample_supported
        (C <= 1024).  One more plan per (C, k); the temperature and the seed are fed per call:
            cands = model.step(None, users, None, recommend=True)
            ids, values, logp = model.score_items(users, cands, k, sample_temperature=0.5, sample_seed=s,
                                                  return_logprob=True)"""
        return slate.score_items(self, lambda: self._feed(user_input, None, True, self.loss_function, None, None, True),
                                 candidates, k, diversify, max_per_group, sample_temperature, sample_seed,
                                 return_logprob)

    def explain_items(self, user_input, items, top=3):
        """WHY did these items get these scores for these users: the score score_items gives row r of one full batch
        of users (the rules of step(recommend=True), dropout off) for each item of its slate items[r] -- [batch_size,
        C] logit indices, -1 an empty slot -- taken apart on the device (arx_explain.h).  The score is an exact sum
        over the item's F output features of 1/F * (u . id row + bias) or 1/F * the bag mean of (u . token row +
        bias); returns arx.explain.Explanation(score, feature, bias, token_value, token_id, token_feature, features):
        score [mb, C] has score_items' bits; feature [mb, C, F] the part of each output feature (was it the item's
        own id row or its genre?), summing to the score up to float32 rounding; bias [mb, C] the part that does not
        depend on the user; token_* [mb, C, top] the `top` largest single-token contributions over all bags of the
        item (these three words of its title), by (value desc, feature asc, bag position asc), (-inf, -1, -1) past
        the last position, None with top = 0; features names the columns as (kind, table_name).  Every bag position
        is an entry of its own: a repeated token appears once per position.  ValueError for a malformed slate or a
        top that is not an int in [0, 16]; output_feat 2 / 3: NotImplementedError.  One plan per (C, top), at most
        four kept.  Not offered: SeqModel, the sharded models (their tables are striped), a "most negative" or
        absolute-value order, merged repeats.
            ex = model.explain_items(users, cands, top=3)
            ex.feature[r, j]          # one number per output feature of item cands[r, j]"""
        return explain.explain_items(self, lambda: self._feed(user_input, None, True, self.loss_function, None, None,
                                                              True), items, top)

    def list_logprob(self, user_input, lists, sample_temperature, exclude_seen=False, tags_any=None, tags_all=None,
                     return_values=False, return_why=False):
        """How likely would THIS model have been to show THESE items in THIS order: the log-probability of a given
        ordered list under the policy of step(recommend=True, sample_temperature=) -- the numerator of an importance
        weight whose denominator return_logprob=True logged at serving time (arx_list_logp.h).  One full batch of
        users (the rules of step(recommend=True), dropout off); lists [batch_size, k]: logit indices, the space
        recommend returns -- a list, a numpy array or a device tensor; k is read from the shape, 1 <= k <= 1024, not
        tied to top_N_items; -1 is an empty slot.  sample_temperature: a number > 0 or one per row.  exclude_seen /
        tags_any / tags_all: the filters of the policy, as in step().  Returns float32 [mb, k] numpy: logprob[r][t]
        is the log-probability of entry t given the DRAWABLE entries before it; 0 at a -1; -inf at an entry the
        policy could never draw (out of range, excluded, outside the tags, a repeat of an earlier entry, a score of
        -inf) -- such an entry is ABSENT for the others, and the row sum, the log-probability of the whole ordered
        list, is -inf.  A list this policy drew itself gives back the bits return_logprob=True reported with it.
        return_values / return_why: the tuple (logprob[, values][, why]) -- values float32 the model's scores of the
        drawable entries (-inf elsewhere), why int32 the reason codes 0 OK, 1 EMPTY, 2 RANGE, 3 EXCLUDED, 4 TAGS,
        5 REPEAT, 6 NOSCORE.  Nothing is drawn: there is no seed.  ValueError, before any feed: k outside [1, 1024],
        a wrong row count, a temperature that is not finite and > 0 (0: a deterministic policy has no propensities --
        compare the list with recommend()), exclude_seen / tags without their prepare_*; NotImplementedError for
        output_feat 2 / 3.  One plan per (filters, k); the temperatures, tag words and lists are fed per call:
            ids, logged = old.step(None, users, None, recommend=True, sample_temperature=0.7, return_logprob=True)
            target = new.list_logprob(users, ids, 0.7)
            w = arx.utils.ope.list_weights(target, logged); value = arx.utils.ope.snips(rewards, w)"""
        return _topk.list_logprob(self, lambda: self._feed(user_input, None, True, self.loss_function, None, None,
                                                           True),
                                  lists, sample_temperature, exclude_seen, tags_any, tags_all, return_values,
                                  return_why)

    def prepare_pair_negatives(self, hist, seed=0, power=None, smooth=1.0, counts=None, hardest_of=None):
        """'bpr' / 'bpr-hinge': the items a DRAWN negative must not hit, per user -- typically the training history:
        {user_index: items} or a (ptr, items) CSR pair in item-index space.  After this call a step without
        neg_item_input draws one negative per row on the device: uniform over the user's other items (power None),
        or in proportion to (counts + smooth) ** power -- counts per item index, by default the number of users
        whose list holds the item; 0.75 is the usual unigram rule (EmbeddingAttribute.prepare_pair_negatives).
        hardest_of = C, an int in [2, 64]: dynamic negative sampling -- a training step draws C candidates by that
        rule, scores them with the current tables and trains against the one the model ranks highest, inside the
        same captured step (EmbeddingAttribute.prepare_pair_negatives, arx_neg_draw_hardest); forward_only steps keep
        the plain single draw.  With dropout < 1 the candidate scores use the UNDROPPED user row.  ValueError for any
        other hardest_of; NotImplementedError, naming what is unsupported, for nonlinear 'relu' / 'tanh' (the latent is
        not a table row) and for users or items that are not exactly one one-hot feature -- all raised before anything
        is uploaded or dropped, so an earlier prepare stays in force.
        A second call replaces the lists, the weights, the seed and the hard mode (the drawing plans are dropped)."""
        if self.loss_function not in ('bpr', 'bpr-hinge'):
            raise ValueError("prepare_pair_negatives: a model of the 'bpr' / 'bpr-hinge' losses")
        self.att_emb.check_hardest_of(hardest_of)
        if hardest_of is not None and self.nonlinear in ('relu', 'tanh'):
            raise NotImplementedError("prepare_pair_negatives(hardest_of=): nonlinear=%r -- the user latent is an MLP "
                                      "output, not a table row the candidates could be scored against"
                                      % (self.nonlinear,))
        for key in ('train_draw', 'eval_draw'):
            self._plans.pop(key, None)
        self.att_emb.prepare_pair_negatives(hist, seed=seed, power=power, smooth=smooth, counts=counts,
                                            hardest_of=hardest_of)

    def _plan(self, key):
        if key in self._plans:
            return self._plans[key]
        rt, m = self.rt, self.att_emb
        loss = self.loss_function
        if key == 'train':
            masks = [m.mask[loss]] if loss in m.mask else []
            p = G.Plan(rt, [self.loss], True, masks)
        elif key == 'eval':
            p = G.Plan(rt, [self.loss_eval], False, m.eval_masks(loss, self.loss_eval.inputs[0]))
        elif key == 'train_draw':              # pair losses, the negatives drawn in the plan (NegPairDraw goes first)
            p = G.Plan(rt, [m.neg_draw, self.loss], True, [])
        elif key == 'eval_draw':
            p = G.Plan(rt, [m.neg_draw, self.loss_eval], False, [])
        elif key == 'recommend':
            p = G.Plan(rt, [self.topk], False, [])
        elif key == 'recommend_ex':
            m.exclusion_args()                 # (raises before anything is built when no lists were prepared)
            if getattr(self, 'topk_ex', None) is None:
                self.topk_ex = excluding_twin(rt, self.topk, m.exclusion_args)
            p = G.Plan(rt, [self.topk_ex], False, [])
        elif key == 'recommend_tags':
            m.tag_args()                       # (raises before anything is built when no tags were prepared)
            if getattr(self, 'topk_tags', None) is None:
                self.topk_tags = excluding_twin(rt, self.topk, tag_args=m.tag_args)
            p = G.Plan(rt, [self.topk_tags], False, [])
        elif key == 'recommend_ex_tags':
            m.exclusion_args()
            m.tag_args()
            if getattr(self, 'topk_ex_tags', None) is None:
                self.topk_ex_tags = excluding_twin(rt, self.topk, m.exclusion_args, m.tag_args)
            p = G.Plan(rt, [self.topk_ex_tags], False, [])
        elif key == 'warp_eval':
            p = G.Plan(rt, [self.batch_loss], False, [m.mask['warp_eval']])
        elif key.startswith('recommend') and key.endswith('_bf16'):
            # the twins whose fused scan filters in bf16 (topk.recommend_key; scan_dtype='bf16'): the same filters, a
            # node and a plan of their own beside the f32 ones
            ex, tg = '_ex' in key, '_tags' in key
            if ex:
                m.exclusion_args()
            if tg:
                m.tag_args()
            nodes = self.__dict__.setdefault('_bf16_nodes', {})
            if key not in nodes:
                nodes[key] = excluding_twin(rt, self.topk, m.exclusion_args if ex else None,
                                            m.tag_args if tg else None, scan_bf16=True)
            p = G.Plan(rt, [nodes[key]], False, [])
        elif key.startswith('recommend') and (key.endswith('_sample') or key.endswith('_sample_logp')):
            # the sampled twins (topk.recommend_key): the same filters, the keys of m.sample_args; '_logp': the twin
            # that also runs the mass pass (node.logp: the log-probability of every draw)
            ex, tg = '_ex' in key, '_tags' in key
            if ex:
                m.exclusion_args()
            if tg:
                m.tag_args()
            nodes = self.__dict__.setdefault('_sample_nodes', {})
            if key not in nodes:
                nodes[key] = excluding_twin(rt, self.topk, m.exclusion_args if ex else None,
                                            m.tag_args if tg else None, sample_args=m.sample_args,
                                            logp=key.endswith('_logp'))
            p = G.Plan(rt, [nodes[key]], False, [])
        else:
            raise KeyError(key)
        self._plans[key] = p
        return p

    def _feed(self, user_input, item_input, recommend, loss, item_sampled, item_sampled_id2idx,
              forward_only, neg_item_input=None):
        m = self.att_emb
        if not recommend:
            if not isinstance(item_input, torch.Tensor) and (self.loss_function not in ('mw', 'mce') or forward_only):
                # host ids: mapped here so that an item without a logit fails like the reference's
                # dict lookup (:173); the plan maps item_id_target again on device (same values)
                self.item_target.feed(m.target_mapping([item_input])[0])
            self.item_id_target.feed(item_input)                              # :176
        update_sampled, _, _ = m.add_input({}, user_input, item_input, neg_item_input=neg_item_input,
                                           item_sampled=item_sampled,
                                           item_sampled_id2idx=item_sampled_id2idx,
                                           forward_only=forward_only, recommend=recommend, loss=loss)
        for op in update_sampled:                                             # :206-207
            op()

    def prepare_next(self, user_input, item_input, item_sampled=None):
        """Announce the batch of the NEXT training step before calling step() for the current one (the host loop
        draws batches before it trains on them: hmf/run_hmf.py:234-242, so a loader can hand step t + 1's ids over
        one step early).  The half of the sparse update that needs the ids only -- contribution keys, their sort,
        the run records (K7, hmf_model.py:146-151) -- then runs for step t + 1 as a side branch of step t's graph,
        off the critical path.  item_sampled: the pool step t + 1 will be given, if it is a new one.  Optional:
        step() without it (or with other ids than announced) computes the same numbers, bit for bit."""
        # (advisor, round 4) identity alone does not see a loader that refills the announced buffers in place: torch
        # tensors are remembered with their version counters, anything else (numpy arrays, lists) is COPIED here
        self._next_batch = tuple(self._announce(x) for x in (user_input, item_input, item_sampled))

    @staticmethod
    def _announce(x):
        import torch
        if x is None or isinstance(x, torch.Tensor):
            return x
        return np.array(x, dtype=np.int32, copy=True)

    @staticmethod
    def _versions(t):
        import torch
        return tuple((x._version if isinstance(x, torch.Tensor) else None) for x in t)

    def _ring_feed(self, plan, item_sampled):
        """step t: queue the announced ids of step t + 1 into the next-step placeholders; True if the plan may run
        in ring mode."""
        nxt, self._next_batch = getattr(self, '_next_batch', None), None
        ann, self._announced = getattr(self, '_announced', None), None
        if nxt is None or not plan.ring_capable():
            return False
        m = self.att_emb
        nodes = {id(m.u_indices['input']): nxt[0], id(self.item_id_target): nxt[1]}
        pool = m.i_indices.get('sampled_pass') if hasattr(m.i_indices, 'get') else None
        known = set(nodes) | ({id(pool)} if pool is not None else set())
        if any(id(n) not in known for n in plan.ring_ids()):
            return False                      # a lookup this method does not know how to announce
        # what step t - 1 sorted ahead is only valid for the ids it was told (tensor identity; a pool given now
        # must be the one announced)
        same = lambda a, b: a is b or (isinstance(a, np.ndarray) and not hasattr(b, '_version')
                                       and np.array_equal(a, np.asarray(b)))
        if ann is None or not same(ann[0], self._cur[0]) or not same(ann[1], self._cur[1]) or \
                (item_sampled is not None and not same(ann[2], item_sampled)) or \
                self._versions(ann) != getattr(self, '_announced_versions', None):
            plan._ring_ready = False        # other ids than announced (or announced buffers refilled since): sort now
        if not plan._ring_ready:
            plan.ring_bootstrap()
        for n in plan.ring_ids():
            if id(n) in nodes:
                n.feed_next(nodes[id(n)])
            elif nxt[2] is not None:
                n.feed_next(nxt[2])
            else:
                n.feed_next(item_sampled if item_sampled is not None else n.value)   # same pool as this step
        self._announced = nxt
        self._announced_versions = self._versions(nxt)
        plan.ring_req = True
        return True

    def step_async(self, session, user_input, item_input, neg_item_input=None, item_sampled=None,
                   item_sampled_id2idx=None, forward_only=False, recommend=False,
                   recommend_new=False, loss=None, run_op=None, run_meta=None, exclude_seen=False,
                   tags_any=None, tags_all=None, sample_temperature=None, sample_seed=None, return_logprob=False,
                   scan_dtype=None):
        """step() without the device->host read of the result: returns the MeanLoss
        node (call .read() for the device scalar) / the top-k index tensor.  recommend with the streaming top-k
        (StreamTopK, fused form): the result is complete only if `self.topk.overflowed()` is False afterwards
        (one device -> host read; step() checks it and re-runs the request on the chunked path).
        exclude_seen (with recommend): leave out each user's items of prepare_recommend_exclusions -- node
        self.topk_ex, plan 'recommend_ex'; a user with fewer than top_N eligible items gets -1 tails.
        tags_any / tags_all (with recommend; an int or one int per row): only the items eligible by their tag words
        of prepare_item_tags -- plans 'recommend_tags' / 'recommend_ex_tags'; both None: the calls above.
        sample_temperature / sample_seed (with recommend): the sampled recommend of step() -- the plans ending in
        '_sample'; None: the calls above.  return_logprob (with sample_temperature): the plans ending in
        '_sample_logp' -- returns (indices, logprob), the two device tensors [mb, top_N].
        scan_dtype='bf16' (with recommend): the plans ending in '_bf16' (step() states the rules)."""
        if loss is None:
            loss = self.loss_function
        check_return_logprob(return_logprob, recommend, sample_temperature)
        bf16 = self._scan_bf16(scan_dtype, recommend, sample_temperature, return_logprob)
        if exclude_seen and recommend:
            self.att_emb.exclusion_args()      # ValueError before any feed when nothing was prepared
        tagged = recommend and (tags_any is not None or tags_all is not None)
        if tagged:
            self.att_emb.feed_tag_words(tags_any, tags_all)       # ValueError before any other feed
        sampled = recommend and sample_temperature is not None
        if sampled:
            self.att_emb.feed_sample(sample_temperature, sample_seed)
        # pair losses: a step without negatives draws them inside its plan (prepare_pair_negatives)
        pair = self.loss_function in ('bpr', 'bpr-hinge') and not recommend
        draw = pair and (neg_item_input is None or len(neg_item_input) == 0)
        if draw and getattr(self.att_emb, 'neg_draw', None) is None:
            raise ValueError("a '%s' step needs neg_item_input, or prepare_pair_negatives() to draw the negatives "
                             "on the device" % self.loss_function)
        self._cur = (user_input, item_input)
        self._feed(user_input, item_input, recommend, loss, item_sampled, item_sampled_id2idx,
                   forward_only, neg_item_input=None if draw else neg_item_input)
        if pair:
            if draw:
                self.rt.drop_feed(self.att_emb.i_indices['neg'].value)    # (a queued older feed must not overwrite the draw)
            self.batch_loss.draw = self.att_emb.neg_draw if draw else None
        if tagged or sampled or bf16:
            key = recommend_key(exclude_seen, tagged, sampled, bool(return_logprob), bf16)
            self._plan(key).run()
            node = self._recommend_node(key)
            return (node.indices, node.logp) if return_logprob else node.indices
        if recommend and exclude_seen:
            self._plan('recommend_ex').run()
            return self.topk_ex.indices
        if recommend:
            self._plan('recommend').run()
            return self.topk.indices
        if loss == 'warp_eval':
            self._plan('warp_eval').run()
            return [self.batch_loss.value, self.batch_loss.rank_value]
        if forward_only:
            self._plan('eval_draw' if draw else 'eval').run()
            return self.loss_eval
        plan = self._plan('train_draw' if draw else 'train')
        if getattr(self, '_next_batch', None) is not None:
            self._ring_feed(plan, item_sampled)
        else:
            self._announced = None
        plan.run()
        self.rt.global_step += 1
        return self.loss

    def step(self, session, user_input, item_input, neg_item_input=None, item_sampled=None,
             item_sampled_id2idx=None, forward_only=False, recommend=False, recommend_new=False,
             loss=None, run_op=None, run_meta=None, exclude_seen=False, tags_any=None, tags_all=None,
             sample_temperature=None, sample_seed=None, return_logprob=False, scan_dtype=None):
        """hmf_model.py:162-228.  Returns: train -> mean loss (float); forward_only ->
        loss_eval (float); recommend -> int32 [mb, top_N]; warp_eval -> [loss, rank].
        'bpr' / 'bpr-hinge': neg_item_input (list, array or device tensor) holds one negative item per row; None or
        empty draws them on the device (prepare_pair_negatives first, else ValueError).  self.pos_score /
        neg_score / auc .read() give the last step's scores (hmf_model.py:104-107).
        recommend with exclude_seen=True: the top_N logit indices without each user's items of
        prepare_recommend_exclusions (ValueError if none were prepared); -1 where a user has fewer eligible items.
        recommend with tags_any / tags_all (an int: one 32-bit word for every row, or one int per row): only the items
        whose tag word of prepare_item_tags has a bit of `any` (0: no constraint) and every bit of `all`; composes
        with exclude_seen.  ValueError without prepare_item_tags, for words outside [0, 2^32) or a wrong length.
        recommend with sample_temperature (a number >= 0 or one per row; None: the deterministic call, untouched): top_N
        DISTINCT items drawn with probability proportional to exp(score / temperature), one after the other without
        replacement, returned in SELECTION order (the first id is the first draw); a row of temperature 0 is its plain
        top-k.  sample_seed: an int in [0, 2^63) -- the same seed gives the same items, on every path; None takes the
        model's draw counter (att_emb.sample_draws: starts at 0, one up per such call).  Composes with exclude_seen
        and the tags.
        return_logprob=True (with sample_temperature): returns (ids int32 [mb, top_N], logprob float32 [mb, top_N]) --
        logprob[r][t] is the log-probability of draw t given the draws before it under THIS policy, softmax(score /
        temperature) over the row's whole eligible vocabulary (arx_sample_logp.h); the row sum is the log-propensity
        of the ordered list; 0 for a temperature-0 row and beside an id -1.  The ids are those of the call without it
        (a drawn item of score -inf -- a row with fewer than top_N finite scores -- is not eligible: -1 stands there).
        ValueError without sample_temperature or without recommend.
        recommend with scan_dtype='bf16' (None / 'f32': the calls above, untouched): where the recommend streams, the
        scan past the first chunk of the vocabulary multiplies on the bf16 matrix pipe as a FILTER widened by a proven
        error bound, and what passes is re-scored in f32 (arx_topk_bf16.h) -- the ids are the top_N by (f32 score desc,
        logit index asc), as without it.  Composes with exclude_seen and the tags; NotImplementedError with
        sample_temperature or return_logprob.  Where the recommend does not stream (a small vocabulary) or the fused
        scan does not apply (a width other than 32 / 64 / 128) the call is the f32 one."""
        check_return_logprob(return_logprob, recommend, sample_temperature)
        bf16 = self._scan_bf16(scan_dtype, recommend, sample_temperature, return_logprob)
        sampled = recommend and sample_temperature is not None
        if sampled:
            # resolved once here: the chunked re-run after a candidate overflow must draw the same sample
            sample_seed = self.att_emb.next_sample_seed(sample_temperature, sample_seed)
        run = lambda: self.step_async(session, user_input, item_input, neg_item_input, item_sampled,
                                      item_sampled_id2idx, forward_only, recommend, recommend_new, loss,
                                      run_op, run_meta, exclude_seen=exclude_seen, tags_any=tags_any,
                                      tags_all=tags_all, sample_temperature=sample_temperature,
                                      sample_seed=sample_seed, return_logprob=return_logprob, scan_dtype=scan_dtype)
        if recommend:
            # (a candidate list of the fused top-k too short for this batch: the request once more, chunked)
            key = recommend_key(exclude_seen, tags_any is not None or tags_all is not None, sampled,
                                bool(return_logprob), bf16)
            self._plan(key)                    # builds the twin node / raises as the step would
            node = self._recommend_node(key)
            out = run_complete(node, run, lambda: self._plans.pop(key, None))
            if return_logprob:
                return out[0].cpu().numpy(), out[1].cpu().numpy()
            return out.cpu().numpy()
        out = run()
        if isinstance(out, list):
            return [o.cpu().numpy() for o in out]
        return float(out.read().item())

    # ---- batch drawing (hmf_model.py:230-260) ----
    def get_batch(self, data, loss='ce', hist=None):
        batch_user_input, batch_item_input = [], []
        for _ in range(self.batch_size):
            u, i, _t = random.choice(data)
            batch_user_input.append(u)
            batch_item_input.append(i)
        return batch_user_input, batch_item_input, []

    def get_permuted_batch(self, data):
        if self.data_length is None:
            self.data_length = len(data)
            self.start_index = 0
            self.train_permutation = np.random.permutation(self.data_length)
        if self.start_index + self.batch_size >= self.data_length:
            self.start_index = 0
            self.train_permutation = np.random.permutation(self.data_length)
        idx = self.train_permutation[self.start_index:self.start_index + self.batch_size]
        self.start_index += self.batch_size
        users = [data[j][0] for j in idx]
        items = [data[j][1] for j in idx]
        return users, items, None
