"""LinearSeq -- shared base of the skip-gram / CBOW recommenders (word2vec/linear_seq.py:11-121)
and the graph both build (word2vec/skipgram_model.py:12-137, cbow_model.py:12-140).

The two models differ only in the item half of the input embedding:
    skip-gram  train: mean([user, item_0])          test: mean([user, mean_i(item_i)])
    CBOW       train: mean([user, mean_i(item_i)])  test: the same
(item_i = mean over the attribute features of the i-th context item; `user` = mean over the
user's features).  With use_sep_item the context items read the 'item' tables and the scorer
the separate 'item_output' tables (embed_attribute.py:96-108).  All n context lookups are ONE
gather launch over the time-major id list; the mean over context positions is a column sum.
Where the context items have exactly one one-hot feature and n >= 2 the whole input embedding
x = 0.5 * user + (0.5 / n) * sum_t item_t is ONE launch (graph.WindowEmbed, fuse_window).

Losses: 'warp', 'ce', 'bbpr' score the whole catalogue in training; 'mw' / 'mce' train on the sampled pool
(n_sampled items, staged by step(item_sampled=...)) like the HMF model and only evaluate / recommend over the
catalogue -- streamed, without [mb, V] logits, past ARX_STREAM_TOPK_BYTES.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import explain
from .. import graph as G
from .. import ops
from .. import slate
from .. import topk as _topk
from ..attributes import embed_attribute
from ..attributes.embed_attribute import Dropout
from ..hmf.hmf_model import _Op, _Var
from ..topk import (StreamTopK, check_return_logprob, check_scan_dtype, excluding_twin, recommend_key, recommend_node,
                    run_complete)
from ..utils.checkpoint import Saver


class ContextMean(G.Node):
    """x = 0.5 * user + sum_t rows_t, rows = context lookups pre-scaled by 0.5 / n ([n*mb, d])."""

    requires_grad = True

    def __init__(self, rt, items, user, n, mb):
        super().__init__(rt, (mb, items.shape[1]), (items, user))
        self.n, self.mb = n, mb

    def forward(self, train):
        items, user = self.inputs
        x = self.alloc_value()
        d = self.shape[1]
        if self.n == 1:
            ops.axpby(1.0, items.value, 0.0, x)
        else:
            ops.col_sum(items.value.view(self.n, self.mb * d), x.view(-1), self.rt.ws)
        ops.add_rows_bcast(0.5, user.value, 1.0, x)

    def backward(self):
        items, user = self.inputs
        g = self.grad
        if items.requires_grad:
            ops.add_rows_bcast(1.0, g, items.grad_beta(), items.alloc_grad())
        if user.requires_grad:
            ops.add_rows_bcast(0.5, g, user.grad_beta(), user.alloc_grad())


class _FirstRows(G.Node):
    """First mb entries of the time-major context id list (= placeholder 'input0')."""

    def __init__(self, rt, parent, n):
        super().__init__(rt, (n,), (parent,))
        self.value = parent.value[:n]

    def forward(self, train):
        pass


class LinearSeq(object):
    def __init__(self, user_size, item_size, size, batch_size, learning_rate,
                 learning_rate_decay_factor, user_attributes=None, item_attributes=None,
                 item_ind2logit_ind=None, logit_ind2item_ind=None, n_input_items=0,
                 loss_function='ce', logit_size_test=None, dropout=1.0, top_N_items=100,
                 use_sep_item=True, n_sampled=None, output_feat=1, indices_item=None,
                 dtype='float32', params=None, use_graph=True, seed=0, cbow=False, fuse_window=None):
        self.user_size = user_size
        self.item_size = item_size
        self.top_N_items = top_N_items
        if user_attributes is not None:
            user_attributes.set_model_size(size)
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
        self.loss_function = loss = loss_function
        self.n_input_items = n_input_items
        self.output_feat = output_feat
        self.n_sampled = n_sampled
        self.batch_size = mb = batch_size
        self.dropout = dropout
        self.dtype = dtype
        if loss not in ('warp', 'ce', 'bbpr', 'mw', 'mce'):
            raise NotImplementedError("loss %r (built here: 'warp', 'ce', 'bbpr', 'mw', 'mce')" % loss)
        sampled = loss in ('mw', 'mce')
        if sampled:
            # the reference builds sampled_logits / target_score / compute_loss(.., 'mw') for this family
            # (skipgram_model.py:104-116, cbow_model.py:107-119) and only forgets to assign batch_loss_test on
            # that branch; this build defines it: 'mw' evaluates with the full-vocabulary 'warp' (run_w2v.py:377),
            # 'mce' (build-defined sampled softmax, arx.h) with the full softmax 'ce' (run_w2v.py:335,385)
            if n_sampled is None:
                raise ValueError("loss %r trains on the sampled pool: n_sampled must be given" % loss)
            if int(n_sampled) <= 0 or int(n_sampled) % 4 != 0:
                raise ValueError("n_sampled must be a positive multiple of 4, got %r" % (n_sampled,))

        self.rt = rt = G.Runtime(learning_rate=learning_rate, use_graph=use_graph)
        self._lr_decay = learning_rate_decay_factor
        self.learning_rate = _Var(lambda: rt.lr_host)
        self.learning_rate_decay_op = _Op(lambda: rt.set_learning_rate(rt.lr_host * self._lr_decay))
        self.global_step = _Var(lambda: rt.global_step)
        self.item_target = G.IdsInput(rt, mb, 'item')               # mapped (logit) target
        self.item_id_target = G.IdsInput(rt, mb, 'item_id')

        n_input = max(n_input_items, 1)
        self._n_input = n_input
        m = embed_attribute.EmbeddingAttribute(user_attributes, item_attributes, mb, n_sampled, n_input,
                                               use_sep_item, item_ind2logit_ind, logit_ind2item_ind,
                                               params=params, runtime=rt, seed=seed)
        self.att_emb = m
        user, _ = m.get_batch_user(1.0, False)                                    # :80
        feats = m._select_feats(m.item_feats, m.item_attributes)
        eligible = len(feats) == 1 and feats[0].kind == 'cat' and n_input >= 2
        self.fuse_window = bool(eligible and (fuse_window is None or fuse_window))
        if self.fuse_window:
            # x = 0.5 * user + (0.5 / n) * sum_t item_t in one launch; one [mb, d] gradient row per window
            mean_all = G.WindowEmbed(rt, m.input_all, feats, n_input, mb, out_scale=0.5 / n_input, base=user,
                                     base_scale=0.5)
        else:
            ctx_all = G.EntityEmbed(rt, m.input_all, feats, with_bias=False, out_scale=0.5 / n_input)
            mean_all = ContextMean(rt, ctx_all, user, n_input, mb)
        if cbow or n_input == 1:
            x_train = mean_all                                                    # cbow_model.py:87-90
        else:
            first = G.EntityEmbed(rt, _FirstRows(rt, m.input_all, mb), feats, with_bias=False, out_scale=0.5)
            x_train = ContextMean(rt, first, user, 1, mb)                         # skipgram_model.py:87
        if float(dropout) != 1.0:
            rt.keep_prob = float(dropout)
            x_train = Dropout(rt, x_train)                                      # :88
        x_test = user if n_input_items == 0 else mean_all                         # :91-99
        logits_test = m.get_prediction(x_test, output_feat=output_feat)
        if sampled:
            # no [mb, V] node on the training side (skipgram_model.py:104-116)
            sampled_logits = m.get_prediction(x_train, 'sampled', output_feat=output_feat)
            target_score = m.get_target_score(x_train, self.item_id_target)
            batch_loss = m.compute_loss(sampled_logits, target_score, loss)
            # (output_feat 2 / 3 pool in score space: no pool node to stream from)
            pool = logits_test.inputs[1] if isinstance(logits_test, G.Prediction) else None
            batch_loss_test = m.sampled_eval_loss(loss, x_test, logits_test, self.item_target, mb, mb, pool)
        else:
            logits = m.get_prediction(x_train, output_feat=output_feat)
            batch_loss = m.compute_loss(logits, self.item_target, loss)
            batch_loss_test = m.compute_loss(logits_test, self.item_target, loss)
        self.set_mask, self.reset_mask = {}, {}
        if loss in ('warp', 'bbpr', 'mw', 'mce'):
            self.set_mask, self.reset_mask = m.get_warp_mask()
        self.loss = G.MeanLoss(rt, batch_loss)
        self.loss_test = G.MeanLoss(rt, batch_loss_test)
        self.output = logits_test
        self.topk = recommend_node(rt, logits_test, min(top_N_items, self.logit_size), mb)    # :135
        self.indices = self.topk
        self._plans = {}
        self.saver = Saver(self)

    def prepare_warp(self, pos_item_set, pos_item_set_eval):
        self.att_emb.prepare_warp(pos_item_set, pos_item_set_eval)

    def prepare_recommend_exclusions(self, item_sets):
        """The items step(recommend=True, exclude_seen=True) leaves out per user: {user_index: items} or a (ptr, items)
        CSR pair in item-index space (EmbeddingAttribute.prepare_recommend_exclusions).  A second call replaces them."""
        for key in ('recommend_ex', 'recommend_ex_sample', 'recommend_ex_tags_sample', 'recommend_ex_sample_logp',
                    'recommend_ex_tags_sample_logp', 'recommend_ex_bf16', 'recommend_ex_tags_bf16'):
            self._plans.pop(key, None)
        _topk.drop_list_logp_plans(self, '_ex')
        self.att_emb.prepare_recommend_exclusions(item_sets)

    def prepare_item_tags(self, tags):
        """The items' 32-bit tag words for step(recommend=True, tags_any=, tags_all=): an integer array [n_items] or
        {item_index: bit numbers 0..31} (EmbeddingAttribute.prepare_item_tags).  A second call replaces them."""
        for key in ('recommend_tags', 'recommend_ex_tags', 'recommend_tags_sample', 'recommend_ex_tags_sample',
                    'recommend_tags_sample_logp', 'recommend_ex_tags_sample_logp', 'recommend_tags_bf16',
                    'recommend_ex_tags_bf16'):
            self._plans.pop(key, None)
        _topk.drop_list_logp_plans(self, '_tags')
        self.att_emb.prepare_item_tags(tags)

    def similar_items(self, logit_ids, k, include_self=False, return_values=False, chunk=65536,
                      return_logprob=False, scan_dtype=None):
        """Cosine nearest neighbours of items (logit indices) over the full vocabulary, in the OUTPUT item latents the
        model scores against (EmbeddingAttribute.similar_items); output_feat 2 / 3: NotImplementedError."""
        return self.att_emb.similar_items(logit_ids, k, include_self=include_self, return_values=return_values,
                                          return_logprob=return_logprob, scan_dtype=scan_dtype,
                                          chunk=chunk, output_feat=self.output_feat)

    def prepare_item_groups(self, groups):
        """The items' groups for score_items(max_per_group=): an integer array [n_items] or {item_index: group} in
        item-index space, mapped to one int32 per logit column (arx.slate.item_group_ids).  A second call replaces
        them."""
        slate.prepare_item_groups(self, groups)

    def score_items(self, user_input, item_input, candidates, k=None, diversify=None, max_per_group=None,
                    sample_temperature=None, sample_seed=None, return_logprob=False):
        """Row r of one full batch (user_input and the [n_input][mb] context item_input, the rules of
        step(recommend=True)) against its own slate candidates[r]: [batch_size, C] logit indices, -1 an empty slot.
        The latent is recommend's x_test of the full window, the pool the OUTPUT item latents; dropout off.
        k None: float32 [mb, C] on the device (-inf at empty slots); 1 <= k <= min(1024, C): (ids, values)
        [mb, k] by (score desc, slot asc), (-1, -inf) past the live slots (LatentProductModel.score_items;
        arx.slate).  output_feat 2 / 3: NotImplementedError.
        diversify (lambda in [0, 1]) and / or max_per_group (after prepare_item_groups()): k is required and (ids,
        values) come in the selection order of the greedy MMR re-rank, cosines between the OUTPUT item latents
        (LatentProductModel.score_items states the rule):
            cands = model.step(None, users, context, recommend=True)
            ids, values = model.score_items(users, context, cands, k, diversify=0.7)
        sample_temperature (a number >= 0 or one per row) / sample_seed / return_logprob: k is required and (ids,
        values) are k distinct items DRAWN from softmax(score / tau) over the row's distinct live candidates, without
        replacement, in selection order, with the noise of the sampled recommend; return_logprob=True adds logprob
        float32 [mb, k], the log-probability of each draw given those before it (LatentProductModel.score_items states
        the rules and the errors; sample_seed=None takes att_emb's draw counter):
            ids, values, logp = model.score_items(users, context, cands, k, sample_temperature=0.5, sample_seed=s,
                                                  return_logprob=True)"""
        def feed():
            self.att_emb.add_input({}, user_input, item_input, recommend=True, loss=self.loss_function)
        return slate.score_items(self, feed, candidates, k, diversify, max_per_group, sample_temperature, sample_seed,
                                 return_logprob)

    def explain_items(self, user_input, item_input, items, top=3):
        """The scores score_items gives row r of one full batch (user_input and the [n_input][mb] context item_input)
        for the items of its slate items[r] ([batch_size, C] logit indices, -1 an empty slot), taken apart into the
        parts of the OUTPUT item latents' features and the `top` largest single-token contributions of their bags:
        arx.explain.Explanation(score, feature, bias, token_value, token_id, token_feature, features)
        (LatentProductModel.explain_items states the fields, the order and the errors; arx_explain.h).  output_feat
        2 / 3: NotImplementedError.  Not offered: SeqModel, the sharded models, a "most negative" or absolute-value
        order, merged repeats."""
        def feed():
            self.att_emb.add_input({}, user_input, item_input, recommend=True, loss=self.loss_function)
        return explain.explain_items(self, feed, items, top)

    def list_logprob(self, user_input, item_input, lists, sample_temperature, exclude_seen=False, tags_any=None,
                     tags_all=None, return_values=False, return_why=False):
        """The log-probability of the given ordered lists [batch_size, k] (logit indices, -1 an empty slot) under the
        policy of step(recommend=True, sample_temperature=) for one full batch (user_input and the [n_input][mb]
        context item_input): float32 [mb, k] numpy, 0 at a -1, -inf at an entry the policy could never draw; with
        return_values / return_why the tuple (logprob[, values][, why]).  LatentProductModel.list_logprob states the
        rule, the reason codes and the errors (arx_list_logp.h); output_feat 2 / 3: NotImplementedError.
            ids, logged = model.step(None, users, context, recommend=True, sample_temperature=0.7, return_logprob=True)
            target = other.list_logprob(users, context, ids, 0.7)"""
        def feed():
            self.att_emb.add_input({}, user_input, item_input, recommend=True, loss=self.loss_function)
        return _topk.list_logprob(self, feed, lists, sample_temperature, exclude_seen, tags_any, tags_all,
                                  return_values, return_why)

    def _plan(self, key):
        if key not in self._plans:
            rt, m, loss = self.rt, self.att_emb, self.loss_function
            if key == 'train':
                masks = [m.mask[loss]] if loss in m.mask else []
                self._plans[key] = G.Plan(rt, [self.loss], True, masks)
            elif key == 'eval':
                self._plans[key] = G.Plan(rt, [self.loss_test], False, m.eval_masks(loss, self.loss_test.inputs[0]))
            elif key == 'recommend_ex':
                if getattr(self, 'topk_ex', None) is None:      # on first use
                    self.topk_ex = excluding_twin(rt, self.topk, m.exclusion_args)
                self._plans[key] = G.Plan(rt, [self.topk_ex], False, [])
            elif key == 'recommend_tags':
                if getattr(self, 'topk_tags', None) is None:
                    self.topk_tags = excluding_twin(rt, self.topk, tag_args=m.tag_args)
                self._plans[key] = G.Plan(rt, [self.topk_tags], False, [])
            elif key == 'recommend_ex_tags':
                if getattr(self, 'topk_ex_tags', None) is None:
                    self.topk_ex_tags = excluding_twin(rt, self.topk, m.exclusion_args, m.tag_args)
                self._plans[key] = G.Plan(rt, [self.topk_ex_tags], False, [])
            elif key.endswith('_bf16'):        # the twins whose fused scan filters in bf16 (topk.recommend_key)
                nodes = self.__dict__.setdefault('_bf16_nodes', {})
                if key not in nodes:
                    nodes[key] = excluding_twin(rt, self.topk, m.exclusion_args if '_ex' in key else None,
                                                m.tag_args if '_tags' in key else None, scan_bf16=True)
                self._plans[key] = G.Plan(rt, [nodes[key]], False, [])
            elif key.endswith('_sample') or key.endswith('_sample_logp'):   # the sampled twins (topk.recommend_key)
                nodes = self.__dict__.setdefault('_sample_nodes', {})
                if key not in nodes:
                    nodes[key] = excluding_twin(rt, self.topk, m.exclusion_args if '_ex' in key else None,
                                                m.tag_args if '_tags' in key else None, sample_args=m.sample_args,
                                                logp=key.endswith('_logp'))
                self._plans[key] = G.Plan(rt, [nodes[key]], False, [])
            else:
                self._plans[key] = G.Plan(rt, [self.topk], False, [])
        return self._plans[key]

    def _recommend(self, key):
        """Run the 'recommend' / 'recommend_ex' / 'recommend_tags' / 'recommend_ex_tags' plan; a streaming top-k whose fused candidate lists overflowed runs
        once more on the chunked path (as LatentProductModel.step)."""
        self._plan(key)
        node = self._bf16_nodes[key] if key.endswith('_bf16') else \
               self._sample_nodes[key] if key.endswith('_sample') or key.endswith('_sample_logp') else \
               {'recommend': self.topk, 'recommend_ex': getattr(self, 'topk_ex', None),
                'recommend_tags': getattr(self, 'topk_tags', None),
                'recommend_ex_tags': getattr(self, 'topk_ex_tags', None)}[key]
        # (the placeholders still hold this request's ids in the second run)
        run_complete(node, lambda: self._plan(key).run(), lambda: self._plans.pop(key, None))
        if key.endswith('_logp'):
            return node.indices.cpu().numpy(), node.logp.cpu().numpy()
        return node.indices.cpu().numpy()

    def step(self, session, user_input, item_input=None, item_output=None, item_sampled=None,
             item_sampled_id2idx=None, forward_only=False, recommend=False, recommend_new=False,
             loss=None, run_op=None, run_meta=None, exclude_seen=False, tags_any=None, tags_all=None,
             sample_temperature=None, sample_seed=None, return_logprob=False, scan_dtype=None):
        """linear_seq.py:67-121.  item_input: [n_input][mb] context items (time-major);
        item_output: [mb] target items.  Returns the mean loss (train / forward_only) or the
        top-N logit indices [mb, top_N] (recommend; exclude_seen=True: without each user's items of
        prepare_recommend_exclusions, -1 where a user has fewer eligible items; tags_any / tags_all -- an int or one
        int per row: only the items eligible by their tag words of prepare_item_tags, composing with exclude_seen;
        sample_temperature / sample_seed: top_N distinct items DRAWN with probability proportional to
        exp(score / temperature), in selection order; return_logprob=True with it: (ids, logprob float32 [mb, top_N]), the
        log-probability of every draw -- LatentProductModel.step states the rules; ValueError without
        sample_temperature or without recommend; scan_dtype='bf16': the streaming scan filters on the bf16 matrix
        pipe and re-scores in f32 -- the same ids; not with sample_temperature / return_logprob).
        'mw' / 'mce': item_sampled (n_sampled item ids) stages a new pool -- the first training step needs one,
        later steps keep it until the next is given (run_w2v.py:315-317); item_sampled_id2idx is the host twin of
        the pool's item -> slot map.  forward_only evaluates 'mw' with the full-vocabulary 'warp' loss and 'mce'
        with 'ce' (the runner passes loss='warp' there, run_w2v.py:377)."""
        m = self.att_emb
        sampled = self.loss_function in ('mw', 'mce')
        if recommend_new:
            raise NotImplementedError("indices_test is never built by the reference (linear_seq.py:98)")
        check_return_logprob(return_logprob, recommend, sample_temperature)
        bf16 = check_scan_dtype(scan_dtype, recommend, sample_temperature, return_logprob) and \
            isinstance(self.topk, StreamTopK)
        if recommend and exclude_seen:
            m.exclusion_args()                 # ValueError before any feed when nothing was prepared
        tagged = recommend and (tags_any is not None or tags_all is not None)
        if tagged:
            m.feed_tag_words(tags_any, tags_all)                  # ValueError before any other feed
        drawn = recommend and sample_temperature is not None
        if drawn:
            m.feed_sample(sample_temperature, sample_seed)        # (fed once: the chunked re-run draws the same sample)
        if sampled and not (recommend or forward_only) and item_sampled is None and m._old_pool is None:
            raise ValueError("the first %r training step needs item_sampled (the pool of n_sampled items)"
                             % self.loss_function)
        if not recommend:
            if isinstance(item_output, torch.Tensor):
                self.item_id_target.feed(item_output)
                m.target_mapping_device(self.item_id_target.value, self.item_target.value)
            else:
                self.item_target.feed(m.target_mapping([item_output])[0])          # :76-77
                if sampled:
                    self.item_id_target.feed(item_output)                          # raw ids: the target score (:79-80)
        update_sampled, _, _ = m.add_input({}, user_input, item_input, neg_item_input=None,
                                           item_sampled=item_sampled, item_sampled_id2idx=item_sampled_id2idx,
                                           forward_only=forward_only, recommend=recommend,
                                           loss=loss or self.loss_function)
        for op in update_sampled:              # stage the pool (embed_attribute.py:320-348)
            op()
        if recommend:
            return self._recommend(recommend_key(exclude_seen, tagged, drawn, bool(return_logprob), bf16))
        if forward_only:
            self._plan('eval').run()
            return float(self.loss_test.read().item())
        self._plan('train').run()
        self.rt.global_step += 1
        return float(self.loss.read().item())
