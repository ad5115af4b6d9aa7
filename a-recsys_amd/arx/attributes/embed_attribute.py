"""EmbeddingAttribute -- the reference's hot-path class on MI355X.

Same constructor and method surface as attributes/embed_attribute.py:19-747 of
the reference (get_batch_user / get_batch_item / get_prediction /
get_target_score / compute_loss / get_warp_mask / prepare_warp /
target_mapping / add_input / get_*_model_size); the bodies build arx.graph
nodes whose kernels live in libarx.so instead of TF ops.  Differences a caller
can observe:
  * returned objects are arx.graph.Node handles, not tf.Tensors;
  * the scorer is evaluated in embedding space (pool rows gathered, then one
    [mb,d]x[d,S] GEMM) instead of multiplying the whole attribute table
    (:171,188) -- algebraically identical, summation order differs;
  * errors raise ValueError / NotImplementedError instead of print+exit();
  * tables may be supplied through `params` (reference variable names) --
    otherwise glorot-uniform like tf.get_variable's default.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import graph as G
from .. import ops
from ..topk import (TopKScan, logits_too_big, no_return_logprob, no_scan_dtype, sample_params, similar_scan,
                    tag_words)
from ..utils.prepare_train import pair_draw_tables

# the full-vocabulary loss a model trained with a sampled loss evaluates with (hmf_model.py:130,144; 'mce' -> 'ce':
# run_hmf.py:255,304)
EVAL_LOSS_OF = {'mw': 'warp', 'mce': 'ce'}


def _np_i32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int32))


def exclusion_csr(item_sets, n_keys, item2logit):
    """Per-user exclusion lists of LOGIT columns as a CSR pair (ptr int32 [n_keys + 1], cols int32 [>= 1]) for the
    recommend path (arx.h arx_topk_exclude_fill).  item_sets: {user_index: items} or a (ptr, items) CSR pair over
    user indices, in ITEM-index space (the forms prepare_warp accepts).  Items go through item2logit (a numpy array,
    -1 where an item has no logit); items without a logit, negative items and users outside [0, n_keys) are dropped;
    every list comes out sorted ascending without duplicates."""
    item2logit = np.asarray(item2logit)
    if isinstance(item_sets, tuple):
        ptr = np.asarray(item_sets[0], dtype=np.int64)
        items = np.asarray(item_sets[1], dtype=np.int64).reshape(-1)
        if len(ptr) == 0:
            ptr = np.zeros(1, dtype=np.int64)
        if np.any(np.diff(ptr) < 0) or ptr[0] != 0 or ptr[-1] > len(items):
            raise ValueError("exclusion CSR: ptr must start at 0, not decrease and end within the items")
        users = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
        items = items[:ptr[-1]]
    elif isinstance(item_sets, dict):
        keys = [u for u, its in item_sets.items() if len(its)]
        parts = [np.asarray(list(item_sets[u]), dtype=np.int64).reshape(-1) for u in keys]
        lens = np.asarray([len(x) for x in parts], dtype=np.int64)
        users = np.repeat(np.asarray(keys, dtype=np.int64), lens)
        items = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    else:
        raise ValueError("exclusions: a {user: items} dict or a (ptr, items) CSR pair")
    ok = (users >= 0) & (users < n_keys) & (items >= 0) & (items < len(item2logit))
    users, items = users[ok], items[ok]
    cols = item2logit[items].astype(np.int64)
    ok = cols >= 0
    users, cols = users[ok], cols[ok]
    order = np.lexsort((cols, users))
    users, cols = users[order], cols[order]
    if len(users):
        keep = np.ones(len(users), dtype=bool)
        keep[1:] = (users[1:] != users[:-1]) | (cols[1:] != cols[:-1])
        users, cols = users[keep], cols[keep]
    out_ptr = np.zeros(n_keys + 1, dtype=np.int64)
    np.cumsum(np.bincount(users, minlength=n_keys), out=out_ptr[1:])
    if out_ptr[-1] >= 2 ** 31:
        raise ValueError("exclusion lists: more than 2^31 - 1 entries")
    if len(cols) == 0:
        cols = np.zeros(1, dtype=np.int64)          # (a valid device pointer; every list is empty)
    return out_ptr.astype(np.int32), cols.astype(np.int32)


def item_tag_words(tags, item2logit, n_logits):
    """One 32-bit tag word per LOGIT column, as int32 bit patterns [n_logits], for the recommend path within item tags
    (arx_tags.h arx_topk_tags_fill).  tags, per ITEM index: an integer array [n_items] of words in [0, 2^32), or
    {item_index: iterable of bit numbers 0..31}.  Items go through item2logit (a numpy array, -1 where an item has no
    logit): an item without a logit is skipped, a column without an item gets 0; where two items share a column their
    words are OR-ed."""
    item2logit = np.asarray(item2logit)
    if isinstance(tags, dict):
        items = np.fromiter(tags.keys(), dtype=np.int64, count=len(tags))
        words = np.zeros(len(tags), dtype=np.uint64)
        for j, bits in enumerate(tags.values()):
            for b in bits:
                if isinstance(b, (bool, np.bool_)) or not isinstance(b, (int, np.integer)) or not 0 <= int(b) <= 31:
                    raise ValueError("item tags: bit numbers must be integers in 0..31, got %r" % (b,))
                words[j] |= np.uint64(1 << int(b))
        if len(items) and items.min() < 0:
            raise ValueError("item tags: negative item index")
    else:
        words = tags.cpu().numpy() if isinstance(tags, torch.Tensor) else np.asarray(tags)
        if words.ndim != 1 or words.dtype == np.bool_ or not np.issubdtype(words.dtype, np.integer):
            raise ValueError("item tags: an integer array [n_items] or a {item_index: bit numbers} dict")
        if len(words) and (words.min() < 0 or words.max() >= 2 ** 32):
            raise ValueError("item tags: words must lie in [0, 2^32)")
        items = np.arange(len(words), dtype=np.int64)
        words = words.astype(np.uint64)
    ok = items < len(item2logit)
    items, words = items[ok], words[ok]
    cols = item2logit[items].astype(np.int64)
    ok = (cols >= 0) & (cols < n_logits)
    out = np.zeros(n_logits, dtype=np.uint32)
    np.bitwise_or.at(out, cols[ok], words[ok].astype(np.uint32))
    return out.view(np.int32)


class FeatureList(list):
    """What _get_embedded(concatenation=False) returns in the reference: the list
    cat_list + mulhot_list.  The fused node computing their mean is attached, so
    arx.graph-level reduce_mean(list, 0) costs nothing extra."""

    def __init__(self, mean_node, n):
        super().__init__([mean_node] * n)
        self.mean_node = mean_node


class ZeroEmbed(G.Node):
    """tf.zeros([mb, dim]) of the no_id branch (embed_attribute.py:356-366)."""

    def __init__(self, rt, n, d):
        super().__init__(rt, (n, d))
        self.value = torch.zeros((n, d), dtype=torch.float32, device=rt.device)

    def forward(self, train):
        pass


class TargetMapping(G.Node):
    """item_target = item_ind2logit_ind[item_id_target] (embed_attribute.py:676-695 target_mapping)
    as a node of the step: the mapping runs inside the captured plan instead of as an eager launch
    in front of it (a B=64 step is bound by exactly those).  `feed` keeps the placeholder
    interface for host-mapped targets (the in-plan mapping rewrites the same values)."""

    def __init__(self, rt, ids_node, emb, name):
        super().__init__(rt, ids_node.shape, (ids_node,))
        self.emb, self.name = emb, name
        self.value = torch.zeros(ids_node.shape[0], dtype=torch.int32, device=rt.device)

    def feed(self, arr):
        src = arr if isinstance(arr, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(arr, dtype=np.int32)))
        self.value.copy_(src.reshape(self.value.shape), non_blocking=True)

    def forward(self, train):
        if self.emb._item2logit_dev is None:
            raise ValueError("target mapping needs item_ind2logit_ind")
        ops.sparse_site_onehot(self.emb._item2logit_dev, self.inputs[0].value, 0, 0.0, self.value, None, None)


class Dropout(G.Node):
    """tf.nn.dropout (embed_attribute.py:236; DropoutWrapper seqModel.py:100,103).  keep_prob is
    read from rt.keep_prob when the plan is built / captured (1.0 => identity; changing it makes
    the plans re-capture); RNG is counter-based (not TF's Philox): parity tests replay the
    drawn masks (`keep`) through the oracle."""

    requires_grad = True
    uses_dropout = True          # plans with such nodes bump the device step counter every step

    def __init__(self, rt, x):
        super().__init__(rt, x.shape, (x,))
        self.keep = None
        rt.dropout_calls += 1
        self.sid = rt.dropout_calls          # fixed stream id of this node; the step counter
                                             # (rt.step_dev, bumped once per train step inside the
                                             # plan / captured graph) varies the draw per step

    def forward(self, train):
        x = self.inputs[0]
        kp = self.rt.keep_prob if train else 1.0
        self.kp_used = kp
        if kp >= 1.0:
            self.value = x.value
            return
        if self.keep is None:
            self.keep = torch.empty(int(np.prod(self.shape)), dtype=torch.uint8, device=self.rt.device)
            self._own = torch.empty(self.shape, dtype=torch.float32, device=self.rt.device)
        self.value = self._own
        ops.dropout_fwd_step(x.value, kp, self.rt.seed * 1000003 + self.sid, self.rt.step_dev, self.value,
                             self.keep)

    def alloc_grad(self):
        x = self.inputs[0]
        if getattr(self, 'kp_used', 1.0) >= 1.0:
            self.grad = x.alloc_grad()          # identity: share the gradient buffer
            return self.grad
        return super().alloc_grad()

    def grad_beta(self):
        if getattr(self, 'kp_used', 1.0) >= 1.0:
            self._grad_written = True
            return self.inputs[0].grad_beta()
        return super().grad_beta()

    def backward(self):
        if self.kp_used >= 1.0:
            return
        x = self.inputs[0]
        if x.grad_beta() != 0.0:
            raise NotImplementedError("dropout input with several consumers")
        ops.dropout_bwd(self.grad, self.keep, self.kp_used, x.alloc_grad())


class EmbeddingAttribute(object):
    def __init__(self, user_attributes, item_attributes, mb, n_sampled, input_steps=0,
                 item_output=False, item_ind2logit_ind=None, logit_ind2item_ind=None,
                 indices_item=None, devices=['/gpu:0'], params=None, runtime=None, seed=0):
        self.user_attributes = user_attributes
        self.item_attributes = item_attributes
        self.batch_size = mb
        self.n_sampled = n_sampled
        self.input_steps = input_steps
        self.item_output = item_output
        self.num_item_features = item_attributes.num_features_cat + item_attributes.num_features_mulhot
        self.item_ind2logit_ind = item_ind2logit_ind
        self.logit_ind2item_ind = logit_ind2item_ind
        if logit_ind2item_ind is not None:
            self.logit_size = len(logit_ind2item_ind)
        self.indices_item = indices_item if indices_item is not None else range(self.logit_size)
        self.devices = devices
        self.rt = runtime if runtime is not None else G.Runtime()
        rt = self.rt
        rt.seed = seed
        self._rng = torch.Generator(device=rt.device)
        self._rng.manual_seed(seed)
        params = params or {}

        # ---- attribute maps -> device constants (embed_attribute.py:308-318) ----
        self.att = {'user': self._init_attributes(user_attributes),
                    'item': self._init_attributes(item_attributes)}
        if item_output:
            self.att['item_output'] = self.att['item']
        self.n_users = self._n_entities(user_attributes)
        self.n_items = self._n_entities(item_attributes)

        # ---- tables (:265-306) ----
        self.tables = {}
        self.user_feats = self._embedded(user_attributes, 'user', False, params)
        self.item_feats = self._embedded(item_attributes, 'item', True, params)
        if item_output:
            self.item_out_feats = self._embedded(item_attributes, 'item_output', True, params)
        else:
            self.item_out_feats = self.item_feats

        # ---- placeholders (:72-93) ----
        self.u_indices = {'input': G.IdsInput(rt, mb, 'user_input_ind')}
        self.i_indices = {}
        self.i_indices['pos'] = G.IdsInput(rt, mb, 'item_pos_ind')
        self.i_indices['neg'] = G.IdsInput(rt, mb, 'item_neg_ind')
        if n_sampled is not None:
            self.i_indices['sampled_pass'] = G.IdsInput(rt, n_sampled, 'item_sampled_ind')
        if input_steps > 0:
            # one [L*mb] time-major buffer; 'input{t}' are row slices of it so the
            # whole sequence is looked up by ONE launch
            self.input_all = G.IdsInput(rt, input_steps * mb, 'item_input_all')
            for step in range(input_steps):
                self.i_indices['input{}'.format(step)] = ('input_all', step)

        # ---- pools (:96-116) ----
        self._pool_nodes = {}
        self._old_pool = None
        self.item2slot = None
        if n_sampled is not None:
            self.item2slot = torch.full((self.n_items + 1,), -1, dtype=torch.int32, device=rt.device)
            # 1 bit per item "in the pool?" in front of the map (arx_slot_map_attach_bitmap)
            self._pool_bits = torch.zeros(((self.n_items + 1) + 32) // 32, dtype=torch.int32, device=rt.device)
            ops.slot_map_attach_bitmap(self.item2slot, self._pool_bits)
        self._item2logit_dev = None
        self._item2logit_np = None
        if item_ind2logit_ind is not None:
            m = np.full((self.n_items + 2,), -1, dtype=np.int32)
            if isinstance(item_ind2logit_ind, dict):
                keys = np.fromiter(item_ind2logit_ind.keys(), dtype=np.int64, count=len(item_ind2logit_ind))
                vals = np.fromiter(item_ind2logit_ind.values(), dtype=np.int64, count=len(item_ind2logit_ind))
                ok = keys < len(m)
                m[keys[ok]] = vals[ok]
            else:
                a = np.asarray(item_ind2logit_ind)
                m[:len(a)] = a
            self._item2logit_np = m
            self._item2logit_dev = rt.upload(m, torch.int32)

        self.mask = {}
        self.pos_item_set = None
        self.pos_item_set_eval = None
        self._pos_dev = {}
        self.set_mask, self.reset_mask = {}, {}

    # ------------------------------------------------------------------ setup
    @staticmethod
    def _n_entities(att):
        if att.num_features_cat > 0:
            return len(att.features_cat[0]) - 1
        return len(att.mulhot_lengths[0]) - 1

    def _init_attributes(self, att):
        rt = self.rt
        cat = [rt.upload(_np_i32(att.features_cat[i]), torch.int32) for i in range(att.num_features_cat)]
        mul = []
        for i in range(att.num_features_mulhot):
            lens = _np_i32(att.mulhot_lengths[i])
            mul.append((rt.upload(_np_i32(att.features_mulhot[i]), torch.int32),
                        rt.upload(_np_i32(att.mulhot_starts[i]), torch.int32),
                        rt.upload(lens, torch.int32), int(lens.max()) if len(lens) else 1))
        return cat, mul

    def _new_var(self, name, shape, params):
        rt = self.rt
        if name in params:
            a = np.asarray(params[name], dtype=np.float32).reshape(shape)
            return rt.upload(a, torch.float32).contiguous()
        # tf.get_variable default initializer: glorot_uniform
        fan_in, fan_out = shape[0], (shape[1] if len(shape) > 1 else 1)
        lim = math.sqrt(6.0 / (fan_in + fan_out))
        t = torch.empty(shape, dtype=torch.float32, device=rt.device)
        t.uniform_(-lim, lim, generator=self._rng)
        return t

    def _embedded(self, attributes, prefix, with_bias, params):
        """embed_attribute.py:265-306 _embedded + _embedded_bias."""
        feats = []
        maps_cat, maps_mul = self.att['item' if prefix.startswith('item') else 'user']
        for i in range(attributes.num_features_cat):
            d = attributes._embedding_size_list_cat[i]
            V = attributes._embedding_classes_list_cat[i]
            ename = '%sembed_cat_%d' % (prefix, i)
            bname = '%s_bias_cat_%d' % (prefix, i) if with_bias else None
            E = self._new_var(ename, (V, d), params)
            b = self._new_var(bname, (V, 1), params).reshape(V).contiguous() if with_bias else None
            t = G.Table(ename, bname, E, b)
            self.tables[ename] = t
            feats.append(G.Feature('cat', t, (maps_cat[i],)))
        for i in range(attributes.num_features_mulhot):
            d = attributes._embedding_size_list_mulhot[i]
            V = attributes._embedding_classes_list_mulhot[i]
            ename = '%sembed_mulhot_%d' % (prefix, i)
            bname = '%s_bias_mulhot_%d' % (prefix, i) if with_bias else None
            E = self._new_var(ename, (V, d), params)
            b = self._new_var(bname, (V, 1), params).reshape(V).contiguous() if with_bias else None
            t = G.Table(ename, bname, E, b)
            self.tables[ename] = t
            vals, starts, lens, mx = maps_mul[i]
            feats.append(G.Feature('mulhot', t, (vals, starts, lens), max_len=mx))
        return feats

    # ------------------------------------------------------------- variables
    def get_params(self):
        """{reference variable name: numpy array} (tables [Vf,d], biases [Vf,1])."""
        out = {}
        for t in self.tables.values():
            out[t.name] = t.E.cpu().numpy()
            if t.bias is not None:
                out[t.bias_name] = t.bias.cpu().numpy().reshape(-1, 1)
        return out

    def get_slots(self):
        out = {}
        for t in self.tables.values():
            out[t.name] = t.acc.cpu().numpy()
            if t.bias is not None:
                out[t.bias_name] = t.bias_acc.cpu().numpy().reshape(-1, 1)
        return out

    # --------------------------------------------------------------- lookups
    def _select_feats(self, feats, attributes, no_id=False, no_attribute=False):
        ncat = attributes.num_features_cat
        cat, mul = feats[:ncat], feats[ncat:]
        if no_attribute:                                  # embed_attribute.py:368-369
            cat, mul = cat[:1], []
        if no_id:
            cat = cat[1:]                                 # :372-373
        return cat + mul

    def get_batch_user(self, keep_prob, concat=True, no_id=False, device='/gpu:0'):
        """embed_attribute.py:222-237 -> (embedded_user [mb, d or sum d], None)."""
        ua = self.user_attributes
        ids = self.u_indices['input']
        if no_id and ua.num_features_cat == 1:            # :356-366
            node = ZeroEmbed(self.rt, self.batch_size, ua._embedding_size_list_cat[0])
        else:
            feats = self._select_feats(self.user_feats, ua, no_id=no_id)
            node = G.EntityEmbed(self.rt, ids, feats, with_bias=False, concat=concat)
        if not (isinstance(keep_prob, (int, float)) and float(keep_prob) == 1.0):
            if isinstance(keep_prob, (int, float)):
                self.rt.keep_prob = float(keep_prob)
            node = Dropout(self.rt, node)
        return node, None

    def _ids_node(self, name):
        h = self.i_indices[name]
        if isinstance(h, tuple):          # 'input{t}': time step t of the sequence buffer (:87-90)
            step = h[1]
            mb = self.batch_size
            h = G.IdsSlice(self.rt, self.input_all, step * mb, mb, 'item_%s_ind' % name)
            self.i_indices[name] = h
        return h

    def get_batch_item(self, name, batch_size, concat=False, keep_prob=1.0, no_attribute=False,
                       device='/gpu:0'):
        """embed_attribute.py:239-254.  concat=False returns (feature list, bias);
        reduce the list with arx.graph-level `reduce_mean` (== tf.reduce_mean(.., 0))."""
        if name not in self.i_indices:
            raise ValueError("unknown item placeholder %r" % name)
        if keep_prob != 1.0:
            raise NotImplementedError('otherwise not implemented')     # :242
        ids = self._ids_node(name)
        feats = self._select_feats(self.item_feats, self.item_attributes, no_attribute=no_attribute)
        if concat:
            node = G.EntityEmbed(self.rt, ids, feats, with_bias=False, concat=True)
            return node, None
        node = G.EntityEmbed(self.rt, ids, feats, with_bias=True)
        return FeatureList(node, len(feats)), node

    def get_batch_item_seq(self, steps, concat=False, no_attribute=False, out_scale=1.0):
        """All `steps` input placeholders ('input0'..) looked up by one launch:
        value rows are time-major [t*mb + b] (the batched form of seqModel.py:150-156)."""
        feats = self._select_feats(self.item_feats, self.item_attributes, no_attribute=no_attribute)
        return G.EntityEmbed(self.rt, self.input_all, feats, with_bias=False, concat=concat,
                             out_scale=out_scale)

    # ----------------------------------------------------------------- pools
    def _pool_embed(self, pool, output_feat):
        key = (pool, output_feat)
        if key in self._pool_nodes:
            return self._pool_nodes[key]
        if output_feat not in (0, 1):
            raise ValueError("_pool_embed serves output_feat 0 / 1; 2 / 3 pool in score space (_pooled_prediction)")
        rt = self.rt
        ia = self.item_attributes
        if pool == 'sampled':
            if self.n_sampled is None:
                raise ValueError("sampled pool requested but n_sampled is None")
            ids = self.i_indices['sampled_pass']
            feats = self._select_feats(self.item_out_feats, ia, no_attribute=(output_feat == 0))
        elif pool == 'full':
            # logit-ordered copies (embed_attribute.py:100-108 / preprocess.py:240-326)
            V = self.logit_size
            ids = G.IdsInput(rt, V, 'full_pool_ids')
            ids.value.copy_(torch.arange(V, dtype=torch.int32, device=rt.device))
            feats = []
            ncat = ia.num_features_cat if output_feat else 1
            nmul = ia.num_features_mulhot if output_feat else 0
            for i in range(ncat):
                if len(ia.full_cat_tr) > i:
                    cmap = rt.upload(_np_i32(ia.full_cat_tr[i]), torch.int32)
                else:
                    cmap = rt.upload(_np_i32(ia.features_cat[i])[_np_i32(self.logit_ind2item_ind)], torch.int32)
                feats.append(G.Feature('cat', self.item_out_feats[i].table, (cmap,)))
            for i in range(nmul):
                lens = np.asarray(ia.full_lengths_tr[i], dtype=np.float64).reshape(-1).astype(np.int32)
                starts = np.zeros(V, dtype=np.int32)
                starts[1:] = np.cumsum(lens)[:-1]
                f = self.item_out_feats[ia.num_features_cat + i]
                feats.append(G.Feature('mulhot', f.table,
                                       (rt.upload(_np_i32(ia.full_values_tr[i]), torch.int32),
                                        rt.upload(starts, torch.int32), rt.upload(lens, torch.int32)),
                                       max_len=int(lens.max())))
        else:
            raise ValueError("pool must be 'full' or 'sampled'")
        node = G.EntityEmbed(rt, ids, feats, with_bias=True)
        self._pool_nodes[key] = node
        return node

    def get_prediction(self, latent, pool='full', device='/gpu:0', output_feat=1, pred_cls=None, steps=None):
        """embed_attribute.py:148-206 -> logits [rows(latent), V or n_sampled].
        output_feat 0 / 1: embedding-space scorer (pool rows averaged first, one GEMM);
        2 / 3: the multi-hot features pool their per-token SCORES (max / log-sum-exp, :194-200).
        pred_cls: scorer node class (SeqModel passes its per-time-step variant); steps = (L, mb): the
        latent's rows are L unrolled steps -- the reference calls get_prediction once per step
        (seqModel.py:480-493), so output_feat 3 takes ONE reduce_max per step (:197)."""
        mk = pred_cls or (lambda lat, pe: G.Prediction(self.rt, lat, pe))
        if isinstance(latent, list):          # one latent per output feature (:169, :178)
            if output_feat not in (1, 2, 3):
                raise NotImplementedError('Error: Attribute combination not implemented!')
            return self._pooled_prediction(latent, pool, output_feat, mk, steps)
        if output_feat in (0, 1):
            return mk(latent, self._pool_embed(pool, output_feat))
        if output_feat not in (2, 3):
            raise NotImplementedError('Error: Attribute combination not implemented!')    # :202
        return self._pooled_prediction(latent, pool, output_feat, mk, steps)

    def _pool_ids_and_maps(self, pool):
        """(ids node, per-feature maps in pool order, W): the sampled placeholder with the item
        maps, or 0..V-1 with the logit-ordered copies (embed_attribute.py:100-108)."""
        rt, ia = self.rt, self.item_attributes
        key = ('ids', pool)
        if key in self._pool_nodes:
            return self._pool_nodes[key]
        if pool == 'sampled':
            ids = self.i_indices['sampled_pass']
            feats = self._select_feats(self.item_out_feats, ia)
            res = (ids, [(f.kind, f.table, f.maps, f.max_len) for f in feats], ids.shape[0], False)
        else:
            V = self.logit_size
            full = self._pool_embed('full', 1)             # builds the logit-ordered maps once
            res = (full.inputs[0], [(f.kind, f.table, f.maps, f.max_len) for f in full.feats], V, True)
        self._pool_nodes[key] = res
        return res

    def _pooled_prediction(self, latent, pool, output_feat, mk, steps=None):
        """logits = mean over output features of: the plain score for a categorical feature, the
        pooled token scores of a multi-hot one."""
        rt = self.rt
        ids, fmaps, W, static = self._pool_ids_and_maps(pool)
        if isinstance(latent, list) and len(latent) < len(fmaps):
            raise ValueError("latent list shorter than the number of output features")
        lat_all = latent
        parts = []
        for k, (kind, table, maps, max_len) in enumerate(fmaps):
            latent = lat_all[k] if isinstance(lat_all, list) else lat_all
            if kind == 'cat' or output_feat == 1:      # plain score / mean over the bag (embedding space)
                pe = G.EntityEmbed(rt, ids, [G.Feature(kind, table, maps, max_len)], with_bias=True)
                parts.append(mk(latent, pe))
                continue
            if static:
                cap = int(maps[2].sum().item())
            else:
                cap = W * max_len
            cap = (cap + 3) // 4 * 4
            bag = G.BagTokens(rt, ids, maps, cap, static=static)
            tokf = G.Feature('cat', table, (None,))
            tokf._inj = False                   # bag tokens repeat: shared table rows (clip norm)
            te = G.EntityEmbed(rt, bag, [tokf], with_bias=True)
            scores = mk(latent, te)
            gmax = None
            if output_feat == 3:
                if type(scores) is not G.Prediction and steps is None:
                    raise ValueError("output_feat 3 under a per-time-step scorer needs steps = (L, mb)")
                gmax = G.GlobalMax(rt, latent, table, steps=steps)
                vf = G.Feature('cat', table, (None,))
                vf._inj = gmax.L == 1           # (the steps' arg-max rows may coincide)
                gmax.vstar = G.EntityEmbed(rt, G._IdsOf(rt, gmax, gmax.vrows, 'gmax_row'), [vf], with_bias=True)
                # clip_by_global_norm (seqModel.py:180): the residual rows are part of the steps' dense matmul
                # gradients of `table`, not a lookup of their own (SeqModel._clip_hook)
                gmax.vstar._is_gmax_vstar = True
                te._gmax = gmax
                for pnode in parts + [scores]:          # its backward must follow every scorer's
                    pnode.extra_inputs = tuple(getattr(pnode, 'extra_inputs', ())) + (gmax,)
            parts.append(G.SegmentPool(rt, scores, bag, W, output_feat, gmax))
        return parts[0] if len(parts) == 1 else G.MeanOf(rt, parts)

    def get_target_score(self, latent, inds, device='/gpu:0'):
        """embed_attribute.py:208-220; `inds` is an item-index placeholder."""
        feats = self._select_feats(self.item_out_feats, self.item_attributes)
        te = G.EntityEmbed(self.rt, inds, feats, with_bias=True)
        return G.TargetScore(self.rt, latent, te)

    def update_sampled_pool(self, item_sampled):
        """embed_attribute.py:320-348 update_sampled: stage the negative pool.  The
        packed token ids / segment ids the reference materialises are produced on
        the fly by the fused gather kernel; what persists is the id list and the
        item -> slot map (the device twin of item_sampled_id2idx)."""
        buf = self.i_indices['sampled_pass']
        if self._old_pool is not None:
            ops.slot_map_set(self.item2slot, buf.value, clear=True)     # buf still holds the previous pool
        self._old_pool = True
        buf.feed(item_sampled)
        self.rt.flush_feeds()
        ops.slot_map_set(self.item2slot, buf.value, clear=False)

    # ------------------------------------------------------------------ loss
    def _mask_state(self, loss, rows):
        if loss not in self.mask:
            W = self.n_sampled if loss in ('mw', 'mce') else self.logit_size       # :652
            if loss in ('mw', 'mce'):
                getter = lambda: self.item2slot
            else:
                getter = lambda: self._item2logit_dev
            self.mask[loss] = G.MaskState(self.rt, self.batch_size, W, self.u_indices['input'], getter,
                                          lambda: self._pos_dev[self._pos_mode])
        return self.mask[loss]

    def compute_loss(self, logits, item_target, loss='ce', true_rank=False, loss_func='log',
                     exp_p=1.005, device='/gpu:0'):
        """embed_attribute.py:525-549.  Implemented on device: 'ce', 'warp', 'mw', 'warp_eval',
        'rs', 'rs-sig', 'rs-sig2', 'bbpr' (loss_func log/exp/poly/poly2/linear/square), and 'mce'
        -- accepted by the reference's assert (:527) but without a branch there: BUILD-DEFINED as
        the sampled softmax log(1 + sum_s m_rs exp(x_rs - t_r)) in the shape of 'mw' (arx.h).
        'bpr' / 'bpr-hinge' (:541-544): `logits` is the NegPos handle of the pair (neg_pos of
        hmf_model.py:106); item_target is not used, as in the reference."""
        if loss not in ['ce', 'mce', 'warp', 'warp_eval', 'rs', 'rs-sig', 'rs-sig2', 'mw', 'bbpr',
                        'bpr', 'bpr-hinge']:
            raise ValueError("unknown loss %r" % loss)
        if loss in ('bpr', 'bpr-hinge'):
            if not isinstance(logits, NegPos):
                raise ValueError("compute_loss(%r): the first argument is the NegPos handle of the pair" % loss)
            return G.PairLoss(self.rt, loss, logits.latent, logits.pos_embed, logits.neg_embed)
        if loss in ('ce',):
            return G.BatchLoss(self.rt, 'ce', logits, item_target)
        if loss in ('warp', 'mw', 'mce', 'warp_eval'):
            ms = self._mask_state(loss, logits.shape[0])
            node = G.BatchLoss(self.rt, loss, logits, item_target, mask=ms, mask_rows=self.batch_size)
            if loss == 'warp_eval':
                return [node, node]
            return node
        if loss in ('rs', 'rs-sig', 'rs-sig2', 'bbpr'):                   # :532-547, :551-603
            ms = self._mask_state(loss, logits.shape[0])
            return G.BatchLoss(self.rt, loss, logits, item_target, mask=ms, mask_rows=self.batch_size,
                               loss_func=loss_func, exp_p=exp_p)
        raise NotImplementedError('Error: not implemented other loss!!')   # :548

    def sampled_eval_loss(self, loss, latent, logits, item_target, rows, mask_rows, pool=None, masked=True):
        """The dev loss of a model that trains with the sampled `loss` ('mw' / 'mce'): EVAL_LOSS_OF[loss] over the
        full vocabulary -- streamed from `latent` and `pool` (the full pool's embedding node; None: the output
        features cannot stream) where the [rows, V] `logits` are too big, on the logits otherwise.  'warp' masks
        the user's positives (mask rows repeat every mask_rows) unless masked is False; 'ce' never takes a mask."""
        kind = EVAL_LOSS_OF[loss]
        ms = self._mask_state('warp', rows) if kind == 'warp' and masked else None
        if pool is not None and logits_too_big(rows, self.logit_size):
            return G.StreamEvalLoss(self.rt, kind, latent, pool, item_target, mask=ms, mask_rows=mask_rows)
        if kind == 'warp' and not masked:
            return G.BatchLoss(self.rt, 'warp', logits, item_target, mask=None, mask_rows=mask_rows)
        return self.compute_loss(logits, item_target, kind)

    def eval_masks(self, loss, batch_loss):
        """The mask list of the plan that evaluates `batch_loss`, the dev loss of a `loss` model (a streamed loss
        reads the positives CSR itself)."""
        kind = EVAL_LOSS_OF.get(loss, loss)
        if isinstance(batch_loss, G.StreamEvalLoss) or kind not in self.mask:
            return []
        return [self.mask[kind]]

    def get_warp_mask(self, device='/gpu:0'):
        """embed_attribute.py:662-672 -> (set_mask, reset_mask) callables per loss."""
        self.set_mask, self.reset_mask = {}, {}
        for loss, ms in self.mask.items():
            self.set_mask[loss] = (lambda m=ms: m.scatter(0))
            self.reset_mask[loss] = (lambda m=ms: m.scatter(1))
        return self.set_mask, self.reset_mask

    def prepare_warp(self, pos_item_set, pos_item_set_eval):
        """embed_attribute.py:674-677.  Accepts the reference's {user: [items]}
        dicts or prebuilt CSR pairs (ptr[n_users+1], items) for large synthetic sets."""
        self.pos_item_set = pos_item_set
        self.pos_item_set_eval = pos_item_set_eval
        self._pos_dev = {'train': self._pos_csr(pos_item_set), 'eval': self._pos_csr(pos_item_set_eval)}
        self._pos_mode = 'train'

    def _pos_csr(self, pos):
        rt = self.rt
        nu = self.n_users + 1
        if pos is None:
            ptr = np.zeros(nu + 1, dtype=np.int32)
            items = np.zeros(1, dtype=np.int32)
        elif isinstance(pos, tuple):
            ptr, items = _np_i32(pos[0]), _np_i32(pos[1])
            if len(ptr) < nu + 1:
                ptr = np.concatenate([ptr, np.full(nu + 1 - len(ptr), ptr[-1], dtype=np.int32)])
        else:
            counts = np.zeros(nu, dtype=np.int64)
            for u, its in pos.items():
                if 0 <= u < nu:
                    counts[u] = len(its)
            ptr = np.zeros(nu + 1, dtype=np.int32)
            ptr[1:] = np.cumsum(counts)
            items = np.zeros(max(1, int(ptr[-1])), dtype=np.int32)
            for u, its in pos.items():
                if 0 <= u < nu and len(its):
                    items[ptr[u]:ptr[u + 1]] = np.asarray(list(its), dtype=np.int32)
        if len(items) == 0:
            items = np.zeros(1, dtype=np.int32)
        return rt.upload(ptr, torch.int32), rt.upload(items, torch.int32)

    def prepare_recommend_exclusions(self, item_sets):
        """Items each user must NOT be recommended (typically the training history): {user_index: items} dicts or a
        (ptr, items) CSR pair in item-index space.  Mapped to logit columns through item_ind2logit_ind, sorted,
        deduplicated and uploaded once; recommend(exclude_seen=True) reads them (exclusion_args)."""
        if self._item2logit_np is None:
            raise ValueError("recommend exclusions need item_ind2logit_ind")
        ptr, cols = exclusion_csr(item_sets, self.n_users + 1, self._item2logit_np)   # users 0..n_users (_pos_csr)
        self._ex_host = (ptr, cols)        # (the striped model re-expresses them per shard: arx.dist.SeqHybridParallel)
        self._ex_dev = (self.rt.upload(ptr, torch.int32), self.rt.upload(cols, torch.int32))

    def exclusion_args(self):
        """(row_keys, key_rows, ex_ptr, ex_cols) of the recommend rows: row r excludes the list of user
        user_input[r % batch_size] (ops.topk_exclude_fill, ops.gemm_nt_topk_filter_excl)."""
        ex = getattr(self, '_ex_dev', None)
        if ex is None:
            raise ValueError("exclude_seen=True needs prepare_recommend_exclusions() first")
        return (self.u_indices['input'].value, self.batch_size, ex[0], ex[1])

    def prepare_item_tags(self, tags):
        """The items' tag words for recommend(tags_any=, tags_all=): an integer array [n_items] of 32-bit words, or
        {item_index: bit numbers 0..31} (item_tag_words).  Mapped to logit columns through item_ind2logit_ind and
        uploaded once as int32 bit patterns [V]; a second call replaces the words in place."""
        if self._item2logit_np is None:
            raise ValueError("item tags need item_ind2logit_ind")
        words = item_tag_words(tags, self._item2logit_np, self.logit_size)
        dev = getattr(self, '_tags_dev', None)
        if dev is None:
            # the per-row request words are placeholders, fed per call: a captured plan replays with new words
            self._tags_any = G.IdsInput(self.rt, self.batch_size, 'tags_any')
            self._tags_all = G.IdsInput(self.rt, self.batch_size, 'tags_all')
            self._tags_dev = self.rt.upload(words, torch.int32)
        else:
            dev.copy_(torch.from_numpy(words))

    def tag_args(self):
        """(col_tags, want_any, want_all, want_rows) of the recommend rows: row r is eligible by the words
        [r % batch_size] of the two placeholders (ops.topk_tags_fill, ops.gemm_nt_topk_filter_tags)."""
        dev = getattr(self, '_tags_dev', None)
        if dev is None:
            raise ValueError("tags_any / tags_all need prepare_item_tags() first")
        return (dev, self._tags_any.value, self._tags_all.value, self.batch_size)

    def feed_tag_words(self, tags_any, tags_all, what='recommend'):
        """Check and feed the request words of one recommend call (topk.tag_words: ValueError before any feed)."""
        self.tag_args()
        wa, wl = tag_words(tags_any, tags_all, self.batch_size, what)
        self._tags_any.feed(wa)
        self._tags_all.feed(wl)

    def sample_args(self):
        """(tau, tau_rows, seed_words) of the sampled recommend: row r draws at temperature [r % batch_size] of the
        placeholder and with the noise row r % batch_size (ops.topk_gumbel_add, ops.gemm_nt_topk_filter_sample).  The
        placeholders are made at first use and fed per call: a captured plan replays with a new temperature and seed."""
        if getattr(self, '_sample_tau', None) is None:
            self._sample_tau = G.FloatInput(self.rt, (self.batch_size,), 'sample_tau')
            self._sample_seed = G.IdsInput(self.rt, 2, 'sample_seed')
        return (self._sample_tau.value, self.batch_size, self._sample_seed.value)

    sample_draws = 0                 # sampled calls that took their seed from this counter (sample_seed=None)

    def next_sample_seed(self, temperature, seed):
        """The seed of one sampled call: an int as given (the counter stays), None: the draw counter, which starts at 0
        and goes up by one -- after the checks of topk.sample_params: a refused call does not move it."""
        sample_params(temperature, 0 if seed is None else seed, self.batch_size)
        if seed is not None:
            return seed
        seed, self.sample_draws = self.sample_draws, self.sample_draws + 1
        return seed

    def feed_sample(self, temperature, seed):
        """Check and feed the temperatures and the seed of one sampled recommend call (topk.sample_params: ValueError
        before any feed)."""
        tau, words = sample_params(temperature, self.next_sample_seed(temperature, seed), self.batch_size)
        self.sample_args()
        self._sample_tau.feed(tau)
        self._sample_seed.feed(words)

    def similar_items(self, logit_ids, k, include_self=False, return_values=False, chunk=65536, output_feat=1,
                      return_logprob=False, scan_dtype=None):
        """(return_logprob=True: NotImplementedError -- nothing is drawn here; scan_dtype='bf16': NotImplementedError --
        the bf16 filter scan of recommend has no cosine form.)
        Cosine nearest neighbours of items over the full vocabulary, in the latent space recommend scores against:
        the rows of _pool_embed('full', output_feat) -- the id row of an id-only model, the mean of the id row and the
        attribute bags for HET / MIX items; the bias plays no part.  logit_ids: the items asked about, logit indices in
        [0, V) (recommend's output space), at least one; 1 <= k <= min(1024, V).  Returns int32 [len(ids), k] logit
        indices on the device ordered by (cosine desc, index asc), and their float32 cosines with return_values;
        include_self False leaves the query itself out; (-1, -inf) where fewer than k items are left (k = V without
        the query).  An all-zero latent has cosine 0 with every item, also as a query.
        Eager, on the runtime's stream: the pool rows are looked up again from the current tables, the inverse norms
        recomputed (topk.similar_scan); buffers are this method's own, cached per (len(ids), k).  chunk: the width of
        TopKScan's first chunk.  output_feat 2 / 3 score each token of a bag: there is no item latent to compare."""
        no_return_logprob("similar_items", return_logprob)
        no_scan_dtype("similar_items", scan_dtype)
        if output_feat not in (0, 1):
            raise NotImplementedError("similar_items: output_feat 2 / 3 pool the token SCORES of an item -- there is "
                                      "no item latent pool to take cosines in")
        V = self.logit_size
        ids = logit_ids.cpu().numpy() if isinstance(logit_ids, torch.Tensor) else np.asarray(logit_ids)
        ids = ids.astype(np.int64).reshape(-1)
        k = int(k)
        if not 1 <= k <= min(1024, V):
            raise ValueError("similar_items: need 1 <= k <= min(1024, %d)" % V)
        if len(ids) < 1:
            raise ValueError("similar_items: need at least one query id")
        if ids.min() < 0 or ids.max() >= V:
            raise ValueError("similar_items: query ids must be logit indices in [0, %d)" % V)
        node = self._pool_embed('full', output_feat)
        node.forward(False)                                 # (the lookup a recommend plan runs: same rows, same buffer)
        table = node.value
        B, dev = len(ids), self.rt.device
        cache = getattr(self, '_similar', None)
        if cache is None:
            cache = self._similar = {}
        key = (B, k, int(chunk), output_feat)
        st = cache.get(key)
        if st is None:
            if len(cache) > 8:
                cache.clear()
            st = cache[key] = (TopKScan(B, V, int(table.shape[1]), k, dev, chunk=chunk),
                               torch.empty(B, dtype=torch.int32, device=dev),
                               torch.empty((B, k), dtype=torch.float32, device=dev),
                               torch.empty((B, k), dtype=torch.int32, device=dev))
            if getattr(self, '_similar_ws', None) is None:
                self._similar_ws = ops.Workspace(dev)
        scan, rows, vals, idx = st
        rows.copy_(torch.from_numpy(ids.astype(np.int32)))
        similar_scan(scan, table, rows, vals, idx, self._similar_ws, include_self)
        return (idx.clone(), vals.clone()) if return_values else idx.clone()

    def check_hardest_of(self, hardest_of):
        """The refusals of prepare_pair_negatives(hardest_of=), raised before anything is uploaded or dropped:
        ValueError unless None or an int in [2, 64]; NotImplementedError where the candidates cannot be scored from
        one table row per side (arx_neg_draw_hardest)."""
        if hardest_of is None:
            return
        if isinstance(hardest_of, bool) or not isinstance(hardest_of, (int, np.integer)) \
                or not 2 <= int(hardest_of) <= 64:
            raise ValueError("prepare_pair_negatives: hardest_of is None or an int in [2, 64], got %r" % (hardest_of,))
        for side, feats in (('user', self.user_feats), ('item', self.item_feats)):
            if len(feats) != 1 or feats[0].kind != 'cat':
                raise NotImplementedError(
                    "prepare_pair_negatives(hardest_of=): the %s side must be exactly one one-hot feature (it has %s); "
                    "multi-hot and multi-feature %ss have no single table row to score a candidate against"
                    % (side, ', '.join(f.kind for f in feats) or 'none', side))

    def prepare_pair_negatives(self, hist, seed=0, power=None, smooth=1.0, counts=None, hardest_of=None):
        """The items a drawn negative of the pair losses must not hit, per user -- typically the training history:
        {user_index: items} or a (ptr, items) CSR pair in item-index space (the forms of
        prepare_recommend_exclusions).  Uploaded as sorted logit columns together with logit_ind2item_ind; steps
        without neg_item_input then draw their negatives on the device (graph.NegPairDraw).  BUILD-DEFINED: the
        reference's draw is a commented-out host rejection loop (hmf_model.py:263-274).
        power None: uniform over the user's other columns (arx_neg_draw_uniform).  A number: in proportion to
        (counts + smooth) ** power (arx_neg_draw_weighted; 0.75 is the unigram rule of word2vec) -- counts per ITEM
        index, by default the number of users whose list holds the item; an item with counts + smooth == 0 is never
        drawn.  The two int64 tables of that draw (prepare_train.pair_draw_tables) are built here, once.
        hardest_of None: one draw per row.  An int C in [2, 64]: dynamic negative sampling -- a TRAINING step draws C
        candidates by the rule above (the plain draws at C consecutive counters), scores each against the row's user
        with the current tables and trains against the one the model ranks highest, all in one launch inside the
        captured step (arx_neg_draw_hardest; ties go to the earlier candidate, a NaN score never wins).  A
        forward_only step keeps the plain single draw: dev loss and auc stay comparable with a run without hard
        negatives.  The scores use the user's table row as it is, WITHOUT dropout, whatever the model's dropout.
        Needs exactly one one-hot feature on the user side and on the item side (NotImplementedError otherwise;
        ValueError for any other hardest_of) -- both are raised before anything is uploaded, and an earlier prepare
        stays in force.  col2row, the table row of every logit column, is built here, once.
        A second call replaces the lists, the tables, the seed and the hard mode."""
        self.check_hardest_of(hardest_of)
        if self._item2logit_np is None or self.logit_ind2item_ind is None:
            raise ValueError("pair negatives need item_ind2logit_ind and logit_ind2item_ind")
        ptr, cols = exclusion_csr(hist, self.n_users + 1, self._item2logit_np)      # users 0..n_users (_pos_csr)
        rt = self.rt
        l2i = _np_i32(self.logit_ind2item_ind)
        tables = (None, None)
        if power is not None:
            V = self.logit_size
            if counts is None:
                col_counts = np.bincount(cols[:ptr[-1]], minlength=V)[:V]          # (the lists are deduplicated)
            else:
                counts = np.asarray(counts).reshape(-1)
                if len(l2i) and (l2i.min() < 0 or l2i.max() >= len(counts)):
                    raise ValueError("prepare_pair_negatives: counts holds one entry per item index")
                col_counts = counts[l2i[:V]]
            cum, ex_cum = pair_draw_tables(col_counts, power, smooth, ptr, cols)
            tables = (rt.upload(ex_cum, torch.int64), rt.upload(cum, torch.int64))
        self._pair_lists = (rt.upload(ptr, torch.int32), rt.upload(cols, torch.int32),
                            rt.upload(l2i, torch.int32)) + tables
        if getattr(self, 'neg_draw', None) is None:
            self.neg_draw = G.NegPairDraw(rt, self.u_indices['input'], self.i_indices['neg'],
                                          lambda: self._pair_lists, self.logit_size, seed)
        self.neg_draw.seed = int(seed)
        self.neg_draw.hard = None
        if hardest_of is not None:
            C = int(hardest_of)
            ut, it = self.user_feats[0].table, self.item_feats[0].table
            umap = self.user_feats[0].maps[0]
            col2row = rt.upload(_np_i32(self.item_attributes.features_cat[0])[l2i[:self.logit_size]], torch.int32)
            self.neg_draw.hard = lambda: (C, ut.E, umap, it.E, it.bias, col2row)

    def set_pos_mode(self, forward_only):
        self._pos_mode = 'eval' if forward_only else 'train'      # :727

    # ----------------------------------------------------------------- feeds
    def target_mapping(self, item_target):
        """embed_attribute.py:679-684: item index -> logit index (host lists)."""
        m = self._item2logit_np
        out = []
        for items in item_target:
            a = np.asarray(items, dtype=np.int64)
            r = m[a]
            if (r < 0).any():
                raise KeyError(int(a[np.argmax(r < 0)]))
            out.append(r.tolist())
        return out

    def target_mapping_device(self, item_ids_dev, out_dev):
        """device twin of target_mapping: out[i] = item_ind2logit_ind[item[i]]."""
        self.rt.flush_feeds()
        ops.sparse_site_onehot(self._item2logit_dev, item_ids_dev, 0, 0.0, out_dev, None, None)
        return out_dev

    def add_input(self, input_feed, user_input, item_input, neg_item_input=None, item_sampled=None,
                  item_sampled_id2idx=None, forward_only=False, recommend=False, loss=None):
        """embed_attribute.py:697-747.  Feeds the placeholders directly (input_feed is
        kept for signature compatibility) and returns the reference's triple; the
        positive-mask index list the reference builds on the host (:721-745) is
        produced on device from the positives CSR, so input_feed_warp is empty."""
        if self.user_attributes is not None:
            self.u_indices['input'].feed(user_input)
        if self.item_attributes is not None and self.input_steps > 0 and item_input is not None:
            if isinstance(item_input, torch.Tensor):
                self.input_all.feed(item_input.reshape(-1))
            else:
                arr = np.asarray(item_input, dtype=np.int32)      # [steps][mb] time-major
                if arr.shape[0] < self.input_steps:
                    pad = np.zeros((self.input_steps - arr.shape[0], arr.shape[1]), dtype=np.int32)
                    arr = np.concatenate([arr, pad], 0)
                self.input_all.feed(arr.reshape(-1))
        if self.item_attributes is not None and loss in ['bpr', 'bpr-hinge'] and recommend is False:   # :704-706
            self.i_indices['pos'].feed(item_input)
            if neg_item_input is not None:           # (None: the plan draws them, prepare_pair_negatives)
                self.i_indices['neg'].feed(neg_item_input)
        update_sampled = []
        input_feed_sampled = {}
        if (self.item_attributes is not None and recommend is False and item_sampled is not None
                and loss in ['mw', 'mce']):
            input_feed_sampled['item_sampled_ind'] = item_sampled
            update_sampled = [lambda: self.update_sampled_pool(item_sampled)]
        self.set_pos_mode(forward_only)
        return update_sampled, input_feed_sampled, {}

    # ------------------------------------------------------------------ sizes
    def get_user_model_size(self, no_id=False, concat=True):
        ua = self.user_attributes
        if concat:
            s = 1 if no_id else 0
            return (sum(ua._embedding_size_list_cat[s:ua.num_features_cat]) +
                    sum(ua._embedding_size_list_mulhot[0:ua.num_features_mulhot]))
        return ua._embedding_size_list_cat[0]

    def get_item_model_size(self, concat=True):
        ia = self.item_attributes
        if concat:
            return (sum(ia._embedding_size_list_cat[0:ia.num_features_cat]) +
                    sum(ia._embedding_size_list_mulhot[0:ia.num_features_mulhot]))
        return ia._embedding_size_list_cat[0]


class NegPos(object):
    """neg_pos = neg_score - pos_score of hmf_model.py:104-106 as the reference hands it to compute_loss: here the
    three operands (user latent, 'pos' lookup, 'neg' lookup) -- the loss kernel forms the scores itself."""

    def __init__(self, latent, pos_embed, neg_embed):
        self.latent, self.pos_embed, self.neg_embed = latent, pos_embed, neg_embed
        self.shape = (latent.shape[0],)


def reduce_mean(x, axis=0):
    """tf.reduce_mean over a feature list (hmf_model.py:97, seqModel.py:154)."""
    if isinstance(x, FeatureList):
        return x.mean_node
    raise NotImplementedError("reduce_mean over %r" % type(x))
