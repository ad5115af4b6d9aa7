"""CPU restatement of the sampled-pool losses ('mw', 'mce') for the skip-gram / CBOW recommenders -- TEST
INFRASTRUCTURE ONLY.  The reference meant this family to train on the sampled pool (skipgram_model.py:104-116,
cbow_model.py:107-119: sampled_logits, target_score, compute_loss(.., 'mw')) but never assigns batch_loss_test on
that branch, so oracle.ref_w2v has no sampled branch.  This helper assembles one from the oracle's existing
functions exactly as oracle.ref_graph.RefLatentProductModel.step does (update_sampled, get_prediction('sampled'),
get_target_score, compute_loss('mw' | 'mce') and their backwards) around RefW2VModel's input embedding.

Dev loss (forward_only): 'mw' -> the full-vocabulary 'warp' on x_test, masked with the EVALUATION positives;
'mce' -> the full softmax 'ce' on x_test.  tests/test_w2v_sampled_cpu.py checks the gradients of this helper
against finite differences of train_loss().
"""
import numpy as np

from oracle import ref_w2v
from oracle.ref_graph import Grads, RefEmbeddingAttribute


class RefW2VSampled(ref_w2v.RefW2VModel):
    def __init__(self, kind, size, batch_size, learning_rate, user_attributes, item_attributes,
                 item_ind2logit_ind, logit_ind2item_ind, n_sampled, n_input_items=1, loss_function='mw',
                 use_sep_item=True, output_feat=1, params=None, dtype=np.float64, top_N_items=100):
        assert loss_function in ('mw', 'mce')
        super().__init__(kind, size, batch_size, learning_rate, user_attributes, item_attributes,
                         item_ind2logit_ind, logit_ind2item_ind, n_input_items=n_input_items,
                         loss_function=loss_function, use_sep_item=use_sep_item, output_feat=output_feat,
                         params=params, dtype=dtype, top_N_items=top_N_items)
        self.n_sampled = n_sampled
        self.att_emb = RefEmbeddingAttribute(user_attributes, item_attributes, batch_size, n_sampled,
                                             self.n_input, use_sep_item, item_ind2logit_ind,
                                             logit_ind2item_ind, params=params, dtype=dtype)
        self.dt = self.att_emb.dt
        self._id2idx = None

    def stage_pool(self, item_sampled, item_sampled_id2idx=None):
        self.att_emb.update_sampled(item_sampled)
        self._id2idx = (item_sampled_id2idx if item_sampled_id2idx is not None
                        else {int(v): i for i, v in enumerate(item_sampled)})

    def _x(self, user_input, item_input):
        u, c_user, es, cs = self._inputs(user_input, item_input)
        n = self.n_input
        all_mean = np.mean(np.stack(es, 0), 0)
        if self.kind == 'skipgram':
            x_train, w_train = (u + es[0]) / 2, [1.0] + [0.0] * (n - 1)
        else:
            x_train, w_train = (u + all_mean) / 2, [1.0 / n] * n
        x_test = u if self.n_input_items == 0 else (u + all_mean) / 2
        return x_train, x_test, w_train, c_user, cs

    def _train_forward(self, user_input, item_input, item_output):
        m, loss = self.att_emb, self.loss_function
        x_train, _, w_train, c_user, cs = self._x(user_input, item_input)
        logits, c_pred = m.get_prediction(x_train, 'sampled', self.output_feat)
        tscore, c_t = m.get_target_score(x_train, item_output)
        mask = m.mask(user_input, loss, self._id2idx)
        bl, c_loss = m.compute_loss(logits, tscore, loss, mask)
        return bl, (c_loss, c_pred, c_t, c_user, cs, w_train)

    def train_loss(self, user_input, item_input, item_output):
        """The training loss of the staged pool at the current parameters (no update)."""
        bl, _ = self._train_forward(user_input, item_input, item_output)
        return self.dt.type(bl.mean())

    def logits_test(self, user_input, item_input):
        _, x_test, _, _, _ = self._x(user_input, item_input)
        return self.att_emb.get_prediction(x_test, 'full', self.output_feat)[0]

    def step(self, user_input, item_input, item_output=None, item_sampled=None, item_sampled_id2idx=None,
             forward_only=False, recommend=False):
        m, loss = self.att_emb, self.loss_function
        if recommend:
            logits = self.logits_test(user_input, item_input)
            return np.argsort(-logits, axis=1, kind='stable')[:, :self.top_N_items].astype(np.int32)
        if forward_only:
            targets = m.target_mapping([item_output])[0]
            logits = self.logits_test(user_input, item_input)
            if loss == 'mw':
                mask = m.mask(user_input, 'warp', None, forward_only=True)
                bl, _ = m.compute_loss(logits, targets, 'warp', mask)
            else:
                bl, _ = m.compute_loss(logits, targets, 'ce', None)
            return self.dt.type(bl.mean())
        if item_sampled is not None:
            self.stage_pool(item_sampled, item_sampled_id2idx)
        bl, (c_loss, c_pred, c_t, c_user, cs, w_train) = self._train_forward(user_input, item_input, item_output)
        mb = len(user_input)
        grads = Grads()
        d_logits, d_t = m.compute_loss_bwd(c_loss, np.full((mb,), 1.0 / mb, dtype=self.dt))
        d_x = m.get_prediction_bwd(c_pred, d_logits, grads)
        d_x = d_x + m.get_target_score_bwd(c_t, d_t, grads)
        for i in range(self.n_input):
            if w_train[i] == 0.0:
                continue
            nf = len(cs[i]['sites'])
            m.get_embedded_bwd(cs[i], [d_x * (0.5 * w_train[i] / nf)] * nf, None, grads)
        m.get_batch_user_bwd(c_user, d_x * 0.5, grads)
        m.apply_gradients(grads, self.learning_rate)
        return self.dt.type(bl.mean())
