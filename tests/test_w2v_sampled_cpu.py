"""Finite-difference check (fp64) of tests/w2v_sampled_ref.py, the yardstick of the sampled-pool losses of the
skip-gram / CBOW recommenders: one 'mw' step and one 'mce' step, skip-gram n = 1 and CBOW n = 3, ID and HET items.

The Adagrad slots give the gradient the helper applied: acc_after - acc0 = g^2 per element (TF-1.0 Adagrad, dense
and sparse alike, duplicates merged first).  |g| of a handful of touched rows of EVERY table is compared with
central differences of the helper's own training loss, so the yardstick cannot be wrong in the same way as the code
under test.  Bound: fp64 central differences at eps = 1e-6 carry eps^2 * f''' truncation (~1e-12) and 2^-53 / eps
(~1e-10) round-off; rtol 1e-5 / atol 1e-8 leave two orders of room.  ('mw' is piecewise linear: a hinge within eps
of its kink would show as a gross mismatch, not a marginal one.)  An untouched row keeps acc0 and its parameters.
"""
import numpy as np
import pytest

from w2v_sampled_ref import RefW2VSampled

CFG_ID = dict(n_users=40, n_items=60, logit_size=50, n_pos=8)
CFG_HET = dict(n_users=40, n_items=60, logit_size=60, n_pos=8, item_mulhot=True, mulhot_vocab=120, avg_len=3,
               max_len=6)
D, B, S = 8, 6, 16
EPS = 1e-6


def _setup(kind, cfg, loss, n_in, sep, seed):
    from arx.utils.synthetic import SyntheticHMF
    syn = SyntheticHMF(seed=seed, **cfg)
    syn.u_attr.set_model_size(D)
    syn.i_attr.set_model_size(D)
    params = {k: np.asarray(v, dtype=np.float64)
              for k, v in syn.glorot_params(D, seed=seed + 1, item_output=sep, scale=0.5).items()}
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind

    def make():
        ref = RefW2VSampled(kind, D, B, 0.5, syn.u_attr, syn.i_attr, i2l, l2i, S, n_input_items=n_in,
                            loss_function=loss, use_sep_item=sep, params=params, dtype=np.float64)
        pos = syn.positives_dict()
        ref.prepare_warp(pos, pos)
        return ref
    rng = np.random.default_rng(seed + 2)
    users, targets = syn.sample_batch(B, rng)
    ctx = np.stack([syn.sample_batch(B, rng)[1] for _ in range(n_in)], 0)
    ctx[0, 0] = targets[0]                                   # a context item equal to a target
    pool = syn.sample_pool(S, rng)
    for slot, item in ((0, int(targets[1])), (1, int(syn.positives_dict()[int(users[2])][0]))):
        if item in pool:
            pool[np.nonzero(pool == item)[0][0]] = pool[slot]
        pool[slot] = item                                    # the mask matters: a target and a positive in the pool
    assert len(set(pool.tolist())) == S
    return make, list(users), ctx.tolist(), list(targets), pool


@pytest.mark.parametrize("loss", ['mw', 'mce'])
@pytest.mark.parametrize("kind,n_in", [('skipgram', 1), ('cbow', 3)])
@pytest.mark.parametrize("cfg,sep", [(CFG_ID, True), (CFG_HET, False)], ids=['ID-sep', 'HET-shared'])
def test_sampled_helper_gradients_match_finite_differences(cfg, sep, kind, n_in, loss):
    make, users, ctx, targets, pool = _setup(kind, cfg, loss, n_in, sep, seed=11)
    ref = make()
    p0 = {k: v.copy() for k, v in ref.att_emb.params.items()}
    acc0 = {k: v.copy() for k, v in ref.att_emb.slots.items()}
    l_step = ref.step(users, ctx, targets, item_sampled=pool)
    probe = make()
    probe.stage_pool(pool)
    assert probe.train_loss(users, ctx, targets) == l_step       # the step reports the loss before its update
    if loss == 'mw':
        assert l_step > 0
    rng = np.random.default_rng(3)
    checked = 0
    for name, acc in ref.att_emb.slots.items():
        g2 = acc - acc0[name]
        assert np.all(g2 >= 0)
        touched = np.nonzero((g2 > 0).any(axis=1))[0]
        untouched = np.nonzero(~(g2 > 0).any(axis=1))[0]
        assert len(untouched) > 0, name
        r = untouched[0]
        np.testing.assert_array_equal(acc[r], acc0[name][r])
        np.testing.assert_array_equal(ref.att_emb.params[name][r], p0[name][r])
        if len(touched) == 0:
            continue
        for r in rng.choice(touched, size=min(4, len(touched)), replace=False):
            for c in rng.choice(acc.shape[1], size=min(2, acc.shape[1]), replace=False):
                w = probe.att_emb.params[name]
                keep = w[r, c]
                w[r, c] = keep + EPS
                lp = probe.train_loss(users, ctx, targets)
                w[r, c] = keep - EPS
                lm = probe.train_loss(users, ctx, targets)
                w[r, c] = keep
                fd = (lp - lm) / (2 * EPS)
                np.testing.assert_allclose(np.sqrt(g2[r, c]), abs(fd), rtol=1e-5, atol=1e-8,
                                           err_msg='%s[%d, %d]' % (name, r, c))
                # ... and the update moved the parameter against the gradient
                step = p0[name][r, c] - ref.att_emb.params[name][r, c]
                np.testing.assert_allclose(step, 0.5 * fd / np.sqrt(acc[r, c]), rtol=1e-5, atol=1e-8)
                checked += 1
    # every table family was reached: users, input items, output items (+ bias)
    assert checked >= 8


def test_sampled_helper_dev_loss_uses_eval_positives():
    """forward_only of an 'mw' model: the full-vocabulary 'warp' loss masked with the EVALUATION positives."""
    make, users, ctx, targets, pool = _setup('cbow', CFG_ID, 'mw', 3, True, seed=5)
    ref = make()
    m = ref.att_emb
    base = ref.step(users, ctx, targets, forward_only=True)
    logits = ref.logits_test(users, ctx)
    tg = m.target_mapping([targets])[0]
    mask = m.mask(users, 'warp', None, forward_only=True)
    want, _ = m.compute_loss(logits, tg, 'warp', mask)
    assert base == want.mean()
    ref.prepare_warp(m.pos_item_set, {})                        # no evaluation positives: nothing is masked
    assert ref.step(users, ctx, targets, forward_only=True) > base
