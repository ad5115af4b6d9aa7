"""Which form K7 (lookup-gradient scatter + sparse Adagrad) takes in a single-GPU train plan, for the smallest
models that reach each form (arx.graph.Plan._choose_fused).  Three training steps each: the third
is a replay, so the side-branch decision of step two is in force.  Everything is read by POSITION -- plan._jobs
entries are (kind, what, key, ...), what of a 'multi' job is (group, rider), a rider is (entry, live sites, use_bias,
virtual, ...) -- so the file runs unchanged on the commit before the planner's records got names; the expected
values were taken from a run of it there.

ARX_K7_EARLY_MIN = 0 lets these small steps keep their side branch (the default keeps it off below 8192 live
contributions: a launch-bound step pays more for the second graph branch than it wins)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HET = dict(n_users=300, n_items=2000, item_mulhot=True, mulhot_vocab=250, avg_len=4, max_len=9)


def _hmf(cfg, d, B, S, seed=3):
    from arx.hmf.hmf_model import LatentProductModel
    from arx.utils.synthetic import SyntheticHMF
    syn = SyntheticHMF(seed=seed, **cfg)
    params = syn.glorot_params(d, seed=seed + 1, scale=0.5)
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind
    model = LatentProductModel(syn.n_users, syn.n_items, d, 1, B, 0.5, 1.0, syn.u_attr, syn.i_attr, i2l, l2i,
                               loss_function='mw', n_sampled=S, params=params)
    pos = syn.positives_dict()
    model.prepare_warp(pos, pos)
    rng = np.random.default_rng(11)
    pool = syn.sample_pool(S, rng)
    id2idx = {int(v): i for i, v in enumerate(pool)}
    for step in range(3):
        users, items = syn.sample_batch(B, rng)
        loss = model.step(None, list(users), list(items), None, pool if step == 0 else None, id2idx, loss='mw')
        assert np.isfinite(loss)
    return model._plan('train')


def _shape(plan):
    """[(kind, rider present, rider virtual)] of the passes of the last step, in order."""
    out = []
    for j in plan._jobs:
        rider = j[1][1] if j[0] == 'multi' else None
        out.append((j[0], rider is not None, bool(rider[3]) if rider is not None else None))
    return out


def _padded_bag_slots(plan):
    return [sum(s.cap for s in sites) for _t, sites, _b, _n in plan.tables if sites[0].kind == 'mulhot']


def test_id_only_tables_share_one_pass_on_the_rank_sort(dev, monkeypatch):
    monkeypatch.setenv('ARX_K7_EARLY_MIN', '0')
    plan = _hmf(dict(n_users=300, n_items=400), 32, 64, 128)
    assert _padded_bag_slots(plan) == []
    assert sum(s.cap for _t, sites, _b, _n in plan.tables for s in sites) == 64 + 64 + 128      # <= 8192: rank sort
    assert _shape(plan) == [('multi', False, None)]
    assert plan._n_passes == 1 and len(plan._early_jobs) == 1
    assert plan.ring_capable()


def test_het_bag_table_rides_on_its_id_table(dev, monkeypatch):
    monkeypatch.setenv('ARX_K7_EARLY_MIN', '0')
    plan = _hmf(HET, 32, 1024, 128)
    assert _padded_bag_slots(plan) == [(1024 + 128) * 9]             # 10368 > 8192
    assert _shape(plan) == [('multi', True, False)]
    assert plan._n_passes == 1 and len(plan._early_jobs) == 1
    # the id table the bags ride on comes first in the group
    group, rider = plan._jobs[0][1]
    assert group[0][1][0].ids_node is rider[1][0].ids_node and rider[0][0].E.shape[0] == 250 + 2


def test_mix_bag_table_is_a_virtual_rider_in_static_token_order(dev, monkeypatch):
    monkeypatch.setenv('ARX_K7_EARLY_MIN', '0')
    monkeypatch.delenv('ARX_K7_CSC', raising=False)
    plan = _hmf(dict(HET, item_mix=True), 32, 1024, 128)
    assert _padded_bag_slots(plan) == [(1024 + 128) * 9]
    assert _shape(plan) == [('multi', True, True)]
    assert plan._n_passes == 1 and len(plan._early_jobs) == 1
    ents = [e for k, e in plan._multi_cache.items() if 'csc' in e]
    assert ents and all(e['csc'] is not None for e in ents)          # static token order (ops.BagCSC)


def test_second_bag_table_keeps_its_own_two_stage_pass(dev, monkeypatch):
    """Users and items both have an id feature and a bag feature past the rank sort: one bag table rides on the
    fused pass (there is one rider per pass), the other cannot and takes the two-stage pass of its own."""
    monkeypatch.setenv('ARX_K7_EARLY_MIN', '0')
    plan = _hmf(dict(HET, user_mulhot=True), 32, 1280, 128)
    assert sorted(_padded_bag_slots(plan)) == [1280 * 8, (1280 + 128) * 9]
    assert _shape(plan) == [('multi', True, False), ('bags', False, None)]
    assert plan._n_passes == 2 and len(plan._early_jobs) == 2
    assert not plan.ring_capable()


def test_cbow_window_site_takes_the_general_pass_without_side_branch(dev, monkeypatch):
    monkeypatch.setenv('ARX_K7_EARLY_MIN', '0')
    from arx.utils.synthetic import SyntheticHMF
    from arx.word2vec import cbow_model
    d, B, S, n_in = 32, 32, 64, 4
    syn = SyntheticHMF(seed=21, n_users=300, n_items=500, logit_size=400)
    syn.u_attr.set_model_size(d)
    syn.i_attr.set_model_size(d)
    params = syn.glorot_params(d, seed=22, item_output=True, scale=0.5)
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind
    model = cbow_model.Model(syn.n_users, syn.n_items, d, B, 0.5, 1.0, syn.u_attr, syn.i_attr, i2l, l2i,
                             n_input_items=n_in, loss_function='mw', use_sep_item=True, top_N_items=8, n_sampled=S,
                             params=params, fuse_window=True)
    pos = syn.positives_dict()
    model.prepare_warp(pos, pos)
    rng = np.random.default_rng(9)
    pool = syn.sample_pool(S, rng)
    id2idx = {int(v): i for i, v in enumerate(pool)}
    for step in range(3):
        users, targets = syn.sample_batch(B, rng)
        ctx = np.stack([syn.sample_batch(B, rng)[1] for _ in range(n_in)], 0)
        loss = model.step(None, list(users), ctx.tolist(), list(targets), item_sampled=pool if step == 0 else None,
                          item_sampled_id2idx=id2idx)
        assert np.isfinite(loss)
    plan = model._plan('train')
    assert sum(s.kind == 'window' for _t, sites, _b, _n in plan.tables for s in sites) == 1
    # the window's table is not among the jobs (the general pass is never sorted ahead), the others share a pass
    assert _shape(plan) == [('multi', False, None)]
    assert plan._n_passes == 2
    assert plan._early_jobs == []
    assert not plan.ring_capable()
