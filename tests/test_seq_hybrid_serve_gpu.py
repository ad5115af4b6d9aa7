"""Serving side of the row-striped sequence model (arx.dist.SeqHybridParallel): full-vocabulary recommend
(model.step_recommend, with and without exclude_seen) and the dev loss (model.step(..., forward_only=True)) of `world`
ranks, each fed 1/world of the sequences, against the single-process oracle (oracle.ref_lstm.RefSeqModel) on the
GLOBAL batch -- after two training steps with rows touched from several ranks, on ragged stripes (301 users, 503
items) and on a logit vocabulary smaller than the item table (400 logits: out-of-vocabulary rows on every shard).
A training step after serving still matches the oracle, and serving leaves the training exchange state (_fetch /
_hstate) alone.  World 1 also equals a plain single-process SeqModel.  The ranks are processes sharing the one GPU of
the test box and exchange over gloo (host-staged), as in tests/test_seq_hybrid_gpu.py.
Reference: lstm/run.py:505-519,550-640, lstm/seqModel.py:326-353,510,514-517."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {'id': dict(n_users=301, n_items=503, logit_size=503),       # (odd sizes: ragged last stripes)
        'oov': dict(n_users=301, n_items=503, logit_size=400)}      # (103 items without a logit)
SIZE, B_LOC, L, S, K = 64, 16, 4, 128, 7
# per case, a seed at which the oracle's top K + 1 scores of every row, with and without the exclusions, are at least
# 5e-4 apart (found by running the oracle alone; _assert_no_near_tie re-checks it in every run)
SEEDS = {(1, 'mw', 'oov'): 4, (2, 'mw', 'id'): 4, (2, 'mce', 'oov'): 6, (3, 'mw', 'oov'): 6, (3, 'mce', 'id'): 8}
GAP = 1e-4           # the oracle's own adjacent scores among ranks 1..K+1 must differ by more than this (relative)


def _ranking(ref, users, inp, positions, V):
    """The oracle's full ranking per row: (logit ids [V], probabilities [V]), tf.nn.top_k's order."""
    full = ref.step_recommend(list(users), inp.tolist(), positions, topk_n=V)
    return [(np.asarray(i, dtype=np.int64), np.asarray(v, dtype=np.float64)) for _, v, i in full]


def _assert_no_near_tie(vals, what):
    v = np.asarray(vals, dtype=np.float64)
    if len(v) > 1:
        gap = (v[:-1] - v[1:]) / v[:-1]
        assert (gap > GAP).all(), "%s: the oracle's adjacent scores are nearly tied (%g): pick another seed" % (
            what, gap.min())


def _exclusion_sets(syn, users, rng):
    """{user index: items}: ~60 random items per user of the batch; the first user keeps only 3 in-vocabulary items."""
    sets = {int(u): rng.integers(0, syn.n_items, size=60).tolist() for u in users}
    in_vocab = np.nonzero(syn.in_logits)[0]
    keep = set(rng.choice(in_vocab, size=3, replace=False).tolist())
    sets[int(users[0])] = [i for i in range(syn.n_items) if i not in keep]
    return sets


def _excluded_expectation(syn, sets, users, ranking):
    out = []
    for u, (idx, pr) in zip(users, ranking):
        gone = {int(syn.item2logit[i]) for i in sets[int(u)] if syn.item2logit[i] >= 0}
        keep = np.asarray([j not in gone for j in idx.tolist()], dtype=bool)
        ii, pp = idx[keep][:K + 1], pr[keep][:K + 1]
        _assert_no_near_tie(pp, 'exclude_seen, user %d' % int(u))
        e_i, e_p = np.full(K, -1, dtype=np.int64), np.zeros(K)
        n = min(K, len(ii))
        e_i[:n], e_p[:n] = ii[:n], pp[:n]
        out.append((e_i, e_p))
    return out


def _check_recommend(got, users, expect, what):
    from test_lstm_gpu import RTOL
    assert len(got) == len(users) == len(expect)
    for (u0, v0, i0), u1, (i1, v1) in zip(got, users, expect):
        assert int(u0) == int(u1), what
        np.testing.assert_array_equal(np.asarray(i0), i1, err_msg=what)
        np.testing.assert_allclose(v0, v1, rtol=RTOL, atol=1e-9, err_msg=what)


def _worker(rank, world, port, out_dir, loss, cfg_name):
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from arx.dist import SeqHybridParallel
    from test_lstm_gpu import _build, _batch, RTOL

    cfg, seed = CFGS[cfg_name], SEEDS[(world, loss, cfg_name)]
    B = B_LOC * world
    syn, emb, model, _, _ = _build(cfg, loss, SIZE, B_LOC, L, S, 5.0, seed=seed)
    _, _, _, remb, ref = _build(cfg, loss, SIZE, B, L, S, 5.0, seed=seed)          # the oracle: global batch
    plain = _build(cfg, loss, SIZE, B_LOC, L, S, 5.0, seed=seed)[2] if world == 1 else None
    V = syn.logit_size
    for mdl in (model, plain):
        if mdl is not None:
            mdl.topk_n = K
    dp = SeqHybridParallel(model)
    rng = np.random.default_rng(7)
    pool = syn.sample_pool(S, rng)
    id2idx = {int(v): i for i, v in enumerate(pool)}
    sl = slice(rank * B_LOC, (rank + 1) * B_LOC)

    def train_step(step, ps):
        users, inp, tg, w = _batch(syn, rng, L, B)                    # the same global batch on every rank
        if step == 1:
            tg[:, :] = tg[:, :1]                                      # every rank hits the SAME target rows
            inp[1:] = tg[:-1]
        l_ref = ref.step(list(users), inp.tolist(), tg.tolist(), w.tolist(), ps, id2idx)
        l_loc = model.step(None, list(users[sl]), inp[:, sl].tolist(), tg[:, sl].tolist(), w[:, sl].tolist(), 0,
                           ps, id2idx)
        if plain is not None:
            plain.step(None, list(users), inp.tolist(), tg.tolist(), w.tolist(), 0, ps, id2idx)
        np.testing.assert_allclose(dp.global_loss(l_loc), l_ref, rtol=RTOL, err_msg='loss step %d' % step)
        np.testing.assert_allclose(float(model._gnorm.item()), ref.last['gnorm'], rtol=RTOL,
                                   err_msg='global norm step %d' % step)

    for step in range(2):
        train_step(step, pool if step == 0 else None)
    fetch_before = {k: id(v) for k, v in dp._fetch.items()}
    hstate_before = {k: id(v) for k, v in dp._hstate.items()}

    # ---- recommend -------------------------------------------------------------------------------------
    users, inp, tg, w = _batch(syn, rng, L, B)
    positions = rng.integers(0, L, size=B).tolist()
    ranking = _ranking(ref, users, inp, positions, V)
    for u, (idx, pr) in zip(users, ranking):
        _assert_no_near_tie(pr[:K + 1], 'recommend, user %d' % int(u))
    r_ref = ref.step_recommend(list(users), inp.tolist(), positions, topk_n=K)
    args = (None, list(users[sl]), inp[:, sl].tolist(), positions[sl], 0)
    got = model.step_recommend(*args)
    _check_recommend(got, users[sl], [(np.asarray(i), np.asarray(v)) for _, v, i in r_ref[sl]], 'recommend')
    if plain is not None:
        _check_recommend(got, users, [(i, v) for _, v, i in plain.step_recommend(*args)], 'recommend vs plain')

    # ---- recommend without the seen items ----------------------------------------------------------------
    with pytest.raises(ValueError):                                   # nothing prepared: before any collective
        model.step_recommend(*args, exclude_seen=True)
    sets = _exclusion_sets(syn, users, np.random.default_rng(11))
    model.prepare_recommend_exclusions(sets)
    expect = _excluded_expectation(syn, sets, users, ranking)
    assert (expect[0][0] == -1).sum() == K - 3                        # the first user: 3 items left
    got = model.step_recommend(*args, exclude_seen=True)
    _check_recommend(got, users[sl], expect[sl], 'exclude_seen')
    if rank == 0:
        assert (np.asarray(got[0][2])[3:] == -1).all() and (np.asarray(got[0][1])[3:] == 0).all()
    if plain is not None:
        plain.prepare_recommend_exclusions(sets)
        _check_recommend(got, users, [(i, v) for _, v, i in plain.step_recommend(*args, exclude_seen=True)],
                         'exclude_seen vs plain')

    # ---- dev loss -----------------------------------------------------------------------------------------
    users, inp, tg, w = _batch(syn, rng, L, B)
    assert (w == 0).any() and (w[:, sl] == 0).any()                   # sequences shorter than L
    tg_rows = np.asarray(syn.i_attr.features_cat[0])[tg.reshape(-1)]
    assert set((tg_rows % world).tolist()) == set(range(world))       # a target owned by each rank
    e_ref = ref.step(list(users), inp.tolist(), tg.tolist(), w.tolist(), forward_only=True)
    eargs = (None, list(users[sl]), inp[:, sl].tolist(), tg[:, sl].tolist(), w[:, sl].tolist(), 0)
    e_loc = model.step(*eargs, forward_only=True)
    assert np.isfinite(e_loc)
    np.testing.assert_allclose(dp.global_loss(e_loc), e_ref, rtol=RTOL, err_msg='dev loss')
    if plain is not None:
        np.testing.assert_allclose(e_loc, plain.step(*eargs, forward_only=True), rtol=RTOL, err_msg='dev loss vs plain')
    dp.EVAL_BLOCK_ROWS = 40 * world                                   # several row blocks, a ragged last one
    np.testing.assert_allclose(dp.global_loss(model.step(*eargs, forward_only=True)), e_ref, rtol=RTOL,
                               err_msg='dev loss in row blocks')

    # ---- serving left the training exchange alone; a step after it still matches ---------------------------
    assert {k: id(v) for k, v in dp._fetch.items()} == fetch_before
    assert {k: id(v) for k, v in dp._hstate.items()} == hstate_before
    train_step(2, None)
    got = dp.global_params()
    for k, v in got.items():
        np.testing.assert_allclose(v, remb.params[k], rtol=RTOL, atol=3e-6, err_msg='%s after serving' % k)
    np.testing.assert_allclose(model.W.w.cpu().numpy(), ref.W, rtol=RTOL, atol=3e-6, err_msg='lstm_w')
    for t in emb.tables.values():                                     # the padding row never moved
        assert not t.E[t.shard['zero_row']].any()
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("world,loss,cfg_name", sorted(SEEDS))
def test_seq_hybrid_serving_matches_global_oracle(dev, tmp_path, world, loss, cfg_name):
    import torch.multiprocessing as mp
    port = 29700 + (os.getpid() % 250) + world
    mp.spawn(_worker, args=(world, port, str(tmp_path), loss, cfg_name), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(world))
