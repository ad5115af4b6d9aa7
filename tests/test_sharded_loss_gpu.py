"""The `loss` argument of the row-sharded models on the HIP backend, 1-rank RCCL group (the path every rank runs):
arx_pair_loss_slots against fp64, 'bpr' / 'bpr-hinge' steps of ShardedHMF (captured and kernel by kernel) against BPR
on the batch in fp64, the model's own negative draw, 'mce' on all three classes against the oracle's 'mce', and
recommend over 'bpr'-trained tables."""
import os

import numpy as np
import pytest

from numpy_backend_pair import PairRef
from oracle import ref_graph as rg
from test_bpr_gpu import _pair_case, _pair_ref
from test_hmf_gpu import ATOL, RTOL

pytestmark = pytest.mark.gpu

KINDS = ('bpr', 'bpr-hinge')


def _group(dev, port):
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    return dist


# ------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,d", [(1, 32), (3, 20), (64, 64), (200, 128), (37, 256)])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("with_w", [False, True])
def test_pair_loss_slots_matches_fp64(dev, kind, B, d, acc, with_w):
    """Packed rows of d + 4 floats, the positives and negatives interleaved over a shuffled block of 2 B + 5 slots
    (the rest, the void row's unused slot and the pad columns keep a sentinel, bit for bit), acc_dU, row weights, one
    void row where B > 1 (exact zeros), forward only with null gradients, two runs bit for bit, the auc's integers."""
    import torch
    from arx import ops
    U, P, pb, N, nb, rw, dU0 = _pair_case(B, d, 5)
    void = np.zeros(B, dtype=bool)
    if B > 1:
        void[B // 2] = True
    gscale = 1.0 / B
    ref = _pair_ref(kind, U, P, pb, N, nb, void, rw if with_w else np.ones(B), gscale, dU0 if acc else 0 * dU0)
    if kind == 'bpr-hinge':
        assert np.abs(1.0 + ref['x']).min() > 1e-4        # no row near the kink: fp32 takes the same branch
    n_slots, dp = 2 * B + 5, d + 4
    perm = np.random.default_rng(B + d).permutation(n_slots)[:2 * B].astype(np.int32)
    pos_slot, neg_slot = perm[0::2].copy(), perm[1::2].copy()             # interleaved, not the identity
    R = np.full((n_slots, dp), 3.0, dtype=np.float32)
    R[pos_slot, :d], R[pos_slot, d] = P, pb
    R[neg_slot, :d], R[neg_slot, d] = N, nb
    spare = neg_slot[void]
    neg_slot[void] = -1
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Ud, Rd, psd, nsd = up(U), up(R), up(pos_slot), up(neg_slot)
    rwd = up(rw) if with_w else None
    SENT = np.float32(9.0)
    runs = []
    for _ in range(2):
        out = {k: torch.full((B,), 9.0, dtype=torch.float32, device=dev) for k in ('ps', 'ns', 'loss')}
        dU, dR = up(dU0), torch.full((n_slots, dp), float(SENT), dtype=torch.float32, device=dev)
        cnt = torch.full((2,), -5, dtype=torch.int32, device=dev)
        ops.pair_loss_slots(Ud, Rd, psd, nsd, kind, gscale, out['ps'], out['ns'], out['loss'], row_w=rwd, dU=dU,
                            acc_dU=bool(acc), dR=dR, auc_counts=cnt)
        out.update(dU=dU, dR=dR, cnt=cnt)
        runs.append({k: v.cpu().numpy().copy() for k, v in out.items()})
    got = runs[0]
    for k, v in got.items():
        np.testing.assert_array_equal(v.view(np.uint32), runs[1][k].view(np.uint32), err_msg=k + ': second run')
    live = ~void
    np.testing.assert_allclose(got['ps'], ref['ps'], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got['ns'][live], ref['ns'][live], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got['loss'], ref['loss'], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got['dU'], ref['dU'], rtol=RTOL, atol=ATOL)
    dR = got['dR']
    np.testing.assert_allclose(dR[pos_slot, :d], ref['dP'], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(dR[pos_slot, d], ref['dpb'], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(dR[neg_slot[live], :d], ref['dN'][live], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(dR[neg_slot[live], d], ref['dnb'][live], rtol=RTOL, atol=ATOL)
    # what no slot names is not written: the tail, the void row's spare slot, the pad columns of every row
    named = np.zeros(n_slots, dtype=bool)
    named[pos_slot] = True
    named[neg_slot[live]] = True
    assert not named[spare].any() and (~named).sum() == 5 + int(void.sum())
    assert (dR[~named].view(np.uint32) == SENT.view(np.uint32)).all()
    assert (dR[:, d + 1:].view(np.uint32) == SENT.view(np.uint32)).all()
    if void.any():
        r = int(np.nonzero(void)[0][0])
        assert got['loss'][r] == 0.0 and got['ns'][r] == 0.0
        assert not np.any(dR[pos_slot[r], :d + 1])                            # exact zeros
        np.testing.assert_array_equal(got['dU'][r], dU0[r] if acc else 0 * dU0[r])
    x32 = got['ns'] - got['ps']
    assert got['cnt'].tolist() == [int(np.sign(x32[live]).sum()), int(live.sum())]
    # forward only: null gradients, the same scores and loss
    f = {k: torch.full((B,), 9.0, dtype=torch.float32, device=dev) for k in ('ps', 'ns', 'loss')}
    ops.pair_loss_slots(Ud, Rd, psd, nsd, kind, gscale, f['ps'], f['ns'], f['loss'], row_w=rwd)
    for k, v in f.items():
        np.testing.assert_array_equal(v.cpu().numpy(), got[k], err_msg=k + ': forward only')


# ------------------------------------------------------------------ 2. whole steps at world 1
def _pair_batch(rng, n_users, n_items, B, void_row):
    users = rng.integers(0, n_users, size=B)
    pos, neg = rng.integers(0, n_items, size=B), rng.integers(0, n_items, size=B)
    users[1] = users[0]                              # duplicate user
    pos[2] = pos[3]                                  # an item that is a positive twice
    neg[4] = pos[5]                                  # ... and one that is a positive and a negative
    neg[6] = neg[7]
    same = neg == pos
    neg[same] = (pos[same] + 1) % n_items
    if void_row is not None:
        neg[void_row] = -1
        users[void_row] = np.setdiff1d(np.arange(n_users), users)[0]
    return users.astype(np.int32), pos.astype(np.int32), neg.astype(np.int32)


def _tables(n_users, n_items, d):
    from arx.utils.synthetic import SyntheticHMF
    syn = SyntheticHMF(n_users=n_users, n_items=n_items, seed=1, permute_logits=False, n_pos=8)
    params = syn.glorot_params(d, seed=2, scale=0.5)
    return syn, params, {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
                         'item_bias': params['item_bias_cat_0'][2:]}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_users,n_items,d,B,graphs", [
    pytest.param(300, 500, 64, 32, True, id="300-500-64-32"),
    pytest.param(300, 500, 64, 32, False, id="300-500-64-32-graphs_off"),
    pytest.param(3000, 4000, 128, 2048, True, id="3000-4000-128-2048")])     # past K7's rank-sort limits
def test_sharded_pair_steps_world1(dev, kind, n_users, n_items, d, B, graphs):
    """Six steps with fed negatives: eager, captured, then replayed on fresh batches (ONE graph; step 3 has a void
    row, so fewer requests than slots) -- loss per step, scores, auc, tables and slots at the end against fp64."""
    import torch
    from arx.dist import ShardedHMF
    dist = _group(dev, 29741)
    try:
        _, _, tables = _tables(n_users, n_items, d)
        model = ShardedHMF(n_users, n_items, d, B, 0, 0.5, 0, 1, dev, tables=tables, graphs=graphs, loss=kind)
        assert model.use_graphs == graphs and not hasattr(model, 'logits') and not hasattr(model, 'item2slot')
        ref = PairRef(tables, 0.5)
        rng = np.random.default_rng(11)
        for step in range(6):
            void_row = 9 if step == 3 else None
            users, pos, neg = _pair_batch(rng, n_users, n_items, B, void_row)
            if void_row is not None:
                before = (model.E_user[users[void_row]].clone(), model.A_user[users[void_row]].clone())
            r = ref.step(users, pos, neg, kind)
            if kind == 'bpr-hinge':
                assert np.abs(1.0 + r['x'][r['live']]).min() > 1e-4, step
            model.step(users, pos, neg)
            l_got = float(model.read_loss().item())
            print('step %d loss %.6f (fp64 %.6f) auc %.6f (fp64 %.6f)' % (step, l_got, r['loss'], model.read_auc(),
                                                                          r['auc']))
            np.testing.assert_allclose(l_got, r['loss'], rtol=RTOL, err_msg='step %d' % step)
            np.testing.assert_allclose(model.pos_score.cpu().numpy(), r['ps'], rtol=RTOL, atol=1e-5)
            np.testing.assert_allclose(model.neg_score.cpu().numpy(), r['ns'], rtol=RTOL, atol=1e-5)
            close = int((np.abs(r['x'][r['live']]) <= 1e-5).sum())       # pairs fp32 cannot tell apart
            assert abs(model.read_auc() - r['auc']) <= close / B + 1e-6
            if void_row is not None:
                assert float(model.bl[void_row].item()) == 0.0
                assert torch.equal(model.E_user[users[void_row]], before[0])
                assert torch.equal(model.A_user[users[void_row]], before[1])
        if graphs:
            assert set(model._graphs) == {'step'} and model.n_captures == 1 and model.n_replays >= 3
        else:
            assert model.n_captures == 0 and not model._graphs
        ref.compare(model.gather_global_tables(slots=True), rtol=RTOL, atol=ATOL)
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------ 3. the model draws its negatives
def test_sharded_pair_model_draws_on_the_device(dev):
    from arx.dist import ShardedHMF
    dist = _group(dev, 29742)
    try:
        n_users, n_items, d, B = 300, 500, 64, 32
        syn, _, tables = _tables(n_users, n_items, d)
        full_user = 7

        def build(seed):
            m = ShardedHMF(n_users, n_items, d, B, 0, 0.5, 0, 1, dev, tables=tables, loss='bpr', seed=seed)
            ptr, items, lists = np.zeros(n_users + 2, dtype=np.int32), [], []
            for u in range(n_users):
                its = syn.pos_items[syn.pos_ptr[u]:syn.pos_ptr[u + 1]].tolist()
                its = list(range(n_items)) if u == full_user else its[::-1] + its[:1]    # unsorted, one doubled
                lists.append(set(its))
                items.extend(its)
                ptr[u + 1] = len(items)
            ptr[-1] = ptr[-2]
            m.set_positives(ptr, np.asarray(items, dtype=np.int32))
            return m, lists
        model, lists = build(3)
        rng = np.random.default_rng(2)
        users = rng.integers(0, n_users, size=B).astype(np.int32)
        users[users == full_user] = full_user + 1
        users[5] = full_user
        pos = rng.integers(0, n_items, size=B).astype(np.int32)
        with pytest.raises(RuntimeError, match="prepare_pair_negatives"):
            model.prepare_route(users, pos)
        model.prepare_pair_negatives()
        seq = []
        for step in range(4):                                   # eager, captured, replayed: every route draws anew
            route = model.prepare_route(users, pos)
            ng = route['neg_items'].cpu().numpy()
            assert ng[5] == -1 and (np.delete(ng, 5) >= 0).all() and ng.max() < n_items
            assert all(int(ng[r]) not in lists[int(users[r])] for r in range(B) if r != 5)
            model.step(route)
            assert np.isfinite(float(model.read_loss().item())) and float(model.bl[5].item()) == 0.0
            seq.append(ng)
        assert all((seq[k] != seq[k + 1]).mean() > 0.5 for k in range(3))
        assert model.n_captures == 1 and model.n_replays == 2
        twin, _ = build(3)
        twin.prepare_pair_negatives()
        for step in range(4):
            np.testing.assert_array_equal(twin.prepare_route(users, pos)['neg_items'].cpu().numpy(), seq[step])
        other, _ = build(4)
        other.prepare_pair_negatives()
        assert (other.prepare_route(users, pos)['neg_items'].cpu().numpy() != seq[0]).mean() > 0.5
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------ 4. 'mce'
@pytest.mark.parametrize("B,S,exchange", [(32, 64, 'rows'), (128, 128, 'rows'), (32, 64, 'logits')])
def test_sharded_mce_world1(dev, B, S, exchange):
    """tests/test_dist_gpu.py's world-1 'mw' test with loss='mce' against the oracle's 'mce'; (128, 128) is a shape
    of the fused 'mce' family: the step must have run on it."""
    from arx import ops
    from arx.dist import ShardedHMF
    dist = _group(dev, 29743)
    try:
        n_users, n_items, d = 300, 500, 64
        syn, params, tables = _tables(n_users, n_items, d)
        model = ShardedHMF(n_users, n_items, d, B, S, 0.5, 0, 1, dev, tables=tables, exchange=exchange, loss='mce')
        ptr = np.concatenate([syn.pos_ptr[:n_users + 1], [syn.pos_ptr[n_users]]]).astype(np.int32)
        model.set_positives(ptr, syn.pos_items)
        ref = rg.RefLatentProductModel(d, B, 0.5, syn.u_attr, syn.i_attr, syn.item_ind2logit_ind_dict(),
                                       syn.logit_ind2item_ind, loss_function='mce', n_sampled=S, params=params,
                                       dtype=np.float64)
        pos = syn.positives_dict()
        ref.prepare_warp(pos, pos)
        rng = np.random.default_rng(3)
        for step in range(6):
            pool = None
            if step in (0, 2, 4):
                pool = syn.sample_pool(S, rng)
                id2idx = {int(v): i for i, v in enumerate(pool)}
                model.set_pool(pool)
            users, items = syn.sample_batch(B, rng)
            l_ref = ref.step(list(users), list(items), pool, id2idx, loss='mce')
            model.step(users, items)
            np.testing.assert_allclose(float(model.read_loss().item()), l_ref, rtol=RTOL, err_msg='step %d' % step)
        if exchange == 'rows':
            want = ops.mce_scorer_supported(B, S, d)
            assert want == ((B, S) == (128, 128) and not ops.SCORER_F32)
            assert isinstance(getattr(model, 'scorer', None), ops.MceScorer) == want
        got = model.gather_global_tables()
        P = ref.att_emb.params
        np.testing.assert_allclose(got['user'], P['userembed_cat_0'][2:], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got['item'], P['itemembed_cat_0'][2:], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got['item_bias'], P['item_bias_cat_0'][2:, 0], rtol=RTOL, atol=ATOL)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("replicated", [False, True])
def test_sharded_het_mce_world1(dev, replicated):
    from arx.dist import ShardedHMFBags, ShardedHMFRepTokens
    from arx.utils.synthetic import SyntheticHMF
    dist = _group(dev, 29744)
    try:
        n_users, n_items, V, d, B, S = 300, 500, 120, 64, 32, 64
        syn = SyntheticHMF(n_users=n_users, n_items=n_items, seed=1, permute_logits=False, n_pos=8,
                           item_mulhot=True, mulhot_vocab=V, avg_len=5, max_len=12)
        ia = syn.i_attr
        n_tok = ia._embedding_classes_list_mulhot[0]
        params = syn.glorot_params(d, seed=2, scale=0.5)
        tables = {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
                  'item_bias': params['item_bias_cat_0'][2:], 'token': params['itemembed_mulhot_0'],
                  'token_bias': params['item_bias_mulhot_0']}
        bags = (np.asarray(ia.features_mulhot[0]), np.asarray(ia.mulhot_starts[0]), np.asarray(ia.mulhot_lengths[0]))
        cls = ShardedHMFRepTokens if replicated else ShardedHMFBags
        model = cls(n_users, n_items, d, B, S, 0.5, 0, 1, dev, bags, n_tok, tables=tables, loss='mce')
        ptr = np.concatenate([syn.pos_ptr[:n_users + 1], [syn.pos_ptr[n_users]]]).astype(np.int32)
        model.set_positives(ptr, syn.pos_items)
        ref = rg.RefLatentProductModel(d, B, 0.5, syn.u_attr, syn.i_attr, syn.item_ind2logit_ind_dict(),
                                       syn.logit_ind2item_ind, loss_function='mce', n_sampled=S, params=params,
                                       dtype=np.float64)
        pos = syn.positives_dict()
        ref.prepare_warp(pos, pos)
        rng = np.random.default_rng(3)
        for step in range(5):
            pool = None
            if step in (0, 2):
                pool = syn.sample_pool(S, rng)
                id2idx = {int(v): i for i, v in enumerate(pool)}
                model.set_pool(pool)
            users, items = syn.sample_batch(B, rng)
            l_ref = ref.step(list(users), list(items), pool, id2idx, loss='mce')
            model.step(users, items)
            np.testing.assert_allclose(float(model.read_loss().item()), l_ref, rtol=RTOL, err_msg='step %d' % step)
        got = model.gather_global_tables()
        P = ref.att_emb.params
        for name, want in (('user', P['userembed_cat_0'][2:]), ('item', P['itemembed_cat_0'][2:]),
                           ('item_bias', P['item_bias_cat_0'][2:, 0]), ('token', P['itemembed_mulhot_0']),
                           ('token_bias', P['item_bias_mulhot_0'][:, 0])):
            np.testing.assert_allclose(got[name], want, rtol=RTOL, atol=ATOL, err_msg=name)
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------ 5. serving does not care about the loss
def test_recommend_of_a_bpr_trained_sharded_model(dev):
    from arx.dist import ShardedHMF
    dist = _group(dev, 29745)
    try:
        n_users, n_items, d, B, k = 300, 500, 64, 32, 10
        _, _, tables = _tables(n_users, n_items, d)
        model = ShardedHMF(n_users, n_items, d, B, 0, 0.5, 0, 1, dev, tables=tables, loss='bpr')
        rng = np.random.default_rng(4)
        for step in range(2):
            model.step(*_pair_batch(rng, n_users, n_items, B, None))
        users = rng.choice(n_users, size=B, replace=False).astype(np.int32)
        ids, vals = model.recommend(users, k, return_values=True)
        t = model.gather_global_tables()
        logits = t['user'][users].astype(np.float64) @ t['item'].astype(np.float64).T + t['item_bias']
        want = np.argsort(-logits, axis=1, kind='stable')[:, :k]
        gaps = np.take_along_axis(logits, want, 1)[:, :-1] - np.take_along_axis(logits, want, 1)[:, 1:]
        assert gaps.min() > 1e-6                                 # (no near tie that fp32 could order the other way)
        np.testing.assert_array_equal(ids.cpu().numpy(), want)
    finally:
        dist.destroy_process_group()
