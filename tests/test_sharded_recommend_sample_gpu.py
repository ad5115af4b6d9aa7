"""ShardedHMF.recommend_sampled(sample_temperature=, sample_seed=, return_logprob=)
on the GPU: world 1 (an nccl group of one,
as tests/test_sharded_recommend_gpu.py sets it up), once two rank processes on the one GPU over gloo, and the law.

The oracle (tests/sample_oracle.py) ranks the device's own logits -- every shard's columns as the shard computes them
(_shard_logits), scattered to global ids -- plus the device's own keyed noise of (seed, global user id, global item id):
the keyed add of tau = 1 on zeros with (col_mul, col_add) = (1, 0) and the users as noise rows.  Ids compare exactly
outside the rows whose k-th / (k + 1)-th keys lie inside the strip bound; the propensities against
tests/recommend_logprob_oracle.py within its tolerance."""
import os
import time

import numpy as np
import pytest

import recommend_logprob_oracle as RL
import sample_oracle as S
import tags_oracle as T
from test_recommend_sample_gpu import TAUS, _check_values
from test_sample_keyed_kernels_gpu import _keyed_noise
from test_sharded_recommend_gpu import _histories, _init_world1, _shard_logits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _taus(rng, n):
    tau = TAUS[rng.integers(1, 4, n)]
    tau[::5] = 0
    return tau


def _oracle(dev, lg, users, tau, seed, k, **filt):
    g = _keyed_noise(dev, seed, users, lg.shape[1], 1, 0)
    kv, sc, ei, ky = S.sample_topk(lg, g, tau, k, **filt)
    return sc, ei, ky, S.close_rows(ky, kv, sc, k)


def _check_logp(what, lg, elig, tau, ids, vals, lp, close):
    ok = ~close
    exp = RL.logp(lg[ok], elig[ok], ids[ok], tau[ok])
    tol = RL.tolerance(lg[ok], elig[ok], tau[ok], exp)
    w = RL.worst(lp[ok], exp, tol)
    print("%s: largest logp error / tolerance %.3f" % (what, w))
    assert w <= 1
    assert (lp[tau == 0] == 0).all() and (lp[ids < 0] == 0).all()
    sc = np.where(ids >= 0, np.take_along_axis(lg, np.maximum(ids, 0), 1), -np.inf)
    np.testing.assert_array_equal(vals[ok], sc[ok])                      # the exact bits of the shard's scorer


def _world1_model(dev, d, n_items=100003, n_users=500, B_loc=64):
    import torch
    from arx.dist import ShardedHMF
    g = torch.Generator(device='cpu').manual_seed(3)
    U = torch.randn(n_users, d, generator=g) * 0.3
    I = torch.randn(n_items, d, generator=g) * 0.3
    b = torch.randn(n_items, generator=g) * 0.1
    model = ShardedHMF(n_users, n_items, d, B_loc, 64, 0.1, 0, 1, dev,
                       tables={'user': U.numpy(), 'item': I.numpy(), 'item_bias': b.numpy()})
    return model, U, I, b


def _logits_of(dev, U, I, b, users, B_loc):
    import torch
    U_all = torch.zeros(B_loc, U.shape[1], device=dev)
    U_all[:len(users)] = U[torch.from_numpy(users)].to(dev)
    return _shard_logits(U_all, I.to(dev), b.to(dev), 1, np.arange(len(users)), dev)


@pytest.mark.parametrize("d", [64, 128])
def test_sharded_sampled_recommend_world1(dev, d):
    """World 1, 100003 items (past the first chunk: the fused keyed filter runs), k = 30."""
    import torch.distributed as dist
    _init_world1(dev, 29791)
    try:
        n_users, n_items, B_loc, k = 500, 100003, 64, 30
        model, U, I, b = _world1_model(dev, d)
        rng = np.random.default_rng(4)
        users = rng.choice(n_users, size=B_loc - 5, replace=False)
        n = len(users)
        lg = _logits_of(dev, U, I, b, users, B_loc)
        tau = _taus(rng, n)
        plain_i, plain_v = (t.cpu().numpy() for t in model.recommend(users, k, return_values=True))
        with pytest.raises(ValueError):
            model.recommend_sampled(users, k, return_logprob=True)
        sc, ei, ky, close = _oracle(dev, lg, users, tau, 11, k)
        assert close.mean() <= 0.04
        ids, vals = (t.cpu().numpy() for t in model.recommend_sampled(users, k, return_values=True, sample_temperature=tau,
                                                              sample_seed=11))
        np.testing.assert_array_equal(ids[~close], ei[~close])
        _check_values(vals[~close], ids[~close], lg[~close], ky[~close])  # within the strip bound
        zero = tau == 0
        np.testing.assert_array_equal(ids[zero], plain_i[zero])          # tau = 0: the plain call, bit for bit
        np.testing.assert_array_equal(vals[zero], plain_v[zero])
        assert (ids[~zero] != plain_i[~zero]).any()
        np.testing.assert_array_equal(model.recommend_sampled(users, k, sample_temperature=tau, sample_seed=11).cpu().numpy(),
                                      ids)                               # a seed replays
        assert (model.recommend_sampled(users, k, sample_temperature=tau, sample_seed=12).cpu().numpy() != ids).any()
        # the same users in another order: the same per-user lists
        perm = rng.permutation(n)
        got = model.recommend_sampled(users[perm], k, sample_temperature=tau[perm], sample_seed=11).cpu().numpy()
        keep = ~close[perm]
        np.testing.assert_array_equal(got[keep], ids[perm][keep])
        # the propensities
        ids2, vals2, lp = (t.cpu().numpy() for t in model.recommend_sampled(users, k, return_values=True,
                                                                    sample_temperature=tau, sample_seed=11,
                                                                    return_logprob=True))
        np.testing.assert_array_equal(ids2, ids)
        _check_logp('d %d plain' % d, lg, RL.eligible(lg), tau, ids2, vals2, lp, close)
        assert (lp[~zero] < 0).all()
        if d == 128:
            return
        # exclusions + tags; user 2 has nothing eligible
        tags = T.random_tags(rng, n_items)
        want_any, want_all = T.random_words(rng, n, zero_every=7)
        want_all[2] = 0xffffffff
        model.prepare_item_tags(tags)
        ex = _histories(rng, users, n_items, top=ei.clip(min=0))
        model.prepare_recommend_exclusions(ex)
        ex_rows = [sorted(set(ex[int(u)])) for u in users]
        filt = dict(tags=tags, want_any=want_any, want_all=want_all, ex_lists=ex_rows)
        sc, ei, ky, close = _oracle(dev, lg, users, tau, 21, k, **filt)
        assert close.mean() <= 0.04
        ids, vals, lp = (t.cpu().numpy() for t in model.recommend_sampled(
            users, k, exclude_seen=True, return_values=True, tags_any=want_any, tags_all=want_all,
            sample_temperature=tau, sample_seed=21, return_logprob=True))
        np.testing.assert_array_equal(ids[~close], ei[~close])
        assert (ids[2] == -1).all() and (lp[2] == 0).all() and np.isneginf(vals[2]).all()
        _check_logp('ex + tags', lg, RL.eligible(lg, tags, want_any, want_all, ex_rows), tau, ids, vals, lp, close)
        ids3 = model.recommend_sampled(users, k, exclude_seen=True, tags_any=want_any, tags_all=want_all,
                               sample_temperature=tau, sample_seed=21).cpu().numpy()
        np.testing.assert_array_equal(ids3, ids)
        np.testing.assert_array_equal(model.recommend(users, k).cpu().numpy(), plain_i)
    finally:
        dist.destroy_process_group()


def test_sharded_sampled_overflow_reruns_chunked(dev):
    """One user excludes the whole first chunk: its threshold is -inf, the fused candidate lists (segments of 8)
    overflow and the shard's selection re-runs chunked: the same ids, the propensities within tolerance."""
    import torch.distributed as dist
    _init_world1(dev, 29792)
    try:
        n_users, n_items, d, B_loc, k = 500, 100003, 64, 64, 30
        model, U, I, b = _world1_model(dev, d)
        rng = np.random.default_rng(6)
        users = rng.choice(n_users, size=B_loc, replace=False)
        lg = _logits_of(dev, U, I, b, users, B_loc)
        tau = np.full(B_loc, 2.0, dtype=np.float32)
        sets = {int(u): rng.integers(0, n_items, 60).tolist() for u in users}
        sets[int(users[0])] = list(range(65536))
        model.prepare_recommend_exclusions(sets)
        ex_rows = [sorted(set(sets[int(u)])) for u in users]
        sc, ei, ky, close = _oracle(dev, lg, users, tau, 3, k, ex_lists=ex_rows)
        kw = dict(exclude_seen=True, return_values=True, sample_temperature=tau, sample_seed=3, return_logprob=True)
        ids, vals, lp = (t.cpu().numpy() for t in model.recommend_sampled(users, k, **kw))
        scan = model.be._scans[(B_loc, n_items, d, k, False)]
        assert scan.fused
        scan.slack, scan.min_capp = 0.0, 8                              # segments shorter than the columns of a range
        ids_o, vals_o, lp_o = (t.cpu().numpy() for t in model.recommend_sampled(users, k, **kw))
        assert int(scan.overflow.item()) != 0 and scan.fused             # (overflowed, re-ran chunked, restored)
        np.testing.assert_array_equal(ids_o[~close], ei[~close])
        np.testing.assert_array_equal(ids_o, ids)
        elig = RL.eligible(lg, ex_lists=ex_rows)
        _check_logp('overflow re-run', lg, elig, tau, ids_o, vals_o, lp_o, close)
        assert (ids_o[0] >= 65536).all()
    finally:
        dist.destroy_process_group()


def _two_rank_worker(rank, world, port, out_dir):
    import sys
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from arx.dist import ShardedHMF

    # uneven shards, both past the first chunk
    n_users, n_items, d, B_loc, k = 401, 2 * 70003 + 1, 64, 48, 30
    g = torch.Generator(device='cpu').manual_seed(9)
    U = torch.randn(n_users, d, generator=g) * 0.3
    I = torch.randn(n_items, d, generator=g) * 0.3
    b = torch.randn(n_items, generator=g) * 0.1
    model = ShardedHMF(n_users, n_items, d, B_loc, 64, 0.1, rank, world, dev,
                       tables={'user': U.numpy(), 'item': I.numpy(), 'item_bias': b.numpy()})
    rng = np.random.default_rng(21)                                     # the same stream on both ranks
    asks = [rng.choice(np.arange(s, n_users, world), size=B_loc - 7 * s, replace=False) for s in range(world)]
    tags = T.random_tags(rng, n_items)
    U_all = torch.zeros(world * B_loc, d, device=dev)
    for s in range(world):
        U_all[s * B_loc:s * B_loc + len(asks[s])] = U[torch.from_numpy(asks[s])].to(dev)
    mine = asks[rank]
    n = len(mine)
    tau = _taus(np.random.default_rng(70 + rank), n)
    want_any, want_all = T.random_words(np.random.default_rng(60 + rank), n, zero_every=7)
    want_all[2] = 0xffffffff                                            # nothing eligible: a row of -1
    lg = _shard_logits(U_all, I.to(dev), b.to(dev), world, rank * B_loc + np.arange(n), dev)
    # ---- no filters
    sc, ei, ky, close = _oracle(dev, lg, mine, tau, 31, k)
    assert close.mean() <= 0.05
    ids, vals, lp = (t.cpu().numpy() for t in model.recommend_sampled(mine, k, return_values=True, sample_temperature=tau,
                                                              sample_seed=31, return_logprob=True))
    np.testing.assert_array_equal(ids[~close], ei[~close])
    owners = ids[ids >= 0] % world
    assert (owners == 0).any() and (owners == 1).any()
    _check_logp('rank %d plain' % rank, lg, RL.eligible(lg), tau, ids, vals, lp, close)
    got, sv = (t.cpu().numpy() for t in model.recommend_sampled(mine, k, return_values=True, sample_temperature=tau,
                                                        sample_seed=31))
    np.testing.assert_array_equal(got, ids)
    _check_values(sv[~close], got[~close], lg[~close], ky[~close])
    # ---- exclusions + tags
    model.prepare_item_tags(tags)
    ex = _histories(np.random.default_rng(40 + rank), mine, n_items, top=ei.clip(min=0))
    model.prepare_recommend_exclusions(ex)
    ex_rows = [sorted(set(ex[int(u)])) for u in mine]
    filt = dict(tags=tags, want_any=want_any, want_all=want_all, ex_lists=ex_rows)
    sc, ei, ky, close = _oracle(dev, lg, mine, tau, 32, k, **filt)
    assert close.mean() <= 0.05
    ids, vals, lp = (t.cpu().numpy() for t in model.recommend_sampled(
        mine, k, exclude_seen=True, return_values=True, tags_any=want_any, tags_all=want_all, sample_temperature=tau,
        sample_seed=32, return_logprob=True))
    np.testing.assert_array_equal(ids[~close], ei[~close])
    assert (ids[2] == -1).all()
    _check_logp('rank %d ex + tags' % rank, lg, RL.eligible(lg, tags, want_any, want_all, ex_rows), tau, ids, vals, lp,
                close)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_sharded_sampled_recommend_two_ranks_one_gpu(dev, tmp_path):
    """Two rank processes on the one GPU over gloo: uneven shards and asks, per-user temperatures travelling with the
    user keys, picks owned by both shards, with and without exclusions + tags; ids and propensities against the global
    oracle.  The two processes run under a time limit of their own."""
    import torch.multiprocessing as mp
    port = 29980 + (os.getpid() % 100)
    ctx = mp.spawn(_two_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 240.0
    try:
        while not ctx.join(timeout=5.0):
            assert time.monotonic() < deadline, "the rank processes did not finish in time"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))


def _law_seeds(users, scores, tau, calls, k=3):
    """The first run of `calls` seeds (in steps of `calls`, at most 8 runs) whose ORACLE draws -- oracle_draws fed the
    keyed rows and columns: noise row = user id, noise column = item id -- pass the thresholds of test_device_law."""
    cols = np.arange(len(scores), dtype=np.uint32)
    for base in range(0, 8 * calls, calls):
        ids = []
        for seed in range(base, base + calls):
            ky = np.asarray(scores, dtype=np.float64)[None, :] + tau * S.gumbel64(S.bits(seed, users, cols))
            ids.append(np.argsort(-ky, axis=1, kind='stable')[:, :k])
        chi2, z = S.law_stats(np.concatenate(ids), scores, tau, k)
        if chi2 < 24.32 and z < 4.5:
            return list(range(base, base + calls)), np.concatenate(ids)
    raise AssertionError("no run of seeds passes the law on the oracle's own draws")


def test_sharded_sampled_law(dev):
    """8 items, k = 3, every user's latent row equal, tau = 1: 8 calls of 512 users with fixed seeds.  The first picks
    and the inclusion counts follow the Plackett-Luce law (the thresholds of test_device_law) -- the noise is keyed by
    the user id, so this also shows independence across users; and the reported propensities match the empirical
    frequencies of the ordered lists (the statistic of test_device_law_against_its_own_propensities)."""
    import torch.distributed as dist
    from arx.dist import ShardedHMF
    from test_recommend_sample_cpu import SCORES
    _init_world1(dev, 29793)
    try:
        n_users, n_items, d, B_loc, k, calls = 512, 8, 8, 512, 3, 8
        Ut = np.zeros((n_users, d), dtype=np.float32)
        Ut[:, 0] = 1.0
        It = np.zeros((n_items, d), dtype=np.float32)
        It[:, 0] = SCORES
        model = ShardedHMF(n_users, n_items, d, B_loc, 4, 0.1, 0, 1, dev,
                           tables={'user': Ut, 'item': It, 'item_bias': np.zeros(n_items, dtype=np.float32)})
        users = np.arange(n_users)
        seeds, oracle_ids = _law_seeds(users, SCORES, 1.0, calls)
        ids, lps = [], []
        for seed in seeds:
            i, lp = model.recommend_sampled(users, k, sample_temperature=1.0, sample_seed=seed, return_logprob=True)
            ids.append(i.cpu().numpy().astype(np.int64))
            lps.append(lp.cpu().numpy().astype(np.float64))
        ids, lps = np.concatenate(ids), np.concatenate(lps)
        assert (ids >= 0).all() and all(len(set(r)) == 3 for r in ids.tolist())
        chi2, z = S.law_stats(ids, SCORES, 1.0)
        print("seeds %d..%d: chi2 %.2f, inclusion %.2f sigma; rows equal to the float64 oracle's %.4f"
              % (seeds[0], seeds[-1], chi2, z, (ids == oracle_ids).all(1).mean()))
        assert chi2 < 24.32 and z < 4.5
        c2, cells, bound = RL.law_chi2(ids, lps, SCORES, 1.0)
        print("propensities: chi2 %.2f over %d cells, bound %.2f" % (c2, cells, bound))
        assert cells > 30 and c2 < bound
        L = np.tile(np.asarray(SCORES, dtype=np.float32), (len(ids), 1))
        elig = np.ones(L.shape, dtype=bool)
        tau = np.ones(len(ids), dtype=np.float32)
        want = RL.logp(L, elig, ids, tau)
        assert RL.worst(lps.astype(np.float32), want, RL.tolerance(L, elig, tau, want)) <= 1
    finally:
        dist.destroy_process_group()
