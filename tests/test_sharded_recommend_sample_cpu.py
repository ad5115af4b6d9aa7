"""ShardedHMF.recommend_sampled(sample_temperature=, sample_seed=, return_logprob=)
without a GPU: gloo worlds of 2 and 3 ranks
with a numpy compute double of the keyed shard stage and the finish (tests/numpy_backend_sample.py), against ONE global
oracle over global ids (tests/sample_oracle.py: sample_topk on the exact scores with the noise of (seed, global user,
global item)) and the float64 propensities of tests/recommend_logprob_oracle.py.  Uneven shards, a rank without users,
per-user temperatures including 0, with and without exclusions + tags; the seed rules; the ABI of
include/arx_sample_shard.h against SAMPLE_SHARD_PROTOTYPES by type; argument validation before any HIP call."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["arx_gemm_nt_topk_filter_sample_keyed", "arx_picks_to_shard", "arx_sample_logp_finish_shards",
         "arx_topk_gumbel_add_keyed", "arx_topk_gumbel_strip_keyed"]


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from arx.dist import ShardedHMF
    from numpy_backend_sample import SampleRecBackend, noise
    import recommend_logprob_oracle as RL
    import sample_oracle as SM
    import tags_oracle as T

    n_users, n_items, d, B_loc, k = 23, 37, 16, 6, 12            # 37 items: uneven shards in both worlds
    rng = np.random.default_rng(7)                               # the same tables on every rank
    U = (rng.integers(-2, 3, size=(n_users, d)) / 2.0).astype(np.float32)
    I = (rng.integers(-2, 3, size=(n_items, d)) / 2.0).astype(np.float32)
    b = (rng.integers(-4, 5, size=n_items) / 4.0).astype(np.float32)
    tags = rng.integers(0, 16, n_items).astype(np.uint32)
    model = ShardedHMF(n_users, n_items, d, B_loc, 8, 0.5, rank, world, 'cpu', backend=SampleRecBackend(),
                       tables={'user': U, 'item': I, 'item_bias': b})
    own = np.arange(rank, n_users, world)
    users = own[:B_loc - (rank % 2)] if rank != world - 1 else own[:0]     # uneven asks; the last rank asks for nobody
    n = len(users)
    logits = (U.astype(np.float64) @ I.astype(np.float64).T + b.astype(np.float64)).astype(np.float32)   # exact
    L = logits[users]
    tau_u = np.random.default_rng(3).choice([0.0, 0.25, 1.0, 3.0], n_users).astype(np.float32)
    tau_u[own[0]] = 0.0
    tau_u[own[1]] = 2.0
    tau = tau_u[users]
    gids = np.arange(n_items)

    def oracle(seed, **filt):
        return SM.sample_topk(L, noise(seed, users, gids), tau, k, **filt)

    def check_logp(ids, vals, lp, elig):
        exp = RL.logp(L, elig, ids, tau)
        tol = RL.tolerance(L, elig, tau, exp)
        assert RL.worst(lp, exp, tol) <= 1
        assert (lp[tau == 0] == 0).all() and (lp[ids < 0] == 0).all()
        sc = np.where(ids >= 0, np.take_along_axis(L, np.maximum(ids, 0), 1), -np.inf).astype(np.float32)
        np.testing.assert_array_equal(vals, sc)                  # the exact scores

    plain = model.recommend(users, k).numpy()
    with pytest.raises(ValueError):
        model.recommend_sampled(users, k, return_logprob=True)           # no temperature
    for bad in (dict(sample_temperature=-1.0), dict(sample_temperature=[1.0] * (n + 1)),
                dict(sample_temperature=1.0, sample_seed=-1), dict(sample_temperature=1.0, sample_seed=2 ** 63),
                dict(sample_temperature=float('nan'))):
        with pytest.raises(ValueError):
            model.recommend_sampled(users, k, **bad)
    assert getattr(model, 'sample_draws', 0) == 0                # a refused call does not move the counter

    # ---- no filters: ids, stripped values, a replay, the tau = 0 rows
    ids, vals = model.recommend_sampled(users, k, return_values=True, sample_temperature=tau, sample_seed=11)
    ids, vals = ids.numpy(), vals.numpy()
    kv, sc, ki, ky = oracle(11)
    np.testing.assert_array_equal(ids, ki)
    assert (np.abs(vals.astype(np.float64) - sc) <= SM.strip_bound(kv, sc)).all()
    np.testing.assert_array_equal(ids[tau == 0], plain[tau == 0])
    np.testing.assert_array_equal(vals[tau == 0], sc[tau == 0])
    np.testing.assert_array_equal(model.recommend_sampled(users, k, sample_temperature=tau, sample_seed=11).numpy(), ids)
    other = model.recommend_sampled(users, k, sample_temperature=tau, sample_seed=12).numpy()    # (a collective: every rank)
    if n:
        assert (ids[tau > 0] != plain[tau > 0]).any() and (other != ids).any()
    # all rows at tau = 0: the plain call
    np.testing.assert_array_equal(model.recommend_sampled(users, k, sample_temperature=0.0, sample_seed=5).numpy(), plain)
    # the propensities; one number for every user
    ids, vals, lp = model.recommend_sampled(users, k, return_values=True, sample_temperature=tau, sample_seed=11,
                                    return_logprob=True)
    np.testing.assert_array_equal(ids.numpy(), ki)
    check_logp(ki, vals.numpy(), lp.numpy(), RL.eligible(L))
    ids, lp = model.recommend_sampled(users, k, sample_temperature=0.5, sample_seed=4, return_logprob=True)
    np.testing.assert_array_equal(ids.numpy(), SM.sample_topk(L, noise(4, users, gids), np.full(n, 0.5), k)[2])
    assert tuple(lp.shape) == (n, k)

    # ---- sample_seed=None counts up a per-model counter (the same on ranks in lockstep)
    a = model.recommend_sampled(users, k, sample_temperature=tau).numpy()
    b2 = model.recommend_sampled(users, k, sample_temperature=tau).numpy()
    assert model.sample_draws == 2
    np.testing.assert_array_equal(a, oracle(0)[2])
    np.testing.assert_array_equal(b2, oracle(1)[2])

    # ---- different seeds on two ranks: ValueError on EVERY rank
    with pytest.raises(ValueError):
        model.recommend_sampled(users, k, sample_temperature=tau, sample_seed=100 + (rank == 0))

    # ---- exclusions + tags (one user keeps fewer than k items: -1 tails)
    model.prepare_item_tags(tags)
    hist = [{int(u): np.random.default_rng(500 + int(u)).integers(0, n_items, size=10).tolist()
             for u in np.arange(g, n_users, world)} for g in range(world)]
    model.prepare_recommend_exclusions(hist[rank])
    wr = np.random.default_rng(99)
    any_u = wr.integers(0, 16, n_users).astype(np.uint32)
    all_u = wr.integers(0, 4, n_users).astype(np.uint32)
    any_u[::4] = 0
    all_u[own[1]] = 15                                           # few items carry all four bits
    ex_rows = [sorted(set(hist[rank][int(u)])) for u in users]
    filt = dict(tags=tags, want_any=any_u[users], want_all=all_u[users], ex_lists=ex_rows)
    ids, vals, lp = model.recommend_sampled(users, k, exclude_seen=True, return_values=True, tags_any=any_u[users],
                                    tags_all=all_u[users], sample_temperature=tau, sample_seed=21, return_logprob=True)
    kv, sc, ki, ky = oracle(21, **filt)
    np.testing.assert_array_equal(ids.numpy(), ki)
    if n:
        assert (ki[1] == -1).any()
    check_logp(ki, vals.numpy(), lp.numpy(), RL.eligible(L, tags, any_u[users], all_u[users], ex_rows))
    ids2 = model.recommend_sampled(users, k, exclude_seen=True, tags_any=any_u[users], tags_all=all_u[users],
                           sample_temperature=tau, sample_seed=21).numpy()
    np.testing.assert_array_equal(ids2, ki)
    np.testing.assert_array_equal(ids2[tau == 0], T.topk(L, k, tags, any_u[users], all_u[users], ex_rows)[1][tau == 0])
    # the plain call is still the plain call
    np.testing.assert_array_equal(model.recommend(users, k).numpy(), plain)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_sampled_recommend_matches_global_oracle_gloo(tmp_path, world):
    import torch.multiprocessing as mp
    port = 34300 + 10 * world + (os.getpid() % 50) * 40
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(world))


def test_draw_does_not_depend_on_the_world_size(tmp_path):
    """The numpy double's keyed noise: one user's keyed shard lists merged over 2 and over 3 shards are the same draw
    (a function of (seed, user, item) and the scores alone)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from numpy_backend_sample import noise
    import sample_oracle as SM
    g = noise(9, [5, 1000003, -1], np.arange(40))
    assert (g[2] == 0).all() and (g[0] != g[1]).any()
    for W in (2, 3):
        for s in range(W):
            np.testing.assert_array_equal(noise(9, [5], np.arange(s, 40, W))[0], g[0, s::W])
    np.testing.assert_array_equal(g[:2], SM.gumbel64(SM.bits(9, [5, 1000003], np.arange(40, dtype=np.uint32)))
                                  .astype(np.float32))


def test_old_backends_without_the_sample_argument_serve_plain_calls():
    """dist.py passes sample= to the backend only when a temperature is given (the convention of tags=): a shard_topk
    without the parameter is called exactly as before."""
    import inspect
    from arx.dist import HipBackend, ShardedHMF, ShardedHetView, ShardedHMFBags, ShardedHMFRepTokens, ShardedW2V
    from numpy_backend_tags import TagsRecBackend
    assert 'sample' in inspect.signature(HipBackend.shard_topk).parameters
    assert 'sample' not in inspect.signature(TagsRecBackend.shard_topk).parameters
    new = ['sample_temperature', 'sample_seed', 'return_logprob']
    plain = ['users', 'k', 'exclude_seen', 'return_values', 'tags_any', 'tags_all']
    for cls in (ShardedHMF, ShardedHetView):
        assert list(inspect.signature(cls.recommend).parameters)[1:] == plain      # recommend's list stays as it was
        p = inspect.signature(cls.recommend_sampled).parameters
        assert list(p)[1:] == plain + new
        assert p['sample_temperature'].default is None and p['sample_seed'].default is None
        assert p['return_logprob'].default is False
    assert list(inspect.signature(ShardedW2V.recommend).parameters)[1:] == ['users', 'context'] + plain[1:]
    assert list(inspect.signature(ShardedW2V.recommend_sampled).parameters)[1:] == ['users', 'context'] + plain[1:] + new
    for cls in (ShardedHMFBags, ShardedHMFRepTokens):             # the forwarders keep their signatures and refuse both
        assert list(inspect.signature(cls.recommend).parameters)[1:] == ['users', 'k', 'exclude_seen', 'return_values']
        with pytest.raises(NotImplementedError):
            cls.recommend_sampled(object.__new__(cls), [0], 1, sample_temperature=1.0)
    assert 'sample' in inspect.signature(ShardedHetView._recommend).parameters

    # world 1 on the CPU with a backend that does not know sample=: plain and tagged calls are served
    import torch
    n_users, n_items, d, B_loc, k = 9, 14, 8, 4, 5
    rng = np.random.default_rng(2)
    tabs = {'user': (rng.integers(-2, 3, size=(n_users, d)) / 2.0).astype(np.float32),
            'item': (rng.integers(-2, 3, size=(n_items, d)) / 2.0).astype(np.float32),
            'item_bias': (rng.integers(-4, 5, size=n_items) / 4.0).astype(np.float32)}
    model = ShardedHMF(n_users, n_items, d, B_loc, 8, 0.5, 0, 1, 'cpu', backend=TagsRecBackend(), tables=tabs)
    ids = model.recommend(np.arange(3), k)
    assert isinstance(ids, torch.Tensor) and tuple(ids.shape) == (3, k)
    model.prepare_item_tags(np.ones(n_items, dtype=np.int64))
    np.testing.assert_array_equal(model.recommend(np.arange(3), k, tags_any=1).numpy(), ids.numpy())
    with pytest.raises(TypeError):
        model.recommend_sampled(np.arange(3), k, sample_temperature=1.0, sample_seed=0)


def test_sample_shard_header_and_its_table_stay_in_step():
    import test_abi_signatures_cpu as A
    from arx import _lib
    decls = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_sample_shard.h")).read())
    assert sorted(decls) == NAMES
    protos = _lib.SAMPLE_SHARD_PROTOTYPES
    assert sorted(protos) == NAMES
    bad = [m for name in NAMES for m in A.mismatches(name, decls[name], protos[name])]
    assert not bad, "\n".join(bad)
    others = (_lib.PROTOTYPES, _lib.TAGS_PROTOTYPES, _lib.SLATE_PROTOTYPES, _lib.DIVERSE_PROTOTYPES,
              _lib.SAMPLE_PROTOTYPES, _lib.SLATE_SAMPLE_PROTOTYPES, _lib.SAMPLE_LOGP_PROTOTYPES)
    for name in NAMES:                                               # not vacuous: one i64 narrowed to i32 is reported
        res, args = protos[name]
        k64 = next(k for k, a in enumerate(args) if a is A.C.c_int64)
        narrowed = list(args)
        narrowed[k64] = A.C.c_int32
        assert any("parameter %d " % k64 in m for m in A.mismatches(name, decls[name], (res, narrowed)))
        assert hasattr(_lib.lib, name) and getattr(_lib.lib, name).argtypes == list(args)
        assert all(name not in t for t in others)
    assert len(A.load_prototypes()) == A.N_ENTRY_POINTS == len(_lib.PROTOTYPES) == 146
    assert '#include "arx_sample_shard.h"' in open(os.path.join(A.ROOT, "include", "arx.h")).read()
    # arx_sample.h and arx_sample_logp.h keep every signature
    for hdr, tab in (("arx_sample.h", _lib.SAMPLE_PROTOTYPES), ("arx_sample_logp.h", _lib.SAMPLE_LOGP_PROTOTYPES)):
        d2 = A.parse_header(open(os.path.join(A.ROOT, "include", hdr)).read())
        assert sorted(d2) == sorted(tab)
        assert not [m for name in tab for m in A.mismatches(name, d2[name], tab[name])]


def _err(lib):
    m = lib.arx_last_error()
    return m.decode() if m else ""


def test_keyed_entries_validate_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib
    A = 4096                                  # stands in for a device pointer: only compared with NULL / alignment
    EINVAL = -1

    def add(lg=A, ld=64, M=4, col0=0, ncols=64, tau=A, tr=4, sw=A, mul=3, ad=2, nr=A):
        return lib.arx_topk_gumbel_add_keyed(lg, ld, M, col0, ncols, tau, tr, sw, mul, ad, nr, None)
    for kw in (dict(lg=None), dict(tau=None), dict(sw=None), dict(mul=0), dict(ad=3), dict(ad=-1), dict(tr=0),
               dict(col0=-1), dict(ld=63),
               dict(col0=2 ** 31 // 3, ncols=8, ld=8),                  # (col0 + 7) * 3 + 2 >= 2^31
               dict(mul=1, ad=0, col0=2 ** 31 - 8, ncols=8, ld=8)):
        assert add(**kw) == EINVAL and "arx_topk_gumbel_add_keyed" in _err(lib), kw
    assert add(M=0) == 0 and add(ncols=0) == 0                         # nothing to do: no launch

    def strip(v=A, ldv=8, idx=A, ldi=8, B=4, k=8, tau=A, tr=4, sw=A, mul=1, ad=0, nr=None):
        return lib.arx_topk_gumbel_strip_keyed(v, ldv, idx, ldi, B, k, tau, tr, sw, mul, ad, nr, None)
    for kw in (dict(v=None), dict(idx=None), dict(tau=None), dict(sw=None), dict(mul=0), dict(ad=1), dict(k=0),
               dict(ldv=7), dict(tr=0)):
        assert strip(**kw) == EINVAL and "arx_topk_gumbel_strip_keyed" in _err(lib), kw
    assert strip(B=0) == 0

    def filt(K=64, N=1000, base=65536, mul=3, ad=2, tau=A, sw=A, thr=A):
        return lib.arx_gemm_nt_topk_filter_sample_keyed(A, K, 130, A, K, N, K, None, thr, 1, base, A, A, 4096, 32, A,
                                                        None, 0, None, 0, None, None, None, None, None, 0, tau, 130,
                                                        sw, mul, ad, None, None)
    for kw in (dict(tau=None), dict(sw=None), dict(thr=None), dict(mul=0), dict(ad=3), dict(ad=-1), dict(K=48),
               dict(base=2 ** 31 // 3, N=64)):
        assert filt(**kw) < 0 and "arx_gemm_nt_topk_filter_sample_keyed" in _err(lib), kw

    def picks(ids=A, ldi=8, B=4, k=8, W=3, s=2, cols=A, ldc=8):
        return lib.arx_picks_to_shard(ids, ldi, B, k, W, s, cols, ldc, None)
    for kw in (dict(ids=None), dict(cols=None), dict(B=-1), dict(k=0), dict(ldi=7), dict(ldc=7), dict(W=0),
               dict(s=3), dict(s=-1)):
        assert picks(**kw) == EINVAL and "arx_picks_to_shard" in _err(lib), kw
    assert picks(B=0) == 0

    def fin(idx=A, ldi=8, ps=A, ldps=20, slab_ps=80, m=A, s=A, ldl=20, slab_l=80, W=3, P=5, tau=A, tr=4, B=4, k=8,
            lp=A, ldo=8, vals=A, ldv=8):
        return lib.arx_sample_logp_finish_shards(idx, ldi, ps, ldps, slab_ps, m, s, ldl, slab_l, W, P, tau, tr, B, k,
                                                 lp, ldo, vals, ldv, None)
    for kw in (dict(idx=None), dict(ps=None), dict(m=None), dict(s=None), dict(tau=None), dict(lp=None), dict(W=0),
               dict(W=65), dict(P=0), dict(ldl=4), dict(k=0), dict(k=1025), dict(ldi=7), dict(ldo=7), dict(ldv=7),
               dict(tr=0), dict(B=-1), dict(slab_ps=-1), dict(slab_l=-1)):
        assert fin(**kw) == EINVAL and "arx_sample_logp_finish_shards" in _err(lib), kw
    assert fin(B=0) == 0 and fin(B=0, vals=None) == 0
