"""list_logprob of the row-sharded model (ShardedHMF.list_logprob) at world 1, beside the propensity stage of
recommend_sampled(return_logprob=True) it shares its mass pass with, and its two own kernels alone.

usage: python tools/sharded_list_logprob_bench.py [--B 4096] [--V 1000000] [--d 128,64] [--k 100] [--tau 1.0]
                                                  [--rounds 5] [--calls 3] [--out FILE.json]
World 1 is an nccl group of one on cuda:0.  The calls alternate inside each round (device-event timing, one warm-up
round first); the median per call is reported.
  list_logprob     the whole call on lists recommend_sampled drew: host checks, feeds, every launch, the clones
  sampled, sampled_logp   whole recommend_sampled calls without / with propensities; their difference is the
                   propensity stage as tools/sharded_sample_bench.py isolates it (logp_stage_diff)
  logp_stage       that stage's launches alone on the model's own buffers: HipBackend.shard_rest_mass
                   (arx_picks_to_shard, the sort, the rest-mass pass) + arx_sample_logp_finish_shards
  prepare_shard, merge_shards   arx_list_logp_prepare_shard / arx_list_logp_merge_shards alone, [B, k]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-recsys_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
from arx import ops  # noqa: E402
from arx.dist import ShardedHMF  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--V", type=int, default=1000000)
ap.add_argument("--d", default="128,64")
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--tau", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, V, k = args.B, args.V, args.k
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29796")
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(fns):
    """{name: median ms per call}: the calls alternate inside each round; the first round is the warm-up."""
    ms = {name: [] for name in fns}
    for rnd in range(args.rounds + 1):
        for name, fn in fns.items():
            t = timed(fn, args.calls)
            if rnd:
                ms[name].append(t)
    return {name: statistics.median(v) for name, v in ms.items()}


results = []
for d in (int(x) for x in args.d.split(",")):
    rng = np.random.default_rng(0)
    tabs = {'user': (rng.standard_normal((B, d)) * 0.3).astype(np.float32),
            'item': (rng.standard_normal((V, d)) * 0.3).astype(np.float32),
            'item_bias': (rng.standard_normal(V) * 0.1).astype(np.float32)}
    model = ShardedHMF(B, V, d, B, 64, 0.1, 0, 1, dev, tables=tabs)
    users = np.arange(B)
    tau = np.full(B, args.tau, dtype=np.float32)
    ids, lp0 = model.recommend_sampled(users, k, sample_temperature=tau, sample_seed=1, return_logprob=True)
    lp1 = model.list_logprob(users, ids, tau)
    same = bool(torch.equal(lp0, lp1))                       # the policy against itself: bit for bit

    def sampled(**kw):
        return model.recommend_sampled(users, k, sample_temperature=tau, sample_seed=1, **kw)

    # the propensity stage alone, on the buffers the calls above left on the model (world 1)
    be = model.be
    _, _, keys_all, U_all = model._rec_lat
    _, _, tau_all, seed_dev = model._rec_smp
    smp = (tau_all, B, seed_dev, 1, 0, keys_all)
    (P_max,) = [q[1] for q in model._rec_logp if q[0] == k]
    packed, _, _, lp = model._rec_logp[(k, P_max)]
    vo = torch.empty((B, k), dtype=torch.float32, device=dev)

    def logp_stage():
        be.shard_rest_mass(U_all, model.E_item[:V], model.b_item[:V], None, ids, 1, 0, smp, packed, P_max)
        be.sample_logp_finish_shards(ids, packed.view(1, B, 2 * P_max + k), P_max, smp, lp, vo)

    i32 = lambda: torch.empty((B, k), dtype=torch.int32, device=dev)
    clean, why, pc, ps, gclean, gwhy = (i32() for _ in range(6))
    prep = lambda: ops.list_logp_prepare_shard(ids, V, 1, 0, None, None, clean, why, pc, ps)
    prep()
    merge = lambda: ops.list_logp_merge_shards(ids, V, why.view(1, B, k), gclean, gwhy)
    ms = alternate({'list_logprob': lambda: model.list_logprob(users, ids, tau), 'sampled': sampled,
                    'sampled_logp': lambda: sampled(return_logprob=True), 'logp_stage': logp_stage,
                    'prepare_shard': prep, 'merge_shards': merge})
    row = dict(B=B, V=V, d=d, k=k, tau=args.tau, P_max=P_max, self_drawn_bit_equal=same,
               **{n + '_ms': round(v, 4) for n, v in ms.items()})
    row['logp_stage_diff_ms'] = round(ms['sampled_logp'] - ms['sampled'], 4)
    row['list_over_logp_stage'] = round(ms['list_logprob'] / ms['logp_stage'], 3)
    row['list_over_logp_stage_diff'] = round(ms['list_logprob'] / (ms['sampled_logp'] - ms['sampled']), 3)
    print(json.dumps(row), flush=True)
    results.append(row)
    del model, U_all, packed
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
dist.destroy_process_group()
