"""The sampled recommend of the row-sharded model (ShardedHMF.recommend_sampled) at world 1:
plain, sampled and sampled + propensities at one shape, and the keyed fused sampling scan (arx_sample_shard.h: noise
column c * W + s, noise row a user id) beside the un-keyed one.

usage: python tools/sharded_sample_bench.py [--B 4096] [--V 1000000] [--d 128,64] [--k 100] [--tau 1.0]
                                            [--rounds 5] [--calls 3] [--out FILE.json]
World 1 is an nccl group of one on cuda:0.  The three recommend calls alternate inside each round, as do the two
scans and the two filter launches (device-event timing, one warm-up round first); the median per call is reported.
The recommend figures are whole calls: host checks, the feeds, every launch and the clone of the result.  The scan is
TopKScan.run(sample=, strip=False) over the whole table; the filter launch alone is arx_gemm_nt_topk_filter_sample
(_keyed) over the columns past the first chunk against each row's final k-th key as its threshold."""
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
from arx.topk import TopKScan, sample_params  # noqa: E402

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
os.environ.setdefault("MASTER_PORT", "29795")
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
CH = 65536


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
    seed = [0]

    def sampled(**kw):
        seed[0] += 1
        return model.recommend_sampled(users, k, sample_temperature=tau, sample_seed=seed[0], **kw)
    rec = alternate({'plain': lambda: model.recommend(users, k), 'sampled': sampled,
                     'sampled_logp': lambda: sampled(return_logprob=True)})
    scan_s = next(s for key, s in model.be._scans.items() if key[-1] is False)
    overflow = int(scan_s.overflow.item())

    # the scan and the filter launch alone: un-keyed beside keyed (shard 2 of 3, random user ids)
    U = torch.from_numpy(tabs['user']).to(dev)
    E, bias = model.E_item[:V], model.b_item[:V]
    tf, words = sample_params(tau, 7, B)
    plain_s = (torch.from_numpy(tf).to(dev), B, torch.from_numpy(words).to(dev))
    ids = torch.from_numpy(rng.integers(0, 2 ** 31, B).astype(np.int32)).to(dev)
    keyed_s = plain_s + (3, 2, ids)
    scan = TopKScan(B, V, d, k, dev)
    ws = ops.Workspace(dev)
    vo = torch.empty((B, k), dtype=torch.float32, device=dev)
    io = torch.empty((B, k), dtype=torch.int32, device=dev)
    run = lambda s: scan.run(U, E, bias, ws, vo, io, sample=s, strip=False)
    sc = alternate({'scan_unkeyed': lambda: run(plain_s), 'scan_keyed': lambda: run(keyed_s)})
    flt = {}
    if scan.fused and V > CH:
        capp, cand_v, cand_i, cpos, parts = scan._cand_bufs(CH, V)
        thr = {}
        for name, s in (('unkeyed', plain_s), ('keyed', keyed_s)):
            run(s)
            thr[name] = vo[:, k - 1].clone()

        def launch(name, s):
            ops.fill_f32(cand_v.view(-1), float('-inf'))
            ops.fill_i32(scan.overflow, 0)
            ops.gemm_nt_topk_filter_sample(U, E[CH:], bias[CH:], thr[name], CH, cand_v, cand_i, capp, scan.overflow, s)
        flt = alternate({'filter_unkeyed': lambda: launch('unkeyed', plain_s),
                         'filter_keyed': lambda: launch('keyed', keyed_s)})
    row = dict(B=B, V=V, d=d, k=k, tau=args.tau, overflow=overflow, **{n + '_ms': round(v, 4) for n, v in
                                                                      {**rec, **sc, **flt}.items()})
    row['sampled_over_plain'] = round(rec['sampled'] / rec['plain'], 3)
    row['logp_over_sampled'] = round(rec['sampled_logp'] / rec['sampled'], 3)
    row['scan_keyed_over_unkeyed'] = round(sc['scan_keyed'] / sc['scan_unkeyed'], 3)
    if flt:
        row['filter_keyed_over_unkeyed'] = round(flt['filter_keyed'] / flt['filter_unkeyed'], 3)
    print(json.dumps(row), flush=True)
    results.append(row)
    del model, scan, U, E, bias
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
dist.destroy_process_group()
