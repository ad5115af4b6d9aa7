"""Full-vocabulary recommend of the row-sharded HMF model (arx.dist.ShardedHMF.recommend) against StreamTopK, the
single-GPU recommend, at the same shape and in the same process; then the C5 shape (100 M items x d 128).

usage: python tools/sharded_recommend_bench.py [--B 4096] [--V 1000000] [--d 128] [--k 100] [--H 0,20,200]
                                               [--c5-V 100000000] [--c5-B 4096] [--no-c5] [--out FILE.json]
       python -m torch.distributed.run --nproc_per_node N tools/sharded_recommend_bench.py ...   (RCCL, N ranks)
B is the global number of users per call (B / N per rank), V the number of items; H columns of history per user are
excluded (H = 0: exclude_seen off).  Per shape: ms per recommend call (median of the rounds, device events around
`--calls` calls, each call with its host side: the overflow read of the fused top-k and the result copy), the shares
of the local stage (backend.shard_topk: scoring GEMM + top-k) and of the merge (arx_topk_merge_shards) -- both timed
alone on the call's own buffers --, and the scoring GEMM's FLOP/s (2 B V d / local-stage time, per rank: V / N
columns) as a fraction of the 155 TF FP32-MFMA peak of the MI355X.  At world 1 the StreamTopK call on the same
latents, table and exclusion lists is timed alternately with recommend."""
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
from arx import graph as G  # noqa: E402
from arx.dist import ShardedHMF  # noqa: E402
from arx.topk import StreamTopK, run_complete  # noqa: E402

PEAK_F32_MFMA = 155e12

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--V", type=int, default=1000000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--H", default="0,20,200")
ap.add_argument("--c5-V", type=int, default=100000000)
ap.add_argument("--c5-B", type=int, default=4096)
ap.add_argument("--no-c5", action="store_true")
ap.add_argument("--only-c5", action="store_true")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

if "RANK" in os.environ:
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", 0))
else:
    rank, world, local = 0, 1, 0
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29781")
torch.cuda.set_device(local)
dev = torch.device('cuda', local)
dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def bench_shape(V, B, d, k, Hs, with_stream, calls, rounds):
    B_loc = B // world
    model = ShardedHMF(B, V, d, B_loc, 64, 0.1, rank, world, dev, seed=1, graphs=False)
    users = np.arange(rank, B, world)[:B_loc]
    rng = np.random.default_rng(100 + rank)
    rows = []
    for H in Hs:
        if H > 0:
            model.prepare_recommend_exclusions({int(u): rng.integers(0, V, size=H).tolist() for u in users})
        rec = lambda: model.recommend(users, k, exclude_seen=H > 0)
        rec()
        rec()
        torch.cuda.synchronize()
        keys_loc, U_loc, keys_all, U_all = model._rec_lat
        out_v, out_i, recv_v, recv_c, vo, io = model._rec_k[k]
        ni = model.ni_loc
        ex = (keys_all, B, model._rec_ex[0], model._rec_ex[1]) if H > 0 else None
        local_stage = lambda: model.be.shard_topk(U_all, model.E_item[:ni], model.b_item[:ni], k, ex, out_v, out_i)
        rv, rc = (recv_v, recv_c) if world > 1 else (out_v.view(1, B, k), out_i.view(1, B, k))
        merge = lambda: model.be.topk_merge_shards(rv, rc, vo, io)
        st = None
        if with_stream and world == 1:
            rt = G.Runtime(dev)

            class Leaf(G.Node):
                def __init__(self, t, bias=None):
                    super().__init__(rt, tuple(t.shape))
                    self.value, self.bias_value = t, bias
            st = StreamTopK(rt, Leaf(U_all), Leaf(model.E_item[:ni], model.b_item[:ni]), k,
                            exclude=(lambda: ex) if ex is not None else None)

            def stream_call():
                run_complete(st, lambda: st.forward(False))
                st.indices.clone()
            stream_call()
        t_rec, t_st, t_loc, t_mrg = [], [], [], []
        for _ in range(rounds):
            t_rec.append(events_ms(rec, calls))
            if st is not None:
                t_st.append(events_ms(stream_call, calls))
            t_loc.append(events_ms(local_stage, calls))
            t_mrg.append(events_ms(merge, calls))
        ms, ml, mm = statistics.median(t_rec), statistics.median(t_loc), statistics.median(t_mrg)
        row = dict(world=world, rank=rank, B=B, V=V, d=d, k=k, H=H, recommend_ms=round(ms, 4),
                   local_stage_ms=round(ml, 4), merge_ms=round(mm, 5), local_share=round(ml / ms, 4),
                   merge_share=round(mm / ms, 5), gemm_tflops=round(2.0 * B * ni * d / (ml * 1e-3) / 1e12, 2),
                   gemm_frac_of_155tf=round(2.0 * B * ni * d / (ml * 1e-3) / PEAK_F32_MFMA, 4),
                   recommend_ms_all=[round(x, 4) for x in t_rec])
        if st is not None:
            mst = statistics.median(t_st)
            row.update(stream_topk_ms=round(mst, 4), ratio_vs_stream_topk=round(ms / mst, 4),
                       stream_topk_ms_all=[round(x, 4) for x in t_st])
            same = torch.equal(model.recommend(users, k, exclude_seen=H > 0), st.indices[:len(users)])
            row['same_ids_as_stream_topk'] = bool(same)
        rows.append(row)
        if rank == 0:
            print("V=%-10d B=%-5d H=%-4d recommend %9.3f ms  local %5.1f%%  merge %6.3f%% (%.4f ms)  GEMM %.1f TF "
                  "(%.0f%% of 155)%s" % (V, B, H, ms, 100 * ml / ms, 100 * mm / ms, mm,
                                         row['gemm_tflops'], 100 * row['gemm_frac_of_155tf'],
                                         "  StreamTopK %.3f ms  x%.3f  same ids %s" % (
                                             row['stream_topk_ms'], row['ratio_vs_stream_topk'],
                                             row['same_ids_as_stream_topk']) if st is not None else ""), flush=True)
        del st
    del model
    torch.cuda.empty_cache()
    return rows


results = []
if not args.only_c5:
    results += bench_shape(args.V, args.B, args.d, args.k, [int(x) for x in args.H.split(",")], True, args.calls,
                           args.rounds)
if not args.no_c5:
    results += bench_shape(args.c5_V, args.c5_B, 128, args.k, [0], False, 2, 1)
if args.out and rank == 0:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
dist.destroy_process_group()
