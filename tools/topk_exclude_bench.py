"""Full-vocabulary top-k of the recommend path with each row's seen items excluded (StreamTopK exclude=), fused and
chunked, against the same calls without exclusion, on random rows.

usage: python tools/topk_exclude_bench.py [--B 4096] [--V 1000000] [--d 128] [--k 100] [--H 20,200] [--rounds 3]
                                          [--out FILE.json]
History draws per row (H columns each):
  uniform      H random columns over the whole vocabulary;
  adversarial  the row's own H best columns (what a trained model produces: every one of them would have been a
               winner, so the threshold of the fused path drops to the (k + H)-th best score).
Plain and excluding calls alternate inside each round (device-event timing, warm-up first); the median per call is
reported with the overflow flag of the fused run (an overflowing request is re-run on the chunked path by the
models)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-recsys_amd"))
import torch  # noqa: E402
from arx import graph as G  # noqa: E402
from arx.topk import StreamTopK, run_complete  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--V", type=int, default=1000000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--H", default="20,200")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, V, d, k = args.B, args.V, args.d, args.k
dev = torch.device('cuda', 0)
rt = G.Runtime(dev)
g = torch.Generator(device=dev)
g.manual_seed(0)


class Leaf(G.Node):
    def __init__(self, shape, scale):
        super().__init__(rt, shape)
        self.value = torch.randn(shape, device=dev, generator=g) * scale
        self.bias_value = None


lat, pool = Leaf((B, d), 0.3), Leaf((V, d), 0.3)
pool.bias_value = torch.randn(V, device=dev, generator=g) * 0.1
keys = torch.arange(B, dtype=torch.int32, device=dev)


def lists_of(cols):
    """[B, H] columns (row r = user r) -> the exclusion tuple (row_keys, key_rows, ex_ptr, ex_cols)"""
    H = cols.shape[1]
    srt = torch.sort(cols.to(torch.int32), dim=1).values.contiguous()
    ptr = torch.arange(B + 1, dtype=torch.int32, device=dev) * H
    return (keys, B, ptr, srt.view(-1))


def timed(node, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        node.forward(False)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


results = []
for H in [int(x) for x in args.H.split(",")]:
    draws = {'uniform': torch.randint(0, V, (B, H), device=dev, generator=g)}
    top = StreamTopK(rt, lat, pool, H)                      # the rows' own H best columns
    run_complete(top, lambda: top.forward(False))
    draws['adversarial'] = top.indices.clone()
    del top
    for draw, cols in draws.items():
        ex = lists_of(cols)
        for mode in ('fused', 'chunked'):
            plain = StreamTopK(rt, lat, pool, k)
            excl = StreamTopK(rt, lat, pool, k, exclude=lambda ex=ex: ex, share=plain)
            plain.fused = excl.fused = mode == 'fused'
            for n in (plain, excl):                        # warm-up
                n.forward(False)
                n.forward(False)
            torch.cuda.synchronize()
            tp, te = [], []
            for _ in range(args.rounds):                   # alternated
                tp.append(timed(plain, args.calls))
                te.append(timed(excl, args.calls))
            ovf_p, ovf_e = plain.overflowed(), excl.overflowed()
            # correctness spot check: no excluded column in the result
            hit = bool((excl.indices[:64, :, None].long() == cols[:64, None, :].long()).any().item())
            mp, me = statistics.median(tp), statistics.median(te)
            row = dict(B=B, V=V, d=d, k=k, H=H, draw=draw, mode=mode, plain_ms=round(mp, 4), excl_ms=round(me, 4),
                       ratio=round(me / mp, 4), plain_overflow=ovf_p, excl_overflow=ovf_e, excluded_in_result=hit,
                       plain_ms_all=[round(x, 4) for x in tp], excl_ms_all=[round(x, 4) for x in te])
            results.append(row)
            print("H=%-4d %-11s %-7s plain %8.3f ms  excl %8.3f ms  x%.3f  overflow %d/%d%s" % (
                H, draw, mode, mp, me, me / mp, ovf_p, ovf_e, "  EXCLUDED COLUMN IN RESULT" if hit else ""))
            del plain, excl
            torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
