"""Full-vocabulary top-k of the recommend path within item tags (StreamTopK tags=), fused and chunked, against the
plain scan at the same shape, on random rows.

usage: python tools/topk_tags_bench.py [--B 4096] [--V 1000000] [--d 128] [--k 100] [--shares 0.5,0.05,0.005]
                                       [--H 200] [--rounds 3] [--calls 5] [--out FILE.json]
Every column carries bit j with probability shares[j]; every row asks for tags_any = 1 << j, so its eligible share
is shares[j].  Each share runs without exclusion lists and with the row's own H best columns excluded (adversarial:
what a trained model produces).  Plain and filtered calls alternate inside each round (device-event timing, warm-up
first); the median per call is reported with the overflow flag of the fused run (an overflowing request is re-run
on the chunked path by the models: the `chunked` rows are what it then costs) and the time of the exclusion-only
scan beside it."""
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
ap.add_argument("--shares", default="0.5,0.05,0.005")
ap.add_argument("--H", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, V, d, k, H = args.B, args.V, args.d, args.k, args.H
shares = [float(x) for x in args.shares.split(",")]
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
col_tags = torch.zeros(V, dtype=torch.int32, device=dev)
for j, p in enumerate(shares):
    col_tags |= (torch.rand(V, device=dev, generator=g) < p).to(torch.int32) << j
zero = torch.zeros(B, dtype=torch.int32, device=dev)

top = StreamTopK(rt, lat, pool, H)                          # the rows' own H best columns
run_complete(top, lambda: top.forward(False))
own_best = top.indices.clone()
del top
ex = (keys, B, torch.arange(B + 1, dtype=torch.int32, device=dev) * H,
      torch.sort(own_best, dim=1).values.contiguous().view(-1))


def timed(node, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        node.forward(False)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


results = []
for j, share in enumerate(shares):
    tags = (col_tags, torch.full((B,), 1 << j, dtype=torch.int32, device=dev), zero, B)
    for with_ex in (False, True):
        for mode in ('fused', 'chunked'):
            plain = StreamTopK(rt, lat, pool, k)
            excl = StreamTopK(rt, lat, pool, k, exclude=lambda: ex, share=plain)
            filt = StreamTopK(rt, lat, pool, k, exclude=(lambda: ex) if with_ex else None, share=plain,
                              tags=lambda tags=tags: tags)
            nodes = (plain, excl, filt)
            for n in nodes:                                # warm-up
                n.fused = mode == 'fused'
                n.forward(False)
                n.forward(False)
            torch.cuda.synchronize()
            t = [[], [], []]
            for _ in range(args.rounds):                   # alternated
                for i, n in enumerate(nodes):
                    t[i].append(timed(n, args.calls))
            ovf_p, ovf_f = plain.overflowed(), filt.overflowed()
            # correctness spot check: only eligible (and no excluded) columns in the result
            idx = filt.indices[:64].long()
            ok = idx >= 0
            bad = bool((((col_tags[idx.clamp(min=0)] >> j) & 1) == 0)[ok].any().item())
            if with_ex:
                bad = bad or bool((idx[:, :, None] == own_best[:64, None, :].long()).any().item())
            mp, me, mf = (statistics.median(x) for x in t)
            row = dict(B=B, V=V, d=d, k=k, share=share, H=H if with_ex else 0, mode=mode, plain_ms=round(mp, 4),
                       excl_ms=round(me, 4), tags_ms=round(mf, 4), ratio=round(mf / mp, 4),
                       ratio_to_excl=round(mf / me, 4), plain_overflow=ovf_p, tags_overflow=ovf_f,
                       wrong_column_in_result=bad, short_rows=int((~ok).any(1).sum().item()),
                       plain_ms_all=[round(x, 4) for x in t[0]], tags_ms_all=[round(x, 4) for x in t[2]])
            results.append(row)
            print("share %-6g ex %-3d %-7s plain %8.3f ms  excl-only %8.3f ms  tags %8.3f ms  x%.3f  overflow %d/%d%s"
                  % (share, row['H'], mode, mp, me, mf, mf / mp, ovf_p, ovf_f,
                     "  WRONG COLUMN IN RESULT" if bad else ""))
            del plain, excl, filt, nodes
            torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
