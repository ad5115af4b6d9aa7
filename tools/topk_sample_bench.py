"""Full-vocabulary SAMPLED top-k of the recommend path (StreamTopK sample=: k draws without replacement from
softmax(score / tau) as the top-k of Gumbel keys), fused and chunked, against the plain scan at the same shape and
against a torch composition, on random rows.

usage: python tools/topk_sample_bench.py [--B 4096] [--V 1000000] [--d 128,64,32] [--k 100] [--taus 0.1,1]
                                         [--rounds 3] [--calls 3] [--out FILE.json]
The torch composition: chunks of 65536 columns, lat @ pool[c].T + b + tau * (-log(-log(rand))), topk, then cat + topk
over the chunks' winners.  Plain, sampled-fused, sampled-chunked and torch calls alternate inside each round
(device-event timing, warm-up first); the median per call is reported with the overflow flag of the fused run (an
overflowing request is re-run on the chunked path by the models: the `chunked` figure is what it then costs) and the
share of rows whose ids agree between the two paths (the two GEMMs differ in the last place of some logits at large
batches, which swaps near-tied neighbours in a few rows per thousand, as it does in the plain scan)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-recsys_amd"))
import torch  # noqa: E402
from arx import graph as G  # noqa: E402
from arx.topk import StreamTopK, sample_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--V", type=int, default=1000000)
ap.add_argument("--d", default="128,64,32")
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--taus", default="0.1,1")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, V, k = args.B, args.V, args.k
dev = torch.device('cuda', 0)
rt = G.Runtime(dev)
g = torch.Generator(device=dev)
g.manual_seed(0)
CH = 65536


class Leaf(G.Node):
    def __init__(self, shape, scale):
        super().__init__(rt, shape)
        self.value = torch.randn(shape, device=dev, generator=g) * scale
        self.bias_value = None


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


results = []
for d in [int(x) for x in args.d.split(",")]:
    lat, pool = Leaf((B, d), 0.3), Leaf((V, d), 0.3)
    pool.bias_value = torch.randn(V, device=dev, generator=g) * 0.1
    for tau in [float(x) for x in args.taus.split(",")]:
        tf, words = sample_params(tau, 12345, B)
        sargs = (torch.from_numpy(tf).to(dev), B, torch.from_numpy(words).to(dev))
        plain = StreamTopK(rt, lat, pool, k)
        fused = StreamTopK(rt, lat, pool, k, share=plain, sample=lambda sargs=sargs: sargs)
        chunked = StreamTopK(rt, lat, pool, k, share=plain, sample=lambda sargs=sargs: sargs)
        chunked.fused = False
        buf = plain._buf

        def composed():
            vs, ids = [], []
            for c0 in range(0, V, CH):
                c1 = min(V, c0 + CH)
                x = torch.addmm(pool.bias_value[c0:c1], lat.value, pool.value[c0:c1].T, out=buf[:, :c1 - c0])
                x.add_(torch.rand_like(x).log_().neg_().log_().neg_(), alpha=tau)
                v, i = torch.topk(x, min(k, c1 - c0), dim=1)
                vs.append(v)
                ids.append(i + c0)
            v, j = torch.topk(torch.cat(vs, 1), k, dim=1)
            return v, torch.gather(torch.cat(ids, 1), 1, j)

        fns = (lambda: plain.forward(False), lambda: fused.forward(False), lambda: chunked.forward(False), composed)
        for f in fns:                                      # warm-up
            f()
            f()
        torch.cuda.synchronize()
        t = [[], [], [], []]
        for _ in range(args.rounds):                       # alternated
            for i, f in enumerate(fns):
                t[i].append(timed(f, args.calls))
        ovf_p, ovf_f = plain.overflowed(), fused.overflowed()
        same = round(float((fused.indices == chunked.indices).all(1).float().mean().item()), 5) if not ovf_f else None
        mp, mf, mc, mt = (statistics.median(x) for x in t)
        row = dict(B=B, V=V, d=d, k=k, tau=tau, plain_ms=round(mp, 4), sampled_fused_ms=round(mf, 4),
                   sampled_chunked_ms=round(mc, 4), torch_ms=round(mt, 4), ratio_to_plain=round(mf / mp, 4),
                   torch_over_fused=round(mt / mf, 4), plain_overflow=ovf_p, sampled_overflow=ovf_f,
                   rows_fused_equals_chunked=same, in_plain_topk_share=round(float(
                       (fused.indices[:64, :, None] == plain.indices[:64, None, :]).any(2).float().mean().item()), 4),
                   **{n + '_ms_all': [round(x, 4) for x in t[i]]
                      for i, n in enumerate(('plain', 'sampled_fused', 'sampled_chunked', 'torch'))})
        results.append(row)
        print("d %-4d tau %-5g plain %8.3f ms  sampled fused %8.3f ms (x%.3f)  chunked %8.3f ms  torch %8.3f ms  "
              "overflow %d/%d  rows fused == chunked %s" % (d, tau, mp, mf, mf / mp, mc, mt, ovf_p, ovf_f, same))
        del plain, fused, chunked, fns, buf
        torch.cuda.empty_cache()
    del lat, pool
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
