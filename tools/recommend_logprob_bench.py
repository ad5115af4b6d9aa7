"""The propensities of the sampled recommend (StreamTopK sample=, logp=True: arx_sample_logp.h) against the sampled
recommend alone and against a torch composition of the same quantity, on random rows.

usage: python tools/recommend_logprob_bench.py [--B 4096] [--V 1000000] [--d 128,64,32] [--k 100] [--tau 1]
                                               [--rounds 3] [--calls 3] [--check-rows 16] [--out FILE.json]
The torch composition, given the picks: chunks of 65536 columns, lat @ pool[c].T + b, the picks' columns set to -inf
(scatter; a spare column takes the picks of other chunks), logsumexp of the chunk / tau, the chunks joined by
logaddexp; then the picks' scores / tau in reverse selection order through logcumsumexp on top of the rest, and the
difference.  (Exclusion lists and tags would add a mask per chunk to it; the timed call has none, which favours
torch.)  Sampled, sampled + logp (fused: one streaming mass pass; chunked: the second sweep) and torch calls alternate
inside each round (device-event timing, warm-up first); the median per call is reported, with the largest
|logp - float64| / tolerance over --check-rows rows at full size (the float64 reference on the host from the device's
own logits of those rows; tolerance: tests/recommend_logprob_oracle.py)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-recsys_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from arx import graph as G  # noqa: E402
from arx import ops  # noqa: E402
from arx.topk import StreamTopK, sample_params  # noqa: E402
import recommend_logprob_oracle as RL  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--V", type=int, default=1000000)
ap.add_argument("--d", default="128,64,32")
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--tau", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--check-rows", type=int, default=16)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, V, k, tau = args.B, args.V, args.k, args.tau
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
    tf, words = sample_params(tau, 12345, B)
    sargs = (torch.from_numpy(tf).to(dev), B, torch.from_numpy(words).to(dev))
    sampled = StreamTopK(rt, lat, pool, k, sample=lambda: sargs)
    fused = StreamTopK(rt, lat, pool, k, share=sampled, sample=lambda: sargs, logp=True)
    chunked = StreamTopK(rt, lat, pool, k, share=sampled, sample=lambda: sargs, logp=True)
    chunked.fused = False
    xbuf = torch.empty((B, CH + 1), device=dev)
    sampled.forward(False)
    picks = sampled.indices.long()

    def composed():
        rest = torch.full((B,), float('-inf'), device=dev)
        sc = torch.empty((B, k), device=dev)
        for c0 in range(0, V, CH):
            c1 = min(V, c0 + CH)
            w = c1 - c0
            x = xbuf[:, :w + 1]                        # one spare column of -inf: where the picks outside the chunk go
            torch.addmm(pool.bias_value[c0:c1], lat.value, pool.value[c0:c1].T, out=xbuf[:, :w])
            x[:, w] = float('-inf')
            inside = (picks >= c0) & (picks < c1)
            loc = torch.where(inside, picks - c0, torch.full_like(picks, w))
            sc = torch.where(inside, torch.gather(x, 1, loc), sc)
            x.scatter_(1, loc, float('-inf'))
            rest = torch.logaddexp(rest, torch.logsumexp(x / tau, 1))
        a = sc / tau
        suffix = torch.logcumsumexp(torch.cat([rest[:, None], a.flip(1)], 1), 1)[:, 1:].flip(1)
        return a - suffix

    fns = (lambda: sampled.forward(False), lambda: fused.forward(False), lambda: chunked.forward(False), composed)
    for f in fns:                                      # warm-up
        f()
        f()
    torch.cuda.synchronize()
    t = [[], [], [], []]
    for _ in range(args.rounds):                       # alternated
        for i, f in enumerate(fns):
            t[i].append(timed(f, args.calls))
    ms, mf, mc, mt = (statistics.median(x) for x in t)
    # accuracy at full size: the device's own logits of a few rows, float64 on the host
    rows = np.linspace(0, B - 1, min(B, args.check_rows)).astype(np.int64)
    L = np.empty((len(rows), V), dtype=np.float32)
    lr = lat.value[torch.from_numpy(rows).to(dev)].contiguous()
    for c0 in range(0, V, CH):
        c1 = min(V, c0 + CH)
        x = torch.empty((len(rows), c1 - c0), device=dev)
        ops.gemm(lr, pool.value[c0:c1], x, rt.ws, transB=True, col_bias=pool.bias_value[c0:c1])
        L[:, c0:c1] = x.cpu().numpy()
    elig = np.ones(L.shape, dtype=bool)
    tr = np.full(len(rows), tau)
    worst = {}
    for name, node in (('fused', fused), ('chunked', chunked)):
        gi, glp = node.indices.cpu().numpy()[rows], node.logp.cpu().numpy()[rows]
        exp = RL.logp(L, elig, gi, tr)
        worst[name] = round(RL.worst(glp, exp, RL.tolerance(L, elig, tr, exp)), 4)
    tdiff = float((composed() - fused.logp).abs().max().item())
    row = dict(B=B, V=V, d=d, k=k, tau=tau, sampled_ms=round(ms, 4), logp_fused_ms=round(mf, 4),
               logp_chunked_ms=round(mc, 4), torch_logp_only_ms=round(mt, 4), ratio_to_sampled=round(mf / ms, 4),
               mass_pass_ms=round(mf - ms, 4), torch_over_mass_pass=round(mt / max(mf - ms, 1e-9), 4),
               overflow=fused.overflowed(), ids_equal=bool((fused.indices == sampled.indices).all().item()),
               worst_err_over_tol=worst, torch_minus_device_max=tdiff,
               **{n + '_ms_all': [round(x, 4) for x in t[i]]
                  for i, n in enumerate(('sampled', 'logp_fused', 'logp_chunked', 'torch_logp_only'))})
    results.append(row)
    print("d %-4d sampled %8.3f ms  + logp fused %8.3f ms (x%.3f)  chunked %8.3f ms  torch (logp only) %8.3f ms  "
          "err/tol %s  |torch - device| %.2g" % (d, ms, mf, mf / ms, mc, mt, worst, tdiff))
    del sampled, fused, chunked, fns, xbuf
    torch.cuda.empty_cache()
    del lat, pool
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
