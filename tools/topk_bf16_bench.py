"""Full-vocabulary top-k of the recommend path with the bf16 filter scan (StreamTopK scan_bf16=True: rows_bf16_norm ->
gemm_nt_topk_filter_bf16 -> cand_rescore) against the plain f32 scan at the same shape, on random rows.

usage: python tools/topk_bf16_bench.py [--B 4096] [--V 1000000] [--ds 128,64,32] [--k 100] [--rounds 5] [--calls 5]
                                       [--out FILE.json]
Per width d: the plain f32 call and the bf16 call alternate inside each round (device-event timing over `calls`
calls, two warm-up calls of each first); the median over the rounds is reported with the spread (min .. max) of both,
so a difference can be read against the noise.  The f32 path is untouched by the option: its line IS the number of the
code without it, taken in the same process.  Then the stages of the bf16 call, each timed alone on the node's own
buffers with the first chunk's thresholds -- convert (image + norms of the pool past the first chunk), scan (the
bf16 filter), re-score -- and the f32 filter launch beside the scan; the survivors per row of both filters (mean,
max; the f32 count is what an exact filter keeps, the difference is what the margin lets through); the overflow
flags; and how many rows' id lists differ between the two calls (a tail winner's value comes from the re-score's
order of adds, the f32 scan's from the matrix pipe's: scores closer than their last bits may swap places)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-recsys_amd"))
import torch  # noqa: E402
from arx import graph as G  # noqa: E402
from arx import ops  # noqa: E402
from arx.topk import StreamTopK, bf16_margin_coeff_f32  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--V", type=int, default=1000000)
ap.add_argument("--ds", default="128,64,32")
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, V, k = args.B, args.V, args.k
dev = torch.device('cuda', 0)
rt = G.Runtime(dev)
g = torch.Generator(device=dev)
g.manual_seed(0)


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


def med(x):
    return round(statistics.median(x), 4)


def survivors(node, n0):
    _, cand_v, _, _, _ = node._cand_bufs(n0, V)
    n = (cand_v != float('-inf')).sum(1).float()
    return round(float(n.mean().item()), 1), int(n.max().item())


results = []
for d in [int(x) for x in args.ds.split(",")]:
    lat, pool = Leaf((B, d), 0.3), Leaf((V, d), 0.3)
    pool.bias_value = torch.randn(V, device=dev, generator=g) * 0.1
    plain = StreamTopK(rt, lat, pool, k)
    bf = StreamTopK(rt, lat, pool, k, share=plain, scan_bf16=True)
    assert plain.fused and bf.fused
    n0 = plain.chunk
    for n in (plain, bf):                                    # warm-up
        n.forward(False)
        n.forward(False)
    torch.cuda.synchronize()
    t = [[], []]
    for _ in range(args.rounds):                             # alternated
        for i, n in enumerate((plain, bf)):
            t[i].append(timed(lambda n=n: n.forward(False), args.calls))
    ovf_p, ovf_b = plain.overflowed(), bf.overflowed()
    sv_p, sv_b = survivors(plain, n0), survivors(bf, n0)
    ip, ib = plain.indices, bf.indices
    differ = int((ip != ib).any(1).sum().item())
    vdiff = float(((plain.value - bf.value).abs() / plain.value.abs().clamp(min=1e-6)).max().item())
    # the stages, on the bf16 node's own buffers and the first chunk's thresholds
    lg = bf._buf[:, :n0]
    bias = pool.bias_value
    ops.gemm(lat.value, pool.value[:n0], lg, rt.ws, transB=True, col_bias=bias[:n0])
    rv, ri = torch.empty((B, k), device=dev), torch.empty((B, k), dtype=torch.int32, device=dev)
    ops.topk_chunk(lg, k, 0, rv, ri)
    thr = rv[:, k - 1]
    capp, cand_v, cand_i, _, _ = bf._cand_bufs(n0, V)
    img, coln = bf._bf16_bufs(V - n0, d)
    coeff = bf16_margin_coeff_f32(d)
    stages = dict(
        convert=lambda: ops.rows_bf16_norm(pool.value[n0:], img, coln),
        scan=lambda: ops.gemm_nt_topk_filter_bf16(lat.value, img, coln, bias[n0:], thr, n0, cand_v, cand_i, capp,
                                                  bf.overflow, coeff),
        rescore=lambda: ops.cand_rescore(lat.value, pool.value, bias, cand_v, cand_i),
        f32_scan=lambda: ops.gemm_nt_topk_filter(lat.value, pool.value[n0:], bias[n0:], thr, n0, cand_v, cand_i, capp,
                                                 bf.overflow))
    st = {}
    for name in ('convert', 'scan', 'rescore', 'f32_scan'):
        ops.fill_f32(cand_v.view(-1), float('-inf'))
        if name == 'rescore':
            stages['scan']()
        stages[name]()
        torch.cuda.synchronize()
        st[name] = med([timed(stages[name], args.calls) for _ in range(args.rounds)])
    mp, mb = med(t[0]), med(t[1])
    row = dict(B=B, V=V, d=d, k=k, chunk=n0, plain_ms=mp, bf16_ms=mb, ratio=round(mb / mp, 4),
               plain_ms_all=[round(x, 4) for x in t[0]], bf16_ms_all=[round(x, 4) for x in t[1]],
               plain_spread_ms=round(max(t[0]) - min(t[0]), 4), bf16_spread_ms=round(max(t[1]) - min(t[1]), 4),
               convert_ms=st['convert'], scan_ms=st['scan'], rescore_ms=st['rescore'], f32_scan_ms=st['f32_scan'],
               survivors_f32_mean=sv_p[0], survivors_f32_max=sv_p[1], survivors_bf16_mean=sv_b[0],
               survivors_bf16_max=sv_b[1], segment_slots=int(cand_v.shape[1]), plain_overflow=ovf_p,
               bf16_overflow=ovf_b, rows_with_other_ids=differ, max_rel_value_diff=vdiff)
    results.append(row)
    print("d %-4d plain %8.3f ms (%.3f..%.3f)  bf16 %8.3f ms (%.3f..%.3f)  x%.3f | convert %.3f  scan %.3f  re-score "
          "%.3f  (f32 scan %.3f) | survivors/row f32 %.1f max %d, bf16 %.1f max %d of %d slots | overflow %d/%d | "
          "rows with other ids %d, max rel value diff %.2e"
          % (d, mp, min(t[0]), max(t[0]), mb, min(t[1]), max(t[1]), mb / mp, st['convert'], st['scan'], st['rescore'],
             st['f32_scan'], sv_p[0], sv_p[1], sv_b[0], sv_b[1], int(cand_v.shape[1]), ovf_p, ovf_b, differ, vdiff))
    del plain, bf, lat, pool, img, coln, cand_v, cand_i, lg
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
