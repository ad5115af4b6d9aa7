"""similar_items next to the recommend scan at the same shape: B query rows against a V x d item table, k winners,
on plain tensors (topk.TopKScan, the scan both model families run).  Run by hand on the MI355X; not part of bench.py.

  recommend : TopKScan.run(latent, table, bias)            -- first chunk GEMM + select, the fused filter GEMM, merge
  similar   : topk.similar_scan(scan, table, rows, ...)    -- arx_rows_inv_norm over the table, arx_gather_rows_unit,
              then the same scan with the cosine scale (arx_cos_chunk_finish, arx_gemm_nt_topk_filter_cos)
  inv_norm  : the norm pass alone (one streaming read of the table; GB/s = V * d * 4 / time)

HIP events around --steps calls, --warmup calls of each first, the median of --repeats regions, the three alternating
region by region.  The expectation from the code: similar = recommend + the norm pass (+ the finish of the first chunk).

usage: python tools/similar_bench.py [--steps 10] [--warmup 3] [--repeats 11] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'a-recsys_amd'), ROOT]

import torch  # noqa: E402

SHAPES = [(4096, 1000000, 128, 100), (256, 200000, 64, 100)]         # (B, V, d, k)


def region_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def bench_shape(dev, B, V, d, k, args):
    from arx import ops
    from arx.topk import TopKScan, similar_scan
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    table = torch.randn(V, d, device=dev, generator=g) * 0.3
    bias = torch.randn(V, device=dev, generator=g) * 0.1
    latent = torch.randn(B, d, device=dev, generator=g) * 0.3
    rows = torch.randint(0, V, (B,), device=dev, generator=g, dtype=torch.int32)
    ws = ops.Workspace(dev)
    rec, sim = TopKScan(B, V, d, k, dev), TopKScan(B, V, d, k, dev)
    rv, ri = torch.empty((B, k), device=dev), torch.empty((B, k), dtype=torch.int32, device=dev)
    sv, si = torch.empty((B, k), device=dev), torch.empty((B, k), dtype=torch.int32, device=dev)
    inv = torch.empty(V, device=dev)
    fns = {'recommend': lambda: rec.run(latent, table, bias, ws, rv, ri),
           'similar': lambda: similar_scan(sim, table, rows, sv, si, ws, False),
           'inv_norm': lambda: ops.rows_inv_norm(table, inv)}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    # complete results only: neither scan may have overflowed at this shape (similar_scan would have re-run chunked)
    flags = {'recommend': int(rec.overflow.item()), 'similar': int(sim.overflow.item())}
    times = {n: [] for n in fns}
    for _ in range(args.repeats):
        for n, fn in fns.items():
            times[n].append(region_ms(fn, args.steps))
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    out = {'B': B, 'V': V, 'd': d, 'k': k, 'fused': bool(rec.fused and sim.fused), 'overflow': flags,
           'ms': {n: round(v, 4) for n, v in med.items()},
           'ms_min_max': {n: [round(min(t), 4), round(max(t), 4)] for n, t in times.items()},
           'similar_over_recommend': round(med['similar'] / med['recommend'], 4),
           'inv_norm_gbs': round(V * d * 4 / med['inv_norm'] / 1e6, 1),
           'recommend_tflops': round(2.0 * B * V * d / med['recommend'] / 1e9, 2),
           'self_excluded': bool((si != rows[:, None]).all().item())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=11)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("similar_bench: needs the GPU (no CPU path, nothing to time without it)")
    dev = torch.device('cuda:0')
    res = []
    for B, V, d, k in SHAPES:
        r = bench_shape(dev, B, V, d, k, args)
        print(json.dumps(r), flush=True)
        res.append(r)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
