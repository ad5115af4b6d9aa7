"""score_items' scoring kernel next to the only formulation a user had without it, at the same shape: B rows, each with
its own slate of C candidates out of a V x d item pool, on plain tensors.  Run by hand on the MI355X; not part of
bench.py.

  slate   : ops.slate_scores(U, P, b, cand, out)                       -- arx_slate_scores, one launch
  order   : slate + arx.slate.slate_order(out, cand, k, ...)           -- the (ids, values) form of score_items
  torch   : (P[cand] * U[:, None, :]).sum(-1) + b[cand]                -- the torch composition; it reads the same rows
            and additionally writes and re-reads B * C * d * 4 bytes
  scan    : TopKScan.run(U, P, b)                                      -- the full-vocabulary recommend scan at the same
            B, as a scale (what one paid for "the model's scores" before: a [B, V] pass that keeps k <= 1024 of them)

Two candidate laws: 'uniform' over V (rows come from HBM) and 'shared' (one slate for all rows: rows come from L2).
HIP events around --calls calls, a warm-up of each first; inside each of the --rounds rounds the forms alternate; the
median over the rounds is reported per call, with the EFFECTIVE rate B * C * (4 d + 12) / t (the pool row, the
candidate id, the bias and the score of every slot; U is not counted) and its share of the 6.29 TB/s measured copy
rate of the chip.

usage: python tools/slate_bench.py [--B 4096] [--V 1000000] [--d 128] [--C 100,1000] [--k 10] [--rounds 3]
                                   [--calls 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'a-recsys_amd'), ROOT]

import torch  # noqa: E402

COPY_TBS = 6.29


def region_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def bench(dev, B, V, d, C, k, law, tensors, args):
    from arx import ops
    from arx.slate import slate_order
    from arx.topk import TopKScan
    U, P, b, ws = tensors
    g = torch.Generator(device=dev)
    g.manual_seed(C)
    if law == 'uniform':
        cand = torch.randint(0, V, (B, C), device=dev, generator=g, dtype=torch.int32)
    else:
        cand = torch.randint(0, V, (1, C), device=dev, generator=g, dtype=torch.int32).repeat(B, 1).contiguous()
    cl = cand.long()
    out = torch.empty((B, C), device=dev)
    kk = min(k, C)
    vals, pos, ids = (torch.empty((B, kk), device=dev), torch.empty((B, kk), dtype=torch.int32, device=dev),
                      torch.empty((B, kk), dtype=torch.int32, device=dev))
    scan = TopKScan(B, V, d, kk, dev)
    sv, si = torch.empty((B, kk), device=dev), torch.empty((B, kk), dtype=torch.int32, device=dev)
    ref = [None]

    def f_torch():
        ref[0] = (P[cl] * U[:, None, :]).sum(-1) + b[cl]

    def f_order():
        ops.slate_scores(U, P, b, cand, out)
        slate_order(out, cand, kk, vals, pos, ids)
    fns = {'slate': lambda: ops.slate_scores(U, P, b, cand, out), 'order': f_order, 'torch': f_torch,
           'scan': lambda: scan.run(U, P, b, ws, sv, si)}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    err = float((out - ref[0]).abs().max().item())
    ref[0] = None
    times = {n: [] for n in fns}
    for _ in range(args.rounds):
        for n, fn in fns.items():
            times[n].append(region_ms(fn, args.calls))
    ref[0] = None
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    nbytes = B * C * (4 * d + 12)
    rate = {n: nbytes / med[n] / 1e9 for n in ('slate', 'torch')}           # TB/s (bytes / ms / 1e9)
    return {'B': B, 'V': V, 'd': d, 'C': C, 'k': kk, 'law': law, 'bytes': nbytes,
            'ms': {n: round(v, 4) for n, v in med.items()},
            'ms_min_max': {n: [round(min(t), 4), round(max(t), 4)] for n, t in times.items()},
            'effective_tbs': {n: round(v, 3) for n, v in rate.items()},
            'share_of_copy_rate': {n: round(v / COPY_TBS, 3) for n, v in rate.items()},
            'torch_over_slate': round(med['torch'] / med['slate'], 2),
            'scan_over_slate': round(med['scan'] / med['slate'], 2),
            'max_abs_diff_to_torch': err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=4096)
    ap.add_argument('--V', type=int, default=1000000)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--C', default='100,1000')
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slate_bench: needs the GPU (no CPU path, nothing to time without it)")
    from arx import ops
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    B, V, d = args.B, args.V, args.d
    tensors = (torch.randn(B, d, device=dev, generator=g) * 0.3, torch.randn(V, d, device=dev, generator=g) * 0.3,
               torch.randn(V, device=dev, generator=g) * 0.1, ops.Workspace(dev))
    res = []
    for C in (int(c) for c in args.C.split(',')):
        for law in ('uniform', 'shared'):
            r = bench(dev, B, V, d, C, args.k, law, tensors, args)
            print(json.dumps(r), flush=True)
            res.append(r)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
