"""score_items(sample_temperature=): the sampled-slate kernel next to the plain order of the same slate and next to the
torch composition a user had without it, at the same shape: B rows, each with its own scored slate of C candidates out
of a V x d item pool, k draws, on plain tensors.  Run by hand on the MI355X; not part of bench.py.

  sample  : ops.slate_sample(cand, scores, (tau, B, seed), k, ids, values, pos, logp)  -- arx_slate_sample, one launch
  nologp  : the same with logp = None (the draw alone)
  order   : arx.slate.slate_order(scores, cand, k, ...)       -- plain score_items(k): top-k, take, mark
  torch   : g = -log(-log(rand)); sort(scores + tau g, descending) over the whole slate; a = scores / tau in that order;
            logp = a - flip(logcumsumexp(flip(a))); the first k of ids, scores, pos, logp -- the torch composition on
            the device.  It does not merge repeated ids, and its noise is a fresh torch.rand (not a function of the
            item: no replay from a seed)
  scores  : ops.slate_scores(U, P, b, cand, scores)           -- the scoring launch in front of all of them
  call    : scores + sample, the two launches of the whole sampled call; call_order: scores + order

HIP events around --calls calls, a warm-up of each first; inside each of the --rounds rounds the forms alternate; the
median over the rounds is reported per call.

usage: python tools/slate_sample_bench.py [--B 4096] [--V 1000000] [--d 128] [--C 256 1000] [--k 100] [--tau 0.5]
                                          [--rounds 5] [--calls 50] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'a-recsys_amd'), ROOT]

import torch  # noqa: E402


def region_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def torch_sample(cl, sc, tau, k):
    """The torch composition: (ids, values, pos, logp) [B, k].  cl int64 [B, C] (every slot live), sc [B, C],
    tau [B]."""
    t = tau[:, None]
    g = -torch.log(-torch.log(torch.rand_like(sc)))
    order = torch.sort(sc + t * g, dim=1, descending=True).indices
    s = torch.gather(sc, 1, order)
    a = s / t
    lp = a - torch.flip(torch.logcumsumexp(torch.flip(a, [1]), 1), [1])
    return torch.gather(cl, 1, order[:, :k]), s[:, :k].contiguous(), order[:, :k], lp[:, :k].contiguous()


def bench(args, C, dev):
    from arx import ops
    from arx.slate import slate_order
    B, V, d, k = args.B, args.V, args.d, args.k
    if not ops.slate_sample_supported(C):
        raise SystemExit("slate_sample_bench: arx_slate_sample_supported refuses C=%d" % C)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    U = torch.randn(B, d, device=dev, generator=g) * 0.3
    P = torch.randn(V, d, device=dev, generator=g) * 0.3
    b = torch.randn(V, device=dev, generator=g) * 0.1
    cand = torch.randint(0, V, (B, C), device=dev, generator=g, dtype=torch.int32)
    tau = torch.full((B,), args.tau, device=dev)
    seed = torch.tensor([12345, 0], dtype=torch.int32, device=dev)
    cl = cand.long()
    sc = torch.empty((B, C), device=dev)
    ops.slate_scores(U, P, b, cand, sc)
    ids, pos = (torch.empty((B, k), dtype=torch.int32, device=dev) for _ in range(2))
    vals, lp = (torch.empty((B, k), device=dev) for _ in range(2))
    sample = (tau, B, seed)
    keep = {}

    def f_torch():
        keep['torch'] = torch_sample(cl, sc, tau, k)

    def f_call():
        ops.slate_scores(U, P, b, cand, sc)
        ops.slate_sample(cand, sc, sample, k, ids, vals, pos, lp)

    def f_call_order():
        ops.slate_scores(U, P, b, cand, sc)
        slate_order(sc, cand, k, vals, pos, ids)
    fns = {'sample': lambda: ops.slate_sample(cand, sc, sample, k, ids, vals, pos, lp),
           'nologp': lambda: ops.slate_sample(cand, sc, sample, k, ids, vals, pos, None),
           'order': lambda: slate_order(sc, cand, k, vals, pos, ids),
           'torch': f_torch,
           'scores': lambda: ops.slate_scores(U, P, b, cand, sc),
           'call': f_call, 'call_order': f_call_order}
    for n, fn in fns.items():
        fn()
        torch.cuda.synchronize()
    fns['sample']()
    torch.cuda.synchronize()
    # a sanity figure, not a test: the mean log-propensity of a k-list under both (the same law, other noise)
    mean_lp = {'sample': round(float(lp.sum(1).mean().item()), 3),
               'torch': round(float(keep['torch'][3].sum(1).mean().item()), 3)}
    keep.clear()
    torch.cuda.empty_cache()
    times = {n: [] for n in fns}
    for _ in range(args.rounds):
        for n, fn in fns.items():
            times[n].append(region_ms(fn, args.calls))
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    return {'B': B, 'V': V, 'd': d, 'C': C, 'k': k, 'tau': args.tau,
            'ms': {n: round(v, 4) for n, v in med.items()},
            'ms_min_max': {n: [round(min(t), 4), round(max(t), 4)] for n, t in times.items()},
            'torch_over_sample': round(med['torch'] / med['sample'], 2),
            'sample_over_order': round(med['sample'] / med['order'], 2),
            'sample_over_nologp': round(med['sample'] / med['nologp'], 2),
            'call_over_call_order': round(med['call'] / med['call_order'], 2),
            'us_per_row': round(med['sample'] * 1e3 / B, 5),
            'mean_list_logp': mean_lp}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=4096)
    ap.add_argument('--V', type=int, default=1000000)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--C', type=int, nargs='+', default=[256, 1000])
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--tau', type=float, default=0.5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slate_sample_bench: needs the GPU (no CPU path, nothing to time without it)")
    dev = torch.device('cuda:0')
    res = []
    for C in args.C:
        res.append(bench(args, C, dev))
        print(json.dumps(res[-1]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
