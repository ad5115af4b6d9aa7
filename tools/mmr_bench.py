"""score_items(diversify=): the greedy MMR re-rank kernel next to the only formulation a user had without it, at the same
shape: B rows, each with its own scored slate of C candidates out of a V x d item pool, k picks, on plain tensors.  Run
by hand on the MI355X; not part of bench.py.

  mmr     : ops.slate_mmr(P, cand, scores, lam, ..., k, ids, values, pos)    -- arx_slate_mmr, one launch
  capped  : the same with groups [V] and max_per_group [B]
  torch   : X = P[cand]; X /= |X|; G = bmm(X, X^T); k steps of (objective, masked arg-max, scatter, row of G, maximum)
            on the device -- the torch composition, from the same scores; [B, C, d] and [B, C, C] are materialised
  torch_capped : the same with a [B, n_groups] count table (gather / scatter_add per step)
  order   : arx.slate.slate_order(scores, cand, k, ...)                      -- plain score_items(k), as a scale: what
            the k picks cost without diversity
  scores  : ops.slate_scores(U, P, b, cand, scores)                          -- the scoring launch in front of all of them

HIP events around --calls calls, a warm-up of each first; inside each of the --rounds rounds the forms alternate; the
median over the rounds is reported per call.  `agree` is the share of (row, step) picks on which the kernel and the
torch composition name the same slot (they break ties differently, and float32 sums in another order move a near-tie:
it is a sanity figure, the tests hold the kernel to the float64 oracle).

usage: python tools/mmr_bench.py [--B 4096] [--V 1000000] [--d 128] [--C 256] [--k 100] [--lam 0.7] [--groups 64]
                                 [--cap 5] [--rounds 3] [--calls 3] [--out FILE.json]
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


def torch_mmr(P, cl, sc, lam, k, grp=None, cap=None, n_groups=0):
    """The torch composition: (pos int64 [B, k]).  cl int64 [B, C] (every slot live), sc [B, C], lam [B]; grp int64
    [V] in [0, n_groups) and cap int64 [B], or None."""
    B, C = cl.shape
    X = P[cl]
    X = X * torch.rsqrt((X * X).sum(-1, keepdim=True))
    G = torch.bmm(X, X.transpose(1, 2))
    lo, hi = sc.min(1, keepdim=True).values, sc.max(1, keepdim=True).values
    rel = (sc - lo) / (hi - lo)
    la, om = lam[:, None], 1.0 - lam[:, None]
    pen = torch.zeros_like(sc)
    shut = torch.zeros((B, C), dtype=torch.bool, device=sc.device)       # taken, or its group is full
    taken = torch.zeros((B, C), dtype=torch.bool, device=sc.device)
    rows = torch.arange(B, device=sc.device)
    pos = torch.empty((B, k), dtype=torch.int64, device=sc.device)
    if grp is not None:
        g = grp[cl]
        count = torch.zeros((B, n_groups), dtype=torch.int64, device=sc.device)
        one = torch.ones((B, 1), dtype=torch.int64, device=sc.device)
    for t in range(k):
        obj = (la * rel - om * pen).masked_fill(shut, float('-inf'))
        j = obj.argmax(1)
        pos[:, t] = j
        taken[rows, j] = True
        pen = torch.maximum(pen, G[rows, j])
        if grp is not None:
            count.scatter_add_(1, g[rows, j][:, None], one)
            shut = taken | (count.gather(1, g) >= cap[:, None])
        else:
            shut = taken
    return pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=4096)
    ap.add_argument('--V', type=int, default=1000000)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--C', type=int, default=256)
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--lam', type=float, default=0.7)
    ap.add_argument('--groups', type=int, default=64)
    ap.add_argument('--cap', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mmr_bench: needs the GPU (no CPU path, nothing to time without it)")
    from arx import ops
    from arx.slate import slate_order
    dev = torch.device('cuda:0')
    B, V, d, C, k = args.B, args.V, args.d, args.C, args.k
    if not ops.slate_mmr_supported(C, d):
        raise SystemExit("mmr_bench: arx_slate_mmr_supported refuses C=%d d=%d" % (C, d))
    if args.groups * args.cap < k:
        raise SystemExit("mmr_bench: groups * cap < k -- every row would run out of eligible slots")
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    U = torch.randn(B, d, device=dev, generator=g) * 0.3
    P = torch.randn(V, d, device=dev, generator=g) * 0.3
    b = torch.randn(V, device=dev, generator=g) * 0.1
    cand = torch.randint(0, V, (B, C), device=dev, generator=g, dtype=torch.int32)
    groups = torch.randint(0, args.groups, (V,), device=dev, generator=g, dtype=torch.int32)
    lam = torch.full((B,), args.lam, device=dev)
    cap = torch.full((B,), args.cap, dtype=torch.int32, device=dev)
    cl, gl, capl = cand.long(), groups.long(), cap.long()
    sc = torch.empty((B, C), device=dev)
    ops.slate_scores(U, P, b, cand, sc)
    ids, pos = (torch.empty((B, k), dtype=torch.int32, device=dev) for _ in range(2))
    vals = torch.empty((B, k), device=dev)
    tpos = {}

    def f_torch():
        tpos['torch'] = torch_mmr(P, cl, sc, lam, k)

    def f_torch_capped():
        tpos['torch_capped'] = torch_mmr(P, cl, sc, lam, k, gl, capl, args.groups)
    fns = {'mmr': lambda: ops.slate_mmr(P, cand, sc, lam, None, None, k, ids, vals, pos),
           'capped': lambda: ops.slate_mmr(P, cand, sc, lam, groups, cap, k, ids, vals, pos),
           'torch': f_torch, 'torch_capped': f_torch_capped,
           'order': lambda: slate_order(sc, cand, k, vals, pos, ids),
           'scores': lambda: ops.slate_scores(U, P, b, cand, sc)}
    agree = {}
    for n, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        if n in ('mmr', 'capped'):
            agree[n] = pos.long().clone()
    for n, t in (('mmr', 'torch'), ('capped', 'torch_capped')):
        agree[n] = round(float((agree[n] == tpos[t]).float().mean().item()), 4)
    tpos.clear()
    torch.cuda.empty_cache()
    times = {n: [] for n in fns}
    for _ in range(args.rounds):
        for n, fn in fns.items():
            times[n].append(region_ms(fn, args.calls))
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    res = {'B': B, 'V': V, 'd': d, 'C': C, 'k': k, 'lam': args.lam, 'groups': args.groups, 'cap': args.cap,
           'ms': {n: round(v, 4) for n, v in med.items()},
           'ms_min_max': {n: [round(min(t), 4), round(max(t), 4)] for n, t in times.items()},
           'torch_over_mmr': round(med['torch'] / med['mmr'], 2),
           'torch_capped_over_capped': round(med['torch_capped'] / med['capped'], 2),
           'mmr_over_order': round(med['mmr'] / med['order'], 2),
           'us_per_row_round': round(med['mmr'] * 1e3 / (B * k), 5),
           'agree_with_torch': agree}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
