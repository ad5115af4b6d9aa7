"""explain_items' kernel next to the only formulation a user had without it, at the same shape: B rows, each with its
own slate of C items of the C3 HET layout (an id row + one bag of tokens per item, bag lengths clip(Poisson(20), 1,
64)), the per-feature parts, the bias part and the `top` largest token contributions of every (row, item) pair, on plain
tensors.  Run by hand on the MI355X; not part of bench.py.

  explain : ops.explain_slate(U, cand, es, top, feat, bias, tok_val, tok_id, tok_feat)   -- arx_explain_slate, one launch
  torch   : the torch composition: the bags padded to the longest one, E_tok[pad[cand]] gathered to [rows, C, len, d],
            a bmm against the row's latent, the masked topk per bag, the masked sum per bag, and the id row's dot.  It
            runs over --chunk rows at a time, because the gathered rows of all B would not fit comfortably (4096 x 100
            x 44 x 128 floats is 9.2 GB); the chunks are part of its time.
  slate   : ops.slate_scores over the pooled latents of the same items -- the yardstick beside it: what the SCORE alone
            costs, one pool row per slot instead of 1 + len table rows

HIP events around --calls calls, a warm-up of each first; inside each of the --rounds rounds the forms alternate; the
median over the rounds is reported per call with min .. max, and the kernel's EFFECTIVE rate over its gathered bytes
B * C * (F_cat + sum len) * (d + 1) * 4 (every table row and its bias, once per slot that names it).

usage: python tools/explain_bench.py [--B 4096] [--V 1000000] [--tokens 100000] [--d 128] [--C 100] [--top 3]
                                     [--rounds 5] [--calls 5] [--chunk 256] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'a-recsys_amd'), ROOT]

import numpy as np  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=4096)
    ap.add_argument('--V', type=int, default=1000000)
    ap.add_argument('--tokens', type=int, default=100000)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--C', type=int, default=100)
    ap.add_argument('--top', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--chunk', type=int, default=256)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("explain_bench: needs the GPU (no CPU path, nothing to time without it)")
    from arx import ops
    dev = torch.device('cuda:0')
    B, V, d, C, T, n_tok = args.B, args.V, args.d, args.C, args.top, args.tokens
    rng = np.random.default_rng(0)
    lens_np = np.clip(rng.poisson(20, size=V), 1, 64).astype(np.int32)
    starts_np = np.concatenate([[0], np.cumsum(lens_np, dtype=np.int64)[:-1]]).astype(np.int32)
    vals_np = rng.integers(0, n_tok, size=int(lens_np.sum())).astype(np.int32)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    U = torch.randn(B, d, device=dev, generator=g) * 0.3
    E_id, b_id = torch.randn(V, d, device=dev, generator=g) * 0.3, torch.randn(V, device=dev, generator=g) * 0.1
    E_tok, b_tok = torch.randn(n_tok, d, device=dev, generator=g) * 0.3, torch.randn(n_tok, device=dev, generator=g) * 0.1
    vals, starts, lens = (torch.from_numpy(a).to(dev) for a in (vals_np, starts_np, lens_np))
    cand = torch.randint(0, V, (B, C), device=dev, generator=g, dtype=torch.int32)
    feats = [types.SimpleNamespace(kind='cat', table=types.SimpleNamespace(E=E_id, bias=b_id), maps=(None,)),
             types.SimpleNamespace(kind='mulhot', table=types.SimpleNamespace(E=E_tok, bias=b_tok),
                                   maps=(vals, starts, lens))]
    es = ops.ExplainSet(feats, V)
    F = 2
    feat = torch.empty((B, C, F), device=dev)
    bias = torch.empty((B, C), device=dev)
    tv = torch.empty((B, C, T), device=dev)
    ti = torch.empty((B, C, T), dtype=torch.int32, device=dev)
    tf = torch.empty((B, C, T), dtype=torch.int32, device=dev)

    # the pooled latents, for the yardstick
    P, pb = torch.empty((V, d), device=dev), torch.empty(V, device=dev)
    ids = torch.arange(V, dtype=torch.int32, device=dev)
    ops.gather_id_plus_bag(E_id, b_id, None, E_tok, b_tok, vals, starts, lens, ids, P, scale=0.5, bias_out=pb)
    sc = torch.empty((B, C), device=dev)

    # the torch composition's static side: the bags padded to the longest one
    Lm = int(lens_np.max())
    pad_np = np.zeros((V, Lm), dtype=np.int64)
    mask_np = np.arange(Lm)[None, :] < lens_np[:, None]
    pad_np[mask_np] = vals_np
    pad, mask, flen = torch.from_numpy(pad_np).to(dev), torch.from_numpy(mask_np).to(dev), lens.float()
    t_feat, t_bias = torch.empty((B, C, F), device=dev), torch.empty((B, C), device=dev)
    t_tv, t_ti = torch.empty((B, C, T), device=dev), torch.empty((B, C, T), dtype=torch.int64, device=dev)
    cl = cand.long()

    def f_torch():
        for r0 in range(0, B, args.chunk):
            c = cl[r0:r0 + args.chunk]
            u = U[r0:r0 + args.chunk]
            b = c.shape[0]
            tok, m = pad[c], mask[c]                                           # [b, C, Lm]
            coef = (1.0 / (F * flen[c])).unsqueeze(-1)
            x = torch.bmm(E_tok[tok].view(b, C * Lm, d), u.unsqueeze(-1)).view(b, C, Lm)
            bt = b_tok[tok]
            x = (x + bt) * coef
            t_feat[r0:r0 + b, :, 1] = (x * m).sum(-1)
            top = torch.topk(x.masked_fill(~m, float('-inf')), T, dim=-1)
            t_tv[r0:r0 + b] = top.values
            t_ti[r0:r0 + b] = torch.gather(tok, 2, top.indices).masked_fill(top.values == float('-inf'), -1)
            bi = b_id[c]
            t_feat[r0:r0 + b, :, 0] = ((E_id[c] * u[:, None, :]).sum(-1) + bi) / F
            t_bias[r0:r0 + b] = bi / F + (bt * m * coef).sum(-1)

    fns = {'explain': lambda: ops.explain_slate(U, cand, es, T, feat, bias, tv, ti, tf),
           'torch': f_torch,
           'slate': lambda: ops.slate_scores(U, P, pb, cand, sc)}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    err = {'feature': float((feat - t_feat).abs().max().item()), 'bias': float((bias - t_bias).abs().max().item()),
           'token_value': float((tv - t_tv).nan_to_num(nan=0.0).abs().max().item()),     # (-inf - -inf: a short bag)
           'token_id_mismatches': int((ti.long() != t_ti).sum().item()),
           'score_minus_feature_sum': float((sc - feat.sum(-1)).abs().max().item())}
    times = {n: [] for n in fns}
    for _ in range(args.rounds):
        for n, fn in fns.items():
            times[n].append(region_ms(fn, args.calls))
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    rows = int((1 + lens[cl].long()).sum().item())                             # table rows gathered by the kernel
    nbytes = rows * (d + 1) * 4
    res = {'B': B, 'V': V, 'tokens': n_tok, 'd': d, 'C': C, 'top': T, 'longest_bag': Lm,
           'mean_bag': round(float(lens_np.mean()), 2), 'gathered_bytes': nbytes,
           'ms': {n: round(v, 4) for n, v in med.items()},
           'ms_min_max': {n: [round(min(t), 4), round(max(t), 4)] for n, t in times.items()},
           'explain_effective_tbs': round(nbytes / med['explain'] / 1e9, 3),
           'slate_effective_tbs': round(B * C * (4 * d + 12) / med['slate'] / 1e9, 3),
           'torch_over_explain': round(med['torch'] / med['explain'], 2),
           'explain_over_slate': round(med['explain'] / med['slate'], 2),
           'max_abs_diff_to_torch': err}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
