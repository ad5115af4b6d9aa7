"""The GRU encoder (csrc/gru.hip) beside the LSTM of the same build.  Not part of bench.py.

  kernels   arx_gru_fwd / arx_gru_bwd alone against arx_lstm_fwd / arx_lstm_bwd at the same shapes:
            L = 50, din = h = 64 at B = 1024 and at B = 8192; L = 20, din = h = 128 at B = 4096
  torch     torch.nn.GRU forward and forward + backward at those shapes -- its arithmetic differs (the reset is applied
            after the product) but its cost is the same: the outside yardstick
  step      the whole C4-shaped training step (tools/lstm_bench.py's workload) with cell='gru' against cell='lstm'
HIP-event time of regions of --iters launches (--steps steps), {median, min, max} of --repeats regions, the two cells
alternating inside one process.

usage: python tools/gru_bench.py [--what kernels,torch,step] [--iters 50] [--repeats 5] [--out FILE.json]
"""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'a-recsys_amd'), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(50, 1024, 64), (50, 8192, 64), (20, 4096, 128)]       # (L, B, din = h)


def region_spread_us(fn, iters, warmup, repeats):
    """{median, min, max} in microseconds per call over `repeats` regions of `iters` calls."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters * 1e3)
    out.sort()
    return {'median': out[len(out) // 2], 'min': out[0], 'max': out[-1]}


def kernels(L, B, h, dev, args):
    from arx import ops
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rn = lambda *s, scale=1.0: torch.randn(*s, device=dev, generator=g) * scale
    n, din = L * B, h
    x, dhs = rn(n, din, scale=0.5), rn(n, h)
    em = lambda *s: torch.empty(*s, device=dev)
    # GRU
    Wg, bg, Wc, bc = rn(din + h, 2 * h, scale=0.2), rn(2 * h, scale=0.1), rn(din + h, h, scale=0.2), rn(h, scale=0.1)
    hs, gates, rh, dzg, dzc = em(n, h), em(n, 3 * h), em(n, h), em(n, 2 * h), em(n, h)
    gf = lambda: ops.gru_fwd(x, Wg, bg, Wc, bc, L, B, din, h, hs, gates, rh)
    gb = lambda: ops.gru_bwd(Wg, Wc, hs, gates, dhs, L, B, din, h, dzg, dzc)
    # LSTM
    W, b = rn(din + h, 4 * h, scale=0.2), rn(4 * h, scale=0.1)
    lhs, lcs, lg, dz = em(n, h), em(n, h), em(n, 4 * h), em(n, 4 * h)
    lf = lambda: ops.lstm_fwd(x, W, b, L, B, din, h, 1.0, lhs, lcs, lg)
    lb = lambda: ops.lstm_bwd(W, lhs, lcs, lg, dhs, L, B, din, h, dz)
    res = {}
    for rnd in range(2):                                  # alternating: the second round is the one reported
        for name, fn in (('gru_fwd_us', gf), ('lstm_fwd_us', lf), ('gru_bwd_us', gb), ('lstm_bwd_us', lb)):
            res[name] = region_spread_us(fn, args.iters, 5, args.repeats)
    res['fwd_gru_over_lstm'] = res['gru_fwd_us']['median'] / res['lstm_fwd_us']['median']
    res['bwd_gru_over_lstm'] = res['gru_bwd_us']['median'] / res['lstm_bwd_us']['median']
    # products of one pass, as flops: forward 2 L B (din + h) 3h; backward 2 L B h 3h (the two recurrent products)
    res['gru_fwd_tflops'] = 2.0 * n * (din + h) * 3 * h / res['gru_fwd_us']['median'] / 1e6
    res['gru_bwd_tflops'] = 2.0 * n * h * 3 * h / res['gru_bwd_us']['median'] / 1e6
    return res


def torch_gru(L, B, h, dev, args):
    net = torch.nn.GRU(h, h).to(dev)
    x = torch.randn(L, B, h, device=dev, requires_grad=True)
    dh = torch.randn(L, B, h, device=dev)

    def fwd():
        with torch.no_grad():
            net(x)

    def fwd_bwd():
        y, _ = net(x)
        y.backward(dh)
    it = max(5, args.iters // 5)
    return {'fwd_us': region_spread_us(fwd, it, 3, args.repeats),
            'fwd_bwd_us': region_spread_us(fwd_bwd, it, 3, args.repeats)}


def c4_step(args, dev):
    """tools/lstm_bench.py's workload, once per cell, regions alternating between the two models."""
    from arx.attributes.embed_attribute import EmbeddingAttribute
    from arx.lstm.seqModel import SeqModel
    from arx.utils.synthetic import SyntheticHMF
    B, L, S, size = args.batch, 50, 1024, 64
    syn = SyntheticHMF(n_users=args.n_users, n_items=args.n_items, permute_logits=False, seed=0)
    syn.u_attr.set_model_size(size)
    syn.i_attr.set_model_size(size)
    START = args.n_items
    rng = np.random.default_rng(1)
    batches = []
    for _ in range(8):
        users = rng.integers(0, args.n_users, size=B).astype(np.int32)
        tg = np.stack([syn.sample_batch(B, rng)[1] for _ in range(L)], 0).astype(np.int32)
        inp = np.concatenate([np.full((1, B), START, dtype=np.int32), tg[:-1]], 0)
        lens = rng.integers(10, L + 1, size=B)
        w = (np.arange(L)[:, None] < lens[None, :]).astype(np.float32)
        batches.append(tuple(torch.from_numpy(a).to(dev) for a in (users, inp, tg, w)))
    pool = torch.from_numpy(syn.sample_pool(S, rng)).to(dev)
    fns = {}
    for cell in ('lstm', 'gru'):
        emb = EmbeddingAttribute(syn.u_attr, syn.i_attr, B, S, L, False, None, syn.logit_ind2item_ind)
        model = SeqModel([L], size, 1, 5.0, B, 0.5, 0.99, emb, loss='mw', use_concat=False, START_ID=START, cell=cell)
        emb.prepare_warp(syn.positives_csr(), syn.positives_csr())
        k = [0]

        def step(model=model, k=k):
            u, i, t, w = batches[k[0] % 8]
            model.step_async(None, u, i, t, w, 0, pool if k[0] == 0 else None, None)
            k[0] += 1
        fns[cell] = step
    res = {}
    for rnd in range(2):
        for cell in ('lstm', 'gru'):
            res[cell + '_us'] = region_spread_us(fns[cell], args.steps, 5, args.repeats)
    res['gru_over_lstm'] = res['gru_us']['median'] / res['lstm_us']['median']
    res['workload'] = "C4: d = h = %d, L = %d, B = %d, %d items, S = %d 'mw', clip 5.0, Adagrad" % (
        size, L, B, args.n_items, S)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='kernels,torch,step')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--n-items', type=int, default=1000000)
    ap.add_argument('--n-users', type=int, default=1000000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    what = args.what.split(',')
    out = {'iters': args.iters, 'repeats': args.repeats}
    for L, B, h in SHAPES:
        key = 'L%d_B%d_h%d' % (L, B, h)
        out[key] = {}
        if 'kernels' in what:
            out[key].update(kernels(L, B, h, dev, args))
        if 'torch' in what:
            out[key]['torch_nn_GRU'] = torch_gru(L, B, h, dev, args)
        print(key, json.dumps(out[key]), flush=True)
        gc.collect()
        torch.cuda.empty_cache()
    if 'step' in what:
        out['c4_step'] = c4_step(args, dev)
        print('c4_step', json.dumps(out['c4_step']), flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
