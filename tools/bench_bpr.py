"""The 'bpr' train step at the C2 / C3 shapes (bench.py's workloads: 1 M users, 1 M items, B = 16384, d = 128):
negatives fed from a device-resident ring and negatives drawn inside the step, beside the 'mw' step of the same build.
HIP-event time of regions of --steps steps, the median of --repeats regions.  Not part of bench.py.

usage: python tools/bench_bpr.py [--workloads c2,c3] [--steps 100] [--warmup 20] [--out FILE.json]
       python tools/bench_bpr.py --kernel-only        # the pair kernel alone (a run for rocprofv3 --kernel-trace --stats)
       python tools/bench_bpr.py --sharded            # the world-1 ShardedHMF 'bpr' step at the C2 shape, fed and drawn
       python tools/bench_bpr.py --weighted [--sharded]   # also: the drawn step with the popularity^0.75 draw, and the
                                                          # two draw kernels alone on the workload's lists
       python tools/bench_bpr.py --workloads c2 --hard 4,16,64    # also: the drawn 'bpr' step training against the
                                                          # hardest of C candidates (arx_neg_draw_hardest) beside the plain
                                                          # drawn step of the same run, and that kernel alone
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

HBM_PEAK_GBS = 8000.0        # bench.py's
WORKLOADS = {'c2': dict(), 'c3': dict(item_mulhot=True)}


def region_ms(fn, steps, warmup, repeats):
    for k in range(warmup):
        fn(k)
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(warmup, warmup + steps):
            fn(k)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return sorted(out)[len(out) // 2]


def region_spread_ms(fn, steps, warmup, repeats):
    """{median, min, max} of `repeats` regions (region_ms keeps the median only)."""
    for k in range(warmup):
        fn(k)
    out = sorted(region_ms(fn, steps, 0, 1) for _ in range(repeats))
    return {'median': out[len(out) // 2], 'min': out[0], 'max': out[-1]}


def pair_kernel_us(B, d, dev, iters=200):
    """arx_pair_loss_fwdbwd alone on random operands; the algorithmic bytes are B (6 d + 7) 4."""
    from arx import ops
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    U, P, N = (torch.randn(B, d, device=dev, generator=g) * 0.1 for _ in range(3))
    pb, nb = torch.randn(B, device=dev, generator=g), torch.randn(B, device=dev, generator=g)
    ps, ns, bl, dpb, dnb = (torch.empty(B, device=dev) for _ in range(5))
    dU, dP, dN = (torch.empty(B, d, device=dev) for _ in range(3))
    fn = lambda k: ops.pair_loss(U, P, pb, N, nb, 'bpr', 1.0 / B, ps, ns, bl, dU=dU, dP=dP, dpbias=dpb, dN=dN,
                                 dnbias=dnb)
    ms = region_ms(fn, iters, 10, 3)
    nbytes = B * (6 * d + 7) * 4
    return {'us': ms * 1e3, 'algorithmic_bytes': nbytes, 'gbs': nbytes / ms / 1e6,
            'frac_of_hbm_peak': nbytes / ms / 1e6 / HBM_PEAK_GBS,
            'note': 'operands are cache-resident at this size: descriptive, not an HBM rate'}


def draw_kernels_us(users, ptr, cols, ex_cum, cum, V, col2item, dev, iters=200):
    """arx_neg_draw_uniform and arx_neg_draw_weighted alone: one batch of users on the model's own lists and tables,
    a new counter per launch.  Latency-bound chains of dependent loads: microseconds, no rate."""
    from arx import ops
    B = int(users.shape[0])
    out, look = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    uni = lambda k: ops.neg_draw_uniform(users, ptr, cols, V, col2item, 1, None, k, out, lookup_items=look)
    wtd = lambda k: ops.neg_draw_weighted(users, ptr, cols, ex_cum, cum, V, col2item, 1, None, k, out,
                                          lookup_items=look)
    res = {}
    for _ in range(2):                                   # alternating: uniform, weighted, uniform, weighted
        for name, fn in (('uniform_us', uni), ('weighted_us', wtd)):
            res.setdefault(name, []).append(region_ms(fn, iters, 10, 3) * 1e3)
    return {k: min(v) for k, v in res.items()}


def hard_kernel_us(users, ptr, cols, V, col2item, hard, Cs, dev, iters=200, repeats=5):
    """arx_neg_draw_hardest alone: one batch of users on the model's own lists and tables (the uniform rule), a new
    counter per launch.  The effective rate counts the gathered candidate rows and biases only, B C (d + 1) 4 bytes."""
    from arx import ops
    _, U, umap, P, pbias, col2row = hard()
    B, d = int(users.shape[0]), int(U.shape[1])
    out, look = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    res = {}
    for C in Cs:
        fn = lambda k: ops.neg_draw_hard(users, ptr, cols, None, None, V, col2item, 1, None, k * C, C, U, umap, P,
                                         pbias, col2row, out, lookup_items=look)
        ms = region_spread_ms(fn, iters, 10, repeats)
        nbytes = B * C * (d + 1) * 4
        res[str(C)] = {'us': ms['median'] * 1e3, 'us_min': ms['min'] * 1e3, 'us_max': ms['max'] * 1e3,
                       'gathered_bytes': nbytes, 'effective_gbs': nbytes / ms['median'] / 1e6}
    return res


def run_workload(name, args, dev):
    from arx.hmf.hmf_model import LatentProductModel
    from arx.utils.prepare_train import DeviceSampler
    from arx.utils.synthetic import SyntheticHMF
    B, d, S = args.batch, args.dim, args.n_sampled
    syn = SyntheticHMF(n_users=args.n_users, n_items=args.n_items, permute_logits=False, seed=0,
                       zipf_items=args.zipf_items, **WORKLOADS[name])
    rng = np.random.default_rng(1)
    nb = 64
    batches = []
    for _ in range(nb):
        u, i = syn.sample_batch(B, rng)
        n = rng.integers(0, args.n_items, size=B).astype(np.int32)
        batches.append(tuple(torch.from_numpy(a).to(dev) for a in (u, i, n)))
    res = {}

    def build(loss):
        m = LatentProductModel(args.n_users, args.n_items, d, 1, B, 0.1, 1.0, syn.u_attr, syn.i_attr,
                               syn.item2logit[:args.n_items], syn.logit_ind2item_ind, loss_function=loss,
                               n_sampled=S if loss == 'mw' else None)
        return m

    want = args.losses.split(',')
    if 'mw' in want:
        # for context: bench.py's step without the pool redraws
        model = build('mw')
        model.prepare_warp(syn.positives_csr(), syn.positives_csr())
        pool = DeviceSampler(syn.item_population, syn.p_sample, device=dev, seed=1).sample(S)

        def mw_step(k):
            u, i, _ = batches[k % nb]
            model.step_async(None, u, i, None, pool if k == 0 else None, None, loss='mw')
        res['mw_ms'] = region_ms(mw_step, args.steps, args.warmup, args.repeats)
        del model
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()

    for loss in ('bpr', 'bpr-hinge'):
        if loss not in want:
            continue
        model = build(loss)

        def fed(k):
            u, i, n = batches[k % nb]
            model.step_async(None, u, i, n)
        res[loss + '_fed_ms'] = region_ms(fed, args.steps, args.warmup, args.repeats)
        res[loss + '_fed_loss'] = float(model.loss.read().item())
        if loss == 'bpr' and 'bpr-drawn' in want:
            model.prepare_pair_negatives(syn.positives_csr(), seed=1)

            def drawn(k):
                u, i, _ = batches[k % nb]
                model.step_async(None, u, i, None)
            res['bpr_drawn_ms'] = region_ms(drawn, args.steps, args.warmup, args.repeats)
            res['bpr_drawn_loss'] = float(model.loss.read().item())
            res['auc_last_step'] = float(model.auc.read().item())
            if args.weighted:
                model.prepare_pair_negatives(syn.positives_csr(), seed=1, power=0.75)
                res['bpr_drawn_weighted_ms'] = region_ms(drawn, args.steps, args.warmup, args.repeats)
                res['bpr_drawn_weighted_loss'] = float(model.loss.read().item())
                res['auc_last_step_weighted'] = float(model.auc.read().item())
                m = model.att_emb
                ptr, cols, c2i, ex_cum, cum = m._pair_lists
                res['draw_kernels'] = draw_kernels_us(batches[0][0], ptr, cols, ex_cum, cum, m.logit_size, c2i, dev)
                model.prepare_pair_negatives(syn.positives_csr(), seed=1)        # the uniform step once more: spread
                res['bpr_drawn_again_ms'] = region_ms(drawn, args.steps, args.warmup, args.repeats)
            if args.hard and name != 'c2':
                res['hard'] = 'skipped: hardest_of needs one-hot items (the c2 shape)'
            elif args.hard:
                # plain, hardest of C for every C, plain again: one run, one model, one set of lists
                hard = {'plain_ms': region_spread_ms(drawn, args.steps, args.warmup, args.repeats)}
                for C in args.hard:
                    model.prepare_pair_negatives(syn.positives_csr(), seed=1, hardest_of=C)
                    hard['hardest_of_%d_ms' % C] = region_spread_ms(drawn, args.steps, args.warmup, args.repeats)
                    hard['hardest_of_%d_loss' % C] = float(model.loss.read().item())
                    hard['hardest_of_%d_auc_last_step' % C] = float(model.auc.read().item())
                m = model.att_emb
                ptr, cols, c2i = m._pair_lists[:3]
                hard['kernel'] = hard_kernel_us(batches[0][0], ptr, cols, m.logit_size, c2i, m.neg_draw.hard,
                                                args.hard, dev)
                model.prepare_pair_negatives(syn.positives_csr(), seed=1)
                hard['plain_again_ms'] = region_spread_ms(drawn, args.steps, args.warmup, args.repeats)
                res['hard'] = hard
        del model
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    return res


def run_sharded(args, dev):
    """The pair step of the row-sharded model on ONE rank (1-rank RCCL group: the exchanges are local copies) at the
    C2 shape: negatives fed through routes prepared ahead (prepare_route is the loader side, off the step path) and
    negatives drawn (the draw sits in prepare_route: route + step are timed together, and the route alone)."""
    import time
    import torch.distributed as dist
    from arx.dist import ShardedHMF
    from arx.utils.synthetic import SyntheticHMF
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29761")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    B, d = args.batch, args.dim
    syn = SyntheticHMF(n_users=args.n_users, n_items=args.n_items, permute_logits=False, seed=0,
                       zipf_items=args.zipf_items)
    rng = np.random.default_rng(1)
    nb = 64
    batches = []
    for _ in range(nb):
        u, i = syn.sample_batch(B, rng)
        batches.append((u, i, rng.integers(0, args.n_items, size=B).astype(np.int32)))
    res = {}
    try:
        for loss in [x for x in ('bpr', 'bpr-hinge') if x in args.losses.split(',')]:
            model = ShardedHMF(args.n_users, args.n_items, d, B, 0, 0.1, 0, 1, dev, loss=loss, seed=1)
            routes = [model.prepare_route(u, i, n) for u, i, n in batches]
            with torch.cuda.stream(model.stream):                 # (saves the two stream joins per step)
                res[loss + '_fed_ms'] = region_ms(lambda k: model.step(routes[k % nb]), args.steps, args.warmup,
                                                  args.repeats)
            res[loss + '_fed_loss'] = float(model.read_loss().item())
            res[loss + '_n_captures'], res[loss + '_n_replays'] = model.n_captures, model.n_replays
            if loss == 'bpr' and 'bpr-drawn' in args.losses.split(','):
                ptr = np.concatenate([syn.pos_ptr[:args.n_users + 1], [syn.pos_ptr[args.n_users]]]).astype(np.int32)
                model.set_positives(ptr, syn.pos_items)
                model.prepare_pair_negatives()

                def drawn(k):
                    u, i, _ = batches[k % nb]
                    model.step(model.prepare_route(u, i))
                with torch.cuda.stream(model.stream):
                    res['bpr_drawn_route_and_step_ms'] = region_ms(drawn, args.steps, args.warmup, args.repeats)
                res['bpr_drawn_loss'] = float(model.read_loss().item())
                res['auc_last_step'] = model.read_auc()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(args.steps):
                    model.prepare_route(*batches[k % nb][:2])
                torch.cuda.synchronize()
                res['bpr_drawn_route_ms'] = (time.perf_counter() - t0) / args.steps * 1e3
                t0 = time.perf_counter()
                for k in range(args.steps):
                    model.prepare_route(*batches[k % nb])
                torch.cuda.synchronize()
                res['bpr_fed_route_ms'] = (time.perf_counter() - t0) / args.steps * 1e3
                if args.weighted:
                    model.prepare_pair_negatives(power=0.75)
                    with torch.cuda.stream(model.stream):
                        res['bpr_drawn_weighted_route_and_step_ms'] = region_ms(drawn, args.steps, args.warmup,
                                                                                 args.repeats)
                    res['bpr_drawn_weighted_loss'] = float(model.read_loss().item())
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for k in range(args.steps):
                        model.prepare_route(*batches[k % nb][:2])
                    torch.cuda.synchronize()
                    res['bpr_drawn_weighted_route_ms'] = (time.perf_counter() - t0) / args.steps * 1e3
                    users = torch.from_numpy(batches[0][0]).to(dev)              # (world 1: user id = local row)
                    res['draw_kernels'] = draw_kernels_us(users, model._neg_csr[0], model._neg_csr[1],
                                                          model._neg_tables[0], model._neg_tables[1], args.n_items,
                                                          None, dev)
                    model.prepare_pair_negatives()                               # the uniform route once more: spread
                    with torch.cuda.stream(model.stream):
                        res['bpr_drawn_again_route_and_step_ms'] = region_ms(drawn, args.steps, args.warmup,
                                                                              args.repeats)
            del model, routes
            gc.collect()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    finally:
        dist.destroy_process_group()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='c2,c3')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batch', type=int, default=16384)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--n-items', type=int, default=1000000)
    ap.add_argument('--n-users', type=int, default=1000000)
    ap.add_argument('--n-sampled', type=int, default=1024)
    ap.add_argument('--zipf-items', type=float, default=1.05)
    ap.add_argument('--losses', default='mw,bpr,bpr-drawn,bpr-hinge',
                    help="which steps to time ('bpr-drawn' needs 'bpr'); one loss alone gives a clean kernel trace")
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--sharded', action='store_true',
                    help="the world-1 ShardedHMF pair step (C2 shape) instead of the single-GPU workloads")
    ap.add_argument('--weighted', action='store_true',
                    help="with 'bpr-drawn': also the step drawing by popularity^0.75 (arx_neg_draw_weighted), and the "
                         "uniform and the weighted draw kernel alone")
    ap.add_argument('--hard', default=None, type=lambda v: [int(c) for c in v.split(',') if c],
                    help="with 'bpr-drawn' on c2: C[,C...] -- also the drawn step with hardest_of=C (arx_neg_draw_hardest) "
                         "beside the plain drawn step of the same run, {median, min, max} of the repeats, and the kernel "
                         "alone (us, effective GB/s over B C (d + 1) 4 gathered bytes)")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'batch': args.batch, 'dim': args.dim, 'n_items': args.n_items, 'n_users': args.n_users,
           'steps': args.steps, 'repeats': args.repeats,
           'pair_kernel': pair_kernel_us(args.batch, args.dim, dev)}
    if args.sharded:
        out['sharded_c2'] = run_sharded(args, dev)
        print('sharded_c2', json.dumps(out['sharded_c2']), flush=True)
    elif not args.kernel_only:
        for name in [w for w in args.workloads.split(',') if w]:
            out[name] = run_workload(name, args, dev)
            print(name, json.dumps(out[name]), flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
