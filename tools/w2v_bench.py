"""The input stage of the skip-gram / CBOW recommenders (arx.word2vec.LinearSeq) at the headline shape -- mb = 16384,
n = 5 context items, d = 128, a 1 M-row item table, Zipf ids (SyntheticHMF, the C2 generator) -- and the whole CBOW
'mw' step with and without the fused window.  Run by hand on the MI355X; not part of bench.py.

(a) input stage, forward + backward-side launches, as captured graph replays (HIP events, median of --repeats
    regions of --steps replays, the two paths alternating):
      parent: gather_onehot over n * mb rows, col_sum, add_rows_bcast (user half), the two add_rows_bcast of the
              backward, sparse_site_onehot + sparse_adagrad over n * mb gradient rows
      fused : gather_window, one add_rows_bcast (user gradient), sparse_site_window + sparse_adagrad over mb rows
    GB/s = algorithmic bytes (from the shapes, stage_bytes()) / median time.
(b) whole step: CBOW 'mw', S = 1024, interactions/s = mb / step time, fuse_window True and False.
(c) --sharded: the world-1 step of the row-sharded model (arx.dist.ShardedW2V, routes prepared ahead, one captured
    graph) next to the single-process LinearSeq step (fused window) of the same shape and --loss; replaces (a), (b).

usage: python tools/w2v_bench.py [--steps 50] [--warmup 10] [--repeats 21] [--skip-step] [--out FILE.json]
       python tools/w2v_bench.py --sharded [--loss mw|mce] [--out FILE.json]
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


def stage_bytes(mb, n, d, uniq):
    """Bytes each path has to move, from the shapes (fp32 rows of d; ids and keys as int32; `uniq` distinct table
    rows in the batch, each read and written once in E and in the Adagrad slot)."""
    row = 4 * d
    table = 4 * uniq * row                                  # E and acc, read + write
    keys = 4 * n * mb * 4                                   # ids in, (key, src, coef) out
    parent = (2 * n * mb * row                              # gather: rows in, [n*mb, d] out
              + n * mb * row + mb * row                     # col_sum
              + 3 * mb * row                                # + 0.5 * user (x read, user read, x write)
              + mb * row + n * mb * row                     # backward: g in, [n*mb, d] gradient rows out
              + 2 * mb * row                                # user gradient
              + n * mb * row + table + keys)                # Adagrad: the gradient rows back in
    fused = (n * mb * row + 2 * mb * row                    # gather_window: rows + user in, x out
             + 2 * mb * row                                 # user gradient
             + mb * row + table + keys)                     # Adagrad: mb gradient rows (each read n times, from cache)
    return parent, fused


def median_ms(graphs, steps, warmup, repeats):
    """Median region time per replay for each captured graph; the graphs alternate region by region."""
    out = [[] for _ in graphs]
    for g in graphs:
        for _ in range(warmup):
            g.launch()
    for _ in range(repeats):
        for k, g in enumerate(graphs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                g.launch()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / steps)
    return [sorted(x)[len(x) // 2] for x in out], [(min(x), max(x)) for x in out]


def input_stage(args, syn, dev):
    from arx import ops
    mb, n, d, V = args.batch, args.n_input, args.dim, args.n_items
    rng = np.random.default_rng(1)
    ids_np = np.stack([syn.sample_batch(mb, rng)[1] for _ in range(n)], 0).reshape(-1).astype(np.int32)
    ids = torch.from_numpy(ids_np).to(dev)
    uniq = int(len(np.unique(ids_np)))
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    E = torch.randn(V, d, device=dev, generator=g) * 0.1
    acc = torch.full_like(E, 0.1)
    user = torch.randn(mb, d, device=dev, generator=g) * 0.1
    grad = torch.randn(mb, d, device=dev, generator=g) * 1e-3       # d loss / d x
    lr = torch.full((1,), 0.1, device=dev)
    aux = torch.zeros(V, dtype=torch.int32, device=dev)
    ws_a, ws_b = ops.Workspace(dev), ops.Workspace(dev)
    # parent
    rows = torch.empty(n * mb, d, device=dev)
    x_a = torch.empty(mb, d, device=dev)
    g_rows = torch.empty(n * mb, d, device=dev)
    g_user_a = torch.empty(mb, d, device=dev)
    k_a, s_a = (torch.empty(n * mb, dtype=torch.int32, device=dev) for _ in range(2))
    c_a = torch.empty(n * mb, device=dev)

    def parent():
        ops.gather_onehot(E, None, None, ids, rows, scale=0.5 / n)
        ops.col_sum(rows.view(n, mb * d), x_a.view(-1), ws_a)
        ops.add_rows_bcast(0.5, user, 1.0, x_a)
        ops.add_rows_bcast(1.0, grad, 0.0, g_rows)
        ops.add_rows_bcast(0.5, grad, 0.0, g_user_a)
        ops.sparse_site_onehot(None, ids, 0, 0.5 / n, k_a, s_a, c_a)
        ops.sparse_adagrad(E, acc, None, None, k_a, s_a, c_a, g_rows, None, lr, ws_a, n=n * mb, aux_cnt=aux)
    # fused
    x_b = torch.empty(mb, d, device=dev)
    g_user_b = torch.empty(mb, d, device=dev)
    k_b, s_b = (torch.empty(n * mb, dtype=torch.int32, device=dev) for _ in range(2))
    c_b = torch.empty(n * mb, device=dev)

    def fused():
        ops.gather_window(E, None, ids, n, x_b, scale=0.5 / n, base=user, base_scale=0.5)
        ops.add_rows_bcast(0.5, grad, 0.0, g_user_b)
        ops.sparse_site_window(None, ids, n, 0, 0.5 / n, k_b, s_b, c_b)
        ops.sparse_adagrad(E, acc, None, None, k_b, s_b, c_b, grad, None, lr, ws_b, n=n * mb, aux_cnt=aux)
    # same numbers first (fresh tables for each), then the timing
    E0 = E.clone()
    parent()
    xa, Ea = x_a.clone(), E.clone()
    E.copy_(E0)
    acc.fill_(0.1)
    fused()
    torch.cuda.synchronize()
    err_x = float((xa - x_b).abs().max())
    err_E = float((Ea - E).abs().max())
    graphs = [ops.CapturedGraph.record(parent, fork=True), ops.CapturedGraph.record(fused, fork=True)]
    (t_par, t_fus), spread = median_ms(graphs, args.steps, args.warmup, args.repeats)
    b_par, b_fus = stage_bytes(mb, n, d, uniq)
    return {'mb': mb, 'n': n, 'd': d, 'rows': V, 'distinct_rows': uniq,
            'max_abs_diff_x': err_x, 'max_abs_diff_E_after_update': err_E,
            'parent_us': t_par * 1e3, 'fused_us': t_fus * 1e3,
            'parent_us_min_max': [v * 1e3 for v in spread[0]], 'fused_us_min_max': [v * 1e3 for v in spread[1]],
            'parent_bytes': b_par, 'fused_bytes': b_fus,
            'parent_gbs': b_par / t_par / 1e6, 'fused_gbs': b_fus / t_fus / 1e6,
            'parent_frac_of_hbm_peak': b_par / t_par / 1e6 / HBM_PEAK_GBS,
            'fused_frac_of_hbm_peak': b_fus / t_fus / 1e6 / HBM_PEAK_GBS}


def _median_step_ms(step, args):
    """Median over regions of --steps calls of step(k), after --warmup calls."""
    for k in range(args.warmup):
        step(k)
    times = []
    for _ in range(max(3, args.repeats // 4)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(args.warmup, args.warmup + args.steps):
            last = step(k)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / args.steps)
    return sorted(times)[len(times) // 2], last


def sharded_step(args, syn, dev):
    """(c): CBOW, --loss, the shape of (b).  Both models start from their own random tables (the timing does not
    depend on the values); the sharded one is timed twice -- reading the loss back every step, as LinearSeq.step
    does, and without."""
    import torch.distributed as dist
    from arx.dist import ShardedW2V
    from arx.utils.prepare_train import DeviceSampler
    mb, n, d, S = args.batch, args.n_input, args.dim, args.n_sampled
    res = whole_step(args, syn, dev, variants=(('fused', True),), loss=args.loss)
    res = {'linear_seq': res['fused']}
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29777")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    model = ShardedW2V(args.n_users, args.n_items, d, mb, S, n, 0.1, 0, 1, dev, cbow=True, loss=args.loss)
    model.set_positives(syn.pos_ptr, syn.pos_items)
    model.set_pool(DeviceSampler(syn.item_population, syn.p_sample, device=dev, seed=1).sample(S))
    rng = np.random.default_rng(2)
    routes = []
    for _ in range(16):
        u, t = syn.sample_batch(mb, rng)
        ctx = np.stack([syn.sample_batch(mb, rng)[1] for _ in range(n)], 0)
        routes.append(model.prepare_route(u, t, ctx))

    def step(k):
        model.step(routes[k % len(routes)])

    def step_read(k):
        model.step(routes[k % len(routes)])
        return float(model.read_loss().item())
    with torch.cuda.stream(model.stream):
        ms_read, loss = _median_step_ms(step_read, args)
        ms, _ = _median_step_ms(step, args)
    res['sharded_world1'] = {'ms_per_step': ms_read, 'interactions_per_s': mb / ms_read * 1e3,
                             'ms_per_step_no_readback': ms, 'interactions_per_s_no_readback': mb / ms * 1e3,
                             'last_loss': loss, 'n_captures': model.n_captures, 'n_replays': model.n_replays,
                             'fused_scorer': bool(model._fused_scorer())}
    dist.destroy_process_group()
    return res


def whole_step(args, syn, dev, variants=(('fused', True), ('unfused', False)), loss='mw'):
    from arx.utils.prepare_train import DeviceSampler
    from arx.word2vec import cbow_model
    mb, n, d, S = args.batch, args.n_input, args.dim, args.n_sampled
    rng = np.random.default_rng(2)
    nb = 16
    batches = []
    for _ in range(nb):
        u, t = syn.sample_batch(mb, rng)
        ctx = np.stack([syn.sample_batch(mb, rng)[1] for _ in range(n)], 0).reshape(-1)
        batches.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (u, ctx, t)))
    pool = DeviceSampler(syn.item_population, syn.p_sample, device=dev, seed=1).sample(S)
    res = {}
    for name, fuse in variants:
        model = cbow_model.Model(args.n_users, args.n_items, d, mb, 0.1, 1.0, syn.u_attr, syn.i_attr,
                                 syn.item2logit[:args.n_items], syn.logit_ind2item_ind, n_input_items=n,
                                 loss_function=loss, use_sep_item=True, n_sampled=S, fuse_window=fuse)
        model.prepare_warp(syn.positives_csr(), syn.positives_csr())
        assert model.fuse_window == fuse

        def step(k):
            u, ctx, t = batches[k % nb]
            return model.step(None, u, ctx, t, item_sampled=pool if k == 0 else None)
        ms, last = _median_step_ms(step, args)
        res[name] = {'ms_per_step': ms, 'interactions_per_s': mb / ms * 1e3, 'last_loss': float(last),
                     'note': 'step() reads the loss back every step (one device -> host sync per step)'}
        del model
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=21)
    ap.add_argument('--batch', type=int, default=16384)
    ap.add_argument('--n-input', type=int, default=5)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--n-items', type=int, default=1000000)
    ap.add_argument('--n-users', type=int, default=1000000)
    ap.add_argument('--n-sampled', type=int, default=1024)
    ap.add_argument('--skip-step', action='store_true', help="(a) only")
    ap.add_argument('--sharded', action='store_true', help="(c): world-1 ShardedW2V step next to LinearSeq's")
    ap.add_argument('--loss', default='mw', choices=['mw', 'mce'], help="the loss of (c)")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.repeats < 20:
        ap.error("--repeats: a median of at least 20 regions")
    if not torch.cuda.is_available():
        sys.exit("tools/w2v_bench.py measures on the GPU; none is available")
    from arx.utils.synthetic import SyntheticHMF
    dev = torch.device('cuda:0')
    syn = SyntheticHMF(n_users=args.n_users, n_items=args.n_items, permute_logits=False, seed=0)
    out = {}
    if args.sharded:
        out['sharded_step_' + args.loss] = sharded_step(args, syn, dev)
    else:
        out['input_stage'] = input_stage(args, syn, dev)
        print('input_stage', json.dumps(out['input_stage']), flush=True)
    if not args.skip_step and not args.sharded:
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        out['cbow_mw_step'] = whole_step(args, syn, dev)
        print('cbow_mw_step', json.dumps(out['cbow_mw_step']), flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
