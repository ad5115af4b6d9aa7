"""Refresh and recommend of the serving view of the sharded HET models (arx.dist.ShardedHetView) at C3's shape, world 1:
1 M items, 100 k tokens, ~20 tokens per bag, d = 128 (ShardedHMFRepTokens, the class that trains C3).

usage: python tools/sharded_het_view_bench.py [--V 1000000] [--tokens 100000] [--bag 20] [--d 128] [--B 4096]
                                              [--k 100] [--rounds 7] [--calls 10] [--out FILE.json]
Three times, device events around `--calls` calls, `--rounds` rounds with the routes alternating inside a round
(median, min and max over the rounds):
  refresh_ms          view.refresh(): ONE arx_het_rows_range launch over the shard's columns, straight into the view
  parent_route_ms     what the code before the view had to do for the same latents: an arange-stride id vector
                      (c * W + rank), arx_gather_id_plus_bag through the id -> row map, the bias copy into place
  parent_gather_ms    ... its arx_gather_id_plus_bag launch alone (ids ready, bias written in place): kernel against
                      kernel, the comparison that is hardest on the new one
  recommend_ms        view.recommend for B users at k (latents fresh: no refresh inside)
and the achieved rate of the refresh over the bytes the rows need (token rows + id rows read, latents written).
The two routes' latents are compared bit for bit."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-recsys_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
from arx import ops  # noqa: E402
from arx.dist import ShardedHMFRepTokens  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--V", type=int, default=1000000)
ap.add_argument("--tokens", type=int, default=100000)
ap.add_argument("--bag", type=int, default=20)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()

os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29783")
torch.cuda.set_device(0)
dev = torch.device('cuda', 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


V, nt, d, B, k = args.V, args.tokens, args.d, args.B, args.k
rng = np.random.default_rng(1)
lens = rng.integers(args.bag // 2, args.bag + args.bag // 2 + 1, size=V).astype(np.int32)       # mean: --bag
starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
vals = rng.integers(0, nt, size=int(lens.sum())).astype(np.int32)
model = ShardedHMFRepTokens(max(B, 1024), V, d, B, 1024, 0.1, 0, 1, dev, (vals, starts, lens), nt, seed=1, graphs=False)
view = model.item_view()
W, r, ni = model.world, model.rank, model.ni_loc

# the parent route's buffers: the same shapes as the view's
E2, b2, tmp_b = torch.zeros_like(view.E_item), torch.zeros_like(view.b_item), torch.zeros_like(view.b_item)
bag = (model.bag_vals, model.bag_starts, model.bag_lens)
ids_ready = (torch.arange(ni, dtype=torch.int32, device=dev) * W + r).contiguous()


def parent_route():
    ids = torch.arange(ni, dtype=torch.int32, device=dev) * W + r
    ops.gather_id_plus_bag(model.E_item, model.b_item, model.lmap, model.E_tok, model.b_tok, *bag, ids, E2[:ni],
                           scale=0.5, bias_out=tmp_b[:ni])
    ops.copy_strided(tmp_b[:ni], b2[:ni])


def parent_gather():
    ops.gather_id_plus_bag(model.E_item, model.b_item, model.lmap, model.E_tok, model.b_tok, *bag, ids_ready, E2[:ni],
                           scale=0.5, bias_out=b2[:ni])


users = np.arange(B)
routes = (('refresh_ms', view.refresh), ('parent_route_ms', parent_route), ('parent_gather_ms', parent_gather),
          ('recommend_ms', lambda: view.recommend(users, k)))
for _, fn in routes:                                     # every shape once, then once more: code objects, buffers
    fn()
    fn()
torch.cuda.synchronize()
same = bool(torch.equal(view.E_item, E2) and torch.equal(view.b_item, b2))
times = {name: [] for name, _ in routes}
for _ in range(args.rounds):
    for name, fn in routes:
        times[name].append(events_ms(fn, args.calls if name != 'recommend_ms' else max(1, args.calls // 3)))

row = dict(V=V, tokens=nt, mean_bag=float(lens.mean()), d=d, B=B, k=k, rounds=args.rounds, calls=args.calls,
           device=torch.cuda.get_device_name(0), same_latents_as_parent_route=same)
for name, ts in times.items():
    row[name] = round(statistics.median(ts), 4)
    row[name + '_min_max'] = [round(min(ts), 4), round(max(ts), 4)]
spread = max(times['parent_route_ms']) - min(times['parent_route_ms'])
row['parent_route_spread_ms'] = round(spread, 4)
row['refresh_not_slower_than_parent_route'] = bool(row['refresh_ms'] <= row['parent_route_ms'] + spread)
row['refresh_over_parent_gather'] = round(row['refresh_ms'] / row['parent_gather_ms'], 4)
need = (float(lens.sum()) + 2.0 * ni) * (d + 1) * 4.0 + float(lens.sum()) * 4.0 + 2.0 * ni * 4.0
row['refresh_bytes_needed'] = int(need)
row['refresh_tb_per_s'] = round(need / (row['refresh_ms'] * 1e-3) / 1e12, 3)
print(json.dumps(row), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(row, f, indent=1)
dist.destroy_process_group()
