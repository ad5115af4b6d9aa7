"""list_logprob (TopKScan.list_logp: arx_list_logp.h) against the mass pass + finish alone on the same lists and against
a torch composition of the same quantity, on random rows.

usage: python tools/list_logprob_bench.py [--B 4096] [--V 1000000] [--d 128,64,32] [--k 100] [--tau 1]
                                          [--rounds 3] [--calls 3] [--check-rows 16] [--out FILE.json]
The lists are each row's plain top-k shuffled (every entry drawable); a second run per width makes 10 % of the entries
impossible: half of them excluded (exclusion lists that hold exactly those columns), half repeats of an earlier entry.
(a) list_logp: prepare, streaming mass pass, finish, stamp.  (b) sort, the same mass pass and finish on the cleaned
lists -- what the draw's own propensities cost.  (c) torch, given the cleaned lists: chunks of 65536 columns,
lat @ pool[c].T + b, the entries' columns set to -inf (scatter; a spare column takes those of other chunks), logsumexp of
the chunk / tau, the chunks joined by logaddexp, then the entries' scores / tau in reverse order through logcumsumexp on
top of the rest (no exclusion mask: that favours torch).  The three alternate inside each round (device-event timing,
warm-up first); the median per call is reported.  prepare and stamp are also timed alone (--small-calls launches in one
window).  Accuracy: the largest |logp - float64| / tolerance over --check-rows rows at full size
(tests/list_logprob_oracle.py on the device's own logits of those rows) and the codes against the oracle's."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-recsys_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from arx import graph as G  # noqa: E402
from arx import ops  # noqa: E402
from arx.topk import ListLogpBuffers, StreamTopK, sample_params  # noqa: E402
import list_logprob_oracle as LL  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--V", type=int, default=1000000)
ap.add_argument("--d", default="128,64,32")
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--tau", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--small-calls", type=int, default=200)
ap.add_argument("--check-rows", type=int, default=16)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, V, k, tau = args.B, args.V, args.k, args.tau
dev = torch.device('cuda', 0)
rt = G.Runtime(dev)
g = torch.Generator(device=dev)
g.manual_seed(0)
CH = 65536


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


def spoil(lists, rng):
    """10 % of the entries made impossible: half excluded (-> the rows' exclusion lists), half repeats of the entry
    before them in the list.  -> (lists, ex_lists per row)"""
    out = lists.copy()
    n = max(2, k // 10)
    ex_lists = []
    for r in range(len(out)):
        at = rng.choice(np.arange(1, k), n, replace=False)
        ex_lists.append(np.unique(out[r, at[:n // 2]]))
        for j in np.sort(at[n // 2:]):
            out[r, j] = out[r, j - 1]
    return out, ex_lists


results = []
rng = np.random.default_rng(0)
for d in [int(x) for x in args.d.split(",")]:
    lat, pool = Leaf((B, d), 0.3), Leaf((V, d), 0.3)
    pool.bias_value = torch.randn(V, device=dev, generator=g) * 0.1
    tf, words = sample_params(tau, 0, B)
    sargs = (torch.from_numpy(tf).to(dev), B, torch.from_numpy(words).to(dev))
    scan = StreamTopK(rt, lat, pool, k)
    scan.forward(False)
    assert not scan.overflowed() and scan.mass_streams(lat.value, pool.value)
    top = scan.indices.cpu().numpy().astype(np.int64)
    shuffled = np.stack([rng.permutation(r) for r in top])
    xbuf = torch.empty((B, CH + 1), device=dev)
    # the device's own logits of a few rows, for the float64 check
    rows = np.linspace(0, B - 1, min(B, args.check_rows)).astype(np.int64)
    L = np.empty((len(rows), V), dtype=np.float32)
    lr = lat.value[torch.from_numpy(rows).to(dev)].contiguous()
    for c0 in range(0, V, CH):
        c1 = min(V, c0 + CH)
        x = torch.empty((len(rows), c1 - c0), device=dev)
        ops.gemm(lr, pool.value[c0:c1], x, rt.ws, transB=True, col_bias=pool.bias_value[c0:c1])
        L[:, c0:c1] = x.cpu().numpy()
    for spoiled in (False, True):
        lists, ex_lists = spoil(shuffled, rng) if spoiled else (shuffled, None)
        ex = None
        if spoiled:
            ptr = np.zeros(B + 1, dtype=np.int32)
            ptr[1:] = np.cumsum([len(x) for x in ex_lists])
            ex = (torch.arange(B, dtype=torch.int32, device=dev), B, torch.from_numpy(ptr).to(dev),
                  torch.from_numpy(np.concatenate(ex_lists + [np.zeros(1, np.int64)]).astype(np.int32)).to(dev))
        d_lists = torch.from_numpy(lists.astype(np.int32)).to(dev)
        lb, lb2 = ListLogpBuffers(B, k, dev), ListLogpBuffers(B, k, dev)
        logp, values = (torch.empty((B, k), dtype=torch.float32, device=dev) for _ in range(2))
        logp2, values2 = (torch.empty((B, k), dtype=torch.float32, device=dev) for _ in range(2))
        why, why2 = (torch.empty((B, k), dtype=torch.int32, device=dev) for _ in range(2))

        def full():                                                   # (a)
            scan.list_logp(lat.value, pool.value, pool.bias_value, rt.ws, d_lists, ex, None, sargs, logp, values, why,
                           lb=lb)
        full()
        clean = lb.clean.clone()
        picks = clean.long()

        def mass_only():                                              # (b)
            m_part, s_part, P = scan.mass_pass(lat.value, pool.value, pool.bias_value, rt.ws, clean, ex, None, sargs,
                                               True, lb2)
            ops.sample_logp_finish(clean, lb2.pick_score, m_part, s_part, P, sargs, logp2, values2)

        def composed():                                               # (c)
            rest = torch.full((B,), float('-inf'), device=dev)
            sc = torch.full((B, k), float('-inf'), device=dev)
            for c0 in range(0, V, CH):
                c1 = min(V, c0 + CH)
                w = c1 - c0
                x = xbuf[:, :w + 1]
                torch.addmm(pool.bias_value[c0:c1], lat.value, pool.value[c0:c1].T, out=xbuf[:, :w])
                x[:, w] = float('-inf')
                inside = (picks >= c0) & (picks < c1)
                loc = torch.where(inside, picks - c0, torch.full_like(picks, w))
                sc = torch.where(inside, torch.gather(x, 1, loc), sc)
                x.scatter_(1, loc, float('-inf'))
                rest = torch.logaddexp(rest, torch.logsumexp(x / tau, 1))
            a = sc / tau
            suffix = torch.logcumsumexp(torch.cat([rest[:, None], a.flip(1)], 1), 1)[:, 1:].flip(1)
            return a - suffix

        def prepare():
            ops.list_logp_prepare(d_lists, V, ex, None, lb2.clean, why2, lb2.pk_cols, lb2.pk_slot)

        def stamp():
            ops.list_logp_stamp(clean, lb.pick_score, why2, logp2, values2)

        fns = (full, mass_only, composed)
        for f in fns + (prepare, stamp):                              # warm-up
            f()
            f()
        torch.cuda.synchronize()
        t = [[], [], []]
        small = [[], []]
        for _ in range(args.rounds):                                  # alternated
            for i, f in enumerate(fns):
                t[i].append(timed(f, args.calls))
            small[0].append(timed(prepare, args.small_calls))
            small[1].append(timed(stamp, args.small_calls))
        ma, mb, mc = (statistics.median(x) for x in t)
        mp, ms = (statistics.median(x) for x in small)
        full()
        glp, gwhy = logp.cpu().numpy()[rows], why.cpu().numpy()[rows]
        tr = np.full(len(rows), tau)
        exp, codes, tol = LL.logp(L, lists[rows], tr, ex_lists=[ex_lists[r] for r in rows] if spoiled else None)
        ok = codes == LL.OK
        worst = float((np.abs(glp[ok].astype(np.float64) - exp[ok]) / tol[ok]).max())
        live = clean >= 0
        tdiff = float((composed() - logp)[live].abs().max().item())
        row = dict(B=B, V=V, d=d, k=k, tau=tau, spoiled=spoiled, list_logp_ms=round(ma, 4),
                   mass_and_finish_ms=round(mb, 4), torch_ms=round(mc, 4), prepare_ms=round(mp, 5),
                   stamp_ms=round(ms, 5), a_over_b=round(ma / mb, 4), c_over_a=round(mc / ma, 4),
                   small_share_of_b=round((mp + ms) / mb, 5), codes_equal=bool((gwhy == codes).all()),
                   drawable_share=round(float(live.float().mean().item()), 4), worst_err_over_tol=round(worst, 4),
                   torch_minus_device_max=tdiff,
                   **{n + '_ms_all': [round(x, 4) for x in t[i]]
                      for i, n in enumerate(('list_logp', 'mass_and_finish', 'torch'))})
        results.append(row)
        print("d %-4d %-8s (a) list_logp %8.3f ms  (b) mass + finish %8.3f ms  (a)/(b) %.4f  (c) torch %8.3f ms  "
              "(c)/(a) %.2f  prepare %.4f ms  stamp %.4f ms  err/tol %.3f  codes %s  |torch - device| %.2g"
              % (d, 'spoiled' if spoiled else 'drawable', ma, mb, ma / mb, mc, mc / ma, mp, ms, worst,
                 row['codes_equal'], tdiff), flush=True)
    del scan, xbuf
    torch.cuda.empty_cache()
    del lat, pool
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
