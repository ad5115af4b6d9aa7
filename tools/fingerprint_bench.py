"""arx_rows_fingerprint against arx_copy_2d of the same array ('Checkpoints of the sharded
models'): device events, rounds of calls with the two kernels alternating, one process.  The copy moves twice the
bytes (read + write); the fingerprint only reads.

    python tools/fingerprint_bench.py [--rows 1000000] [--width 128] [--rounds 5] [--calls 20]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "a-recsys_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12          # bytes / s (spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    from arx import ops
    from arx.utils.checkpoint import rows_fingerprint
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    x = torch.empty((a.rows, a.width), dtype=torch.float32, device=dev).uniform_(-1, 1)
    y = torch.empty_like(x)
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    ops.rows_fingerprint(x, 3, 8, out)
    ops.copy_2d(x, y)
    torch.cuda.synchronize()
    n = min(a.rows, 20000)                                  # the result, against the numpy twin (a slice: host time)
    chk = torch.zeros(1, dtype=torch.int64, device=dev)
    ops.rows_fingerprint(x[:n], 3, 8, chk)
    assert int(chk.item()) & ((1 << 64) - 1) == rows_fingerprint(x[:n].cpu().numpy(), 3, 8)
    assert torch.equal(x, y)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    fp, cp = [], []
    for _ in range(a.rounds):
        fp.append(timed(lambda: ops.rows_fingerprint(x, 3, 8, out)))
        cp.append(timed(lambda: ops.copy_2d(x, y)))
    nbytes = a.rows * a.width * 4
    f, c = float(np.median(fp)), float(np.median(cp))
    print("rows %d width %d (%.1f MB)" % (a.rows, a.width, nbytes / 1e6))
    print("arx_rows_fingerprint  %.4f ms  (rounds %s)  %.2f TB/s read = %.1f %% of the 8 TB/s HBM peak"
          % (f, " ".join("%.4f" % v for v in fp), nbytes / f / 1e9, 100 * nbytes / (f * 1e-3) / HBM_PEAK))
    print("arx_copy_2d           %.4f ms  (rounds %s)  %.2f TB/s read + written"
          % (c, " ".join("%.4f" % v for v in cp), 2 * nbytes / c / 1e9))


if __name__ == "__main__":
    main()
