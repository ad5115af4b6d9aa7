"""Inputs, float64 references and tolerances of the LSTM kernel matrix (tests/test_lstm_kernels_gpu.py), shared with
tests/test_lstm_paths_cpu.py, which checks them before they meet a kernel.  Plain helpers, no fixtures; the reference is
oracle.ref_lstm and nothing else."""
import numpy as np

import lstm_paths as LP
from oracle import ref_lstm

F32, F64 = np.float32, np.float64
FORGET_BIASES = (0.0, 1.0, 2.5)
FACTOR = 8.0                    # kernel error <= FACTOR * e_ref + REL * |ref|
REL = 1e-6
FLT_MIN = float(np.finfo(F32).tiny)         # 2^-126: below it an f32 result is subnormal


# ---------------------------------------------------------------- the matrix
def matrix():
    """[(id, name, din, h, B token, L, forget_bias, hot)] -- the table of lstm_paths.table() crossed, forget_bias
    cycling through 0.0, 1.0, 2.5 inside every path, plus one 'hot' (saturating) variant per path.  A B token is an
    int, or one of 'w-1', 'w', 'w+15', 'w+24' with w = lstm_paths.wreg_min_B(cu) (resolved on the device)."""
    out = []
    cu0 = 10 ** 6                           # no device at collection time: B values near w become offsets from it
    tab = LP.table(cu0)
    w0 = LP.wreg_min_B(cu0)
    for name, (_, shapes, Bs, Ls) in tab.items():
        toks = [b if b < w0 - 1 else ('w' if b == w0 else 'w%+d' % (b - w0)) for b in Bs]
        i = 0
        for din, h in shapes:
            for tok in toks:
                for L in Ls:
                    fb = FORGET_BIASES[(i + (i // 3 if len(Ls) == 3 else 0)) % 3]     # (not in step with L)
                    out.append(("%s-d%d-h%d-B%s-L%d-fb%g" % (name, din, h, tok, L, fb), name, din, h, tok, L, fb,
                                False))
                    i += 1
        din, h = shapes[-1]
        tok = {'r4': 7, 'wreg': 'w+24', 'generic': 5}.get(name, 17)
        out.append(("%s-d%d-h%d-B%s-L%d-hot" % (name, din, h, tok, Ls[-1]), name, din, h, tok, Ls[-1], 1.0, True))
    return out


def resolve_B(tok, cu):
    if isinstance(tok, int):
        return tok
    w = LP.wreg_min_B(cu)
    return w + (int(tok[1:]) if len(tok) > 1 else 0)


# ---------------------------------------------------------------- inputs
def inputs(L, B, din, h, seed, hot=False):
    """x [L,B,din], W [din+h,4h], b [4h], dhs [L,B,h] in float32.  Plain: the scales of test_lstm_fwd_bwd (x 0.5,
    W 0.2, b 0.1): pre-activations of a few units.  Hot: W 1.5 and x 16 / sqrt(din), so the x part of a
    pre-activation has sigma 24 and the largest reach |z| of about 100: __expf overflows into rcp(inf), e = 0."""
    rng = np.random.default_rng(seed)
    sx, sw = (16.0 / np.sqrt(din), 1.5) if hot else (0.5, 0.2)
    x = (rng.standard_normal((L, B, din)) * sx).astype(F32)
    W = (rng.standard_normal((din + h, 4 * h)) * sw).astype(F32)
    b = (rng.standard_normal((4 * h,)) * 0.1).astype(F32)
    dhs = rng.standard_normal((L, B, h)).astype(F32)
    return x, W, b, dhs


def _maxabs(a, b):
    return float(np.max(np.abs(a.astype(F64) - b)))


def reference(x, W, b, dhs, fb):
    """The float64 oracle on casts of the f32 inputs, the same oracle on the f32 arrays themselves (it keeps its
    input dtype: a plain f32 restatement), and e_ref = max |f32 restatement - f64| per output array.

    dz comes twice: 'dz' continues each forward (the f64 backward from the f64 forward, the f32 one from the f32
    forward: what a kernel fed its own forward is compared with), 'dz_fed' starts both from the SAME f32-rounded
    oracle cells and gates ('cs32', 'g32': what the second backward run is fed)."""
    with np.errstate(over='ignore'):        # hot inputs: np.exp(-z) overflows to inf, 1 / (1 + inf) = 0 is meant
        x6, W6, b6, d6 = x.astype(F64), W.astype(F64), b.astype(F64), dhs.astype(F64)
        r_hs, r_cs, r_g = ref_lstm.lstm_fwd(x6, W6, b6, fb)
        f_hs, f_cs, f_g = ref_lstm.lstm_fwd(x, W, b, F32(fb))
        r_dz = ref_lstm.lstm_bwd(x6, W6, r_hs, r_cs, r_g, d6)[0]
        f_dz = ref_lstm.lstm_bwd(x, W, f_hs, f_cs, f_g, dhs)[0]
        cs32, g32 = r_cs.astype(F32), r_g.astype(F32)
        r_dzf = ref_lstm.lstm_bwd(x6, W6, r_hs, cs32.astype(F64), g32.astype(F64), d6)[0]
        f_dzf = ref_lstm.lstm_bwd(x, W, f_hs, cs32, g32, dhs)[0]
    assert f_hs.dtype == F32 and f_dz.dtype == F32 and f_dzf.dtype == F32
    ref = {'hs': r_hs, 'cs': r_cs, 'gates': r_g, 'dz': r_dz, 'dz_fed': r_dzf}
    e_ref = {'hs': _maxabs(f_hs, r_hs), 'cs': _maxabs(f_cs, r_cs), 'gates': _maxabs(f_g, r_g),
             'dz': _maxabs(f_dz, r_dz), 'dz_fed': _maxabs(f_dzf, r_dzf)}
    return ref, e_ref, cs32, g32


def ratio(got, ref, e_ref):
    """max over elements of err / (e_ref + REL * |ref| / FACTOR): the check passes iff this is <= FACTOR."""
    err = np.abs(got.astype(F64) - ref)
    return float(np.max(err / (e_ref + REL * np.abs(ref) / FACTOR))), float(err.max())


def poison_rows(B):
    """Rows to fill with NaN: inside full tiles (1, 6), the middle, and next to the last row (inside the tail tile
    when there is one); rows 0 and B - 1 stay clean beside them.  None at B < 3."""
    return sorted({r for r in (1, 6, B // 2, B - 2) if 0 < r < B - 1})


# ---------------------------------------------------------------- gate functions alone (one-hot weights)
def gate_sweep():
    """Non-negative sweep values in ascending order (float32); the test runs them and their negatives.
    -> (values, number of leading band values around the 1/16 seam)"""
    seam = F32(0.0625)
    near = [seam]
    lo = hi = seam
    for _ in range(3):
        lo, hi = np.nextafter(lo, F32(0)), np.nextafter(hi, F32(1))
        near += [lo, hi]
    band = np.unique(np.concatenate([np.linspace(0.05, 0.08, 1201).astype(F32), np.array(near, F32)]))
    rest = np.array([0.0, 1e-45, 1e-40, 5e-39, FLT_MIN, 1e-4, 1.0, 8.3, 9.1, 17.0, 88.0, 89.0, 104.0], F32)
    return np.concatenate([band, rest]), len(band)


def onehot_case(h, g, bias=None):
    """din == h, W[k, g*h + k] = 1 and all else 0, so the step-0 pre-activation of gate g, unit k is exactly
    x[row, k] (products 1 * x and 0 * x: nothing is rounded) and gates[0][:, g*h + k] is the gate function of the
    sweep.  b and the h rows of W are -0.0 (so a row of -0.0 sums to -0.0) unless `bias` [4] gives one value per gate.

    x [1, B, h]: the sweep and its negatives row-major (padded with 0.5), then a row of +0.0, a row of -0.0, and
    three rows that hold +inf, -inf, NaN in unit 0 and zeros elsewhere (0 * inf is NaN: those rows are read at
    gate g, unit 0 alone).  -> x, W, b, vals (the 2n sweep values: vals[i] sits at row i // h, unit i % h),
    rows = {'pz', 'nz', 'pinf', 'ninf', 'nan'}"""
    pos, _ = gate_sweep()
    vals = np.concatenate([pos, -pos]).astype(F32)
    nrow = -(-len(vals) // h)
    x = np.full((nrow + 5, h), 0.5, F32)
    x.reshape(-1)[:len(vals)] = vals
    rows = {'pz': nrow, 'nz': nrow + 1, 'pinf': nrow + 2, 'ninf': nrow + 3, 'nan': nrow + 4}
    x[nrow] = 0.0
    x[nrow + 1] = -0.0
    x[nrow + 2:] = 0.0
    x[nrow + 2, 0], x[nrow + 3, 0], x[nrow + 4, 0] = np.inf, -np.inf, np.nan
    W = np.zeros((2 * h, 4 * h), F32)
    W[h:] = -0.0                # h_{-1} is +0: its products are -0 and leave a pre-activation of -0 alone
    W[np.arange(h), g * h + np.arange(h)] = 1.0
    b = np.full(4 * h, -0.0, F32)
    if bias is not None:
        b = np.repeat(np.asarray(bias, F32), h)
    return x[None], W, b, vals, rows
