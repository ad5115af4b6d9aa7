"""Every dispatch path of csrc/gru.hip against the float64 oracle, at its edges -- the method of
tests/test_lstm_kernels_gpu.py applied case by case (ratio, FACTOR, REL and poison_rows are lstm_cases' own).

arx_gru_fwd / arx_gru_bwd choose among three kernel pairs by (din, h) alone (tests/gru_paths.py restates the rule);
every case here asserts through that module that it runs the pair it names.

The matrix (test_gru_case; shapes from gru_paths.table()):
  * reference: tests/gru_oracle.py on float64 casts of the f32 inputs.  The same oracle on the f32 arrays is a plain
    f32 restatement; e_ref = max |f32 restatement - f64| per output array, and the kernel's error against f64 may be
    at most 8 * e_ref + 1e-6 * |ref| elementwise, for hs, gates, rh, dzg and dzc (8: the LSTM's factor -- the chain
    lengths and the gate functions are the same)
  * an array whose reference is identically zero in both precisions has e_ref = 0 and no ratio: rh at L = 1
    (r * h_{-1}, h_{-1} = 0).  There the kernel's array must be zero too, every element
  * backward twice: fed the kernel's own forward (as the model does), and fed the oracle's f32-rounded hs and gates
    (so a backward error cannot hide behind a compensating forward one)
  * canaries: hs, gates, rh, dzg, dzc carry 16 spare rows behind the last step, prefilled with a sentinel: the spare
    rows come back untouched and every live element has been overwritten
  * row independence: chosen rows of x (of dhs for backward) are NaN; exactly those rows come out NaN and every other
    row is bit-equal to the clean run
  * determinism: two runs are bit-equal
  * one 'hot' variant on wreg and mfma has pre-activations up to |z| of about 100 (lstm_cases.inputs(hot=True)'s
    scales: __expf overflow into rcp(inf), e = 0)
test_gru_grads: seqModel.gru_grads (the node's gradient composition) on plain tensors, per path at L = 1 (the h halves
  of dWg and dWc are zero) and L = 3: dx, dWg, dbg, dWc, dbc under the same bound, e_ref from the f32 oracle's arrays.
test_empty_calls: L == 0 and B == 0 return OK and leave every output at its sentinel.

MEASURED on an MI355X (test_zz_report prints these).  Largest err / (e_ref + 1e-6 |ref| / 8) per path and array -- the
check is "<= 8"; no kernel needed more, so 8 stands:
    path      gates   rh     hs     dzg    dzc    dzg (fed)  dzc (fed)
    wreg      1.47    1.46   1.63   1.71   1.80   0.84       0.70
    mfma1     1.10    1.13   1.10   1.19   1.20   0.79       0.72
    mfma2     1.11    1.31   1.09   1.71   1.08   0.90       1.02
    generic   1.68    2.18   1.72   1.45   1.29   2.42       1.21
    grads     dx 1.31   dWg 1.22   dbg 1.04   dWc 1.05   dbc 1.39
Wall time of the module: 2.7 s for 53 cases.
"""
import time

import numpy as np
import pytest

import gru_oracle as GO
import gru_paths as GP
from lstm_cases import FACTOR, REL, poison_rows, ratio

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT = 55.0                     # what every output element holds before a kernel writes it
SPARE = 16                      # spare rows behind the last step
_WORST = {}                     # path -> {array: (ratio, case id)}
_T0 = time.time()


# ---------------------------------------------------------------- the matrix, inputs, references
def matrix():
    """[(id, name, din, h, B, L, hot)]: gru_paths.table() crossed, plus one hot variant on wreg and on mfma."""
    out = []
    for name, (shapes, Bs, Ls) in GP.table().items():
        for din, h in shapes:
            for B in Bs:
                for L in Ls:
                    out.append(("%s-d%d-h%d-B%d-L%d" % (name, din, h, B, L), name, din, h, B, L, False))
        if name != 'generic':
            din, h = shapes[-1]
            out.append(("%s-d%d-h%d-B17-L%d-hot" % (name, din, h, Ls[-1]), name, din, h, 17, Ls[-1], True))
    return out


def inputs(L, B, din, h, seed, hot=False):
    """x, Wg, bg, Wc, bc, dhs in float32, at the scales of lstm_cases.inputs: plain x 0.5, W 0.2, b 0.1; hot W 1.5 and
    x 16 / sqrt(din), so the x part of a pre-activation has sigma 24 and the largest reach |z| of about 100."""
    rng = np.random.default_rng(seed)
    sx, sw = (16.0 / np.sqrt(din), 1.5) if hot else (0.5, 0.2)
    x = (rng.standard_normal((L, B, din)) * sx).astype(F32)
    Wg = (rng.standard_normal((din + h, 2 * h)) * sw).astype(F32)
    bg = (rng.standard_normal((2 * h,)) * 0.1).astype(F32)
    Wc = (rng.standard_normal((din + h, h)) * sw).astype(F32)
    bc = (rng.standard_normal((h,)) * 0.1).astype(F32)
    dhs = rng.standard_normal((L, B, h)).astype(F32)
    return x, Wg, bg, Wc, bc, dhs


def _maxabs(a, b):
    return float(np.max(np.abs(a.astype(F64) - b)))


def reference(x, Wg, bg, Wc, bc, dhs):
    """The float64 oracle on casts of the f32 inputs, the same oracle on the f32 arrays, and e_ref per array.
    'dzg' / 'dzc' and the parameter gradients continue each forward; 'dzg_fed' / 'dzc_fed' start both precisions from
    the SAME f32-rounded oracle hs and gates ('hs32', 'g32': what the second backward run is fed)."""
    with np.errstate(over='ignore'):        # hot inputs: np.exp(-z) overflows to inf, 1 / (1 + inf) = 0 is meant
        a6 = [v.astype(F64) for v in (x, Wg, bg, Wc, bc, dhs)]
        r_hs, r_g, r_rh = GO.gru_fwd(*a6[:5])
        f_hs, f_g, f_rh = GO.gru_fwd(x, Wg, bg, Wc, bc)
        r_b = GO.gru_bwd(a6[0], a6[1], a6[3], r_hs, r_g, a6[5])
        f_b = GO.gru_bwd(x, Wg, Wc, f_hs, f_g, dhs)
        hs32, g32 = r_hs.astype(F32), r_g.astype(F32)
        r_f = GO.gru_bwd(a6[0], a6[1], a6[3], hs32.astype(F64), g32.astype(F64), a6[5])
        f_f = GO.gru_bwd(x, Wg, Wc, hs32, g32, dhs)
    assert f_hs.dtype == F32 and f_b[0].dtype == F32 and f_f[0].dtype == F32
    names = ('dzg', 'dzc', 'dx', 'dWg', 'dbg', 'dWc', 'dbc')
    ref = {'hs': r_hs, 'gates': r_g, 'rh': r_rh, 'dzg_fed': r_f[0], 'dzc_fed': r_f[1]}
    ref.update(zip(names, r_b))
    e_ref = {'hs': _maxabs(f_hs, r_hs), 'gates': _maxabs(f_g, r_g), 'rh': _maxabs(f_rh, r_rh),
             'dzg_fed': _maxabs(f_f[0], r_f[0]), 'dzc_fed': _maxabs(f_f[1], r_f[1])}
    e_ref.update((k, _maxabs(f, r)) for k, f, r in zip(names, f_b, r_b))
    return ref, e_ref, hs32, g32


# ---------------------------------------------------------------- plumbing (as the LSTM module's)
def _t(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_SENT_BITS = _bits(np.float32(SENT)).item()


def _buf(dev, rows, cols):
    import torch
    return torch.full((rows + SPARE, cols), SENT, dtype=torch.float32, device=dev)


def _live(buf, L, B, what, written=True):
    """The [L, B, cols] live part of a canaried buffer, after checking the spare rows (and that no live element still
    holds the sentinel, or with written=False that every one does)."""
    a = buf.cpu().numpy()
    n = L * B
    assert np.all(_bits(a[n:]) == _SENT_BITS), "%s: spare rows behind the last step were written" % what
    if not written:
        assert np.all(_bits(a[:n]) == _SENT_BITS), "%s: written by a call that had nothing to do" % what
        return None
    kept = int(np.count_nonzero(_bits(a[:n]) == _SENT_BITS))
    assert kept == 0, "%s: %d live elements were never written" % (what, kept)
    return a[:n].reshape(L, B, -1)


def _fwd(dev, x, tw, h):
    from arx import ops
    L, B, din = x.shape
    hs, gates, rh = _buf(dev, L * B, h), _buf(dev, L * B, 3 * h), _buf(dev, L * B, h)
    ops.gru_fwd(_t(dev, x), tw[0], tw[1], tw[2], tw[3], L, B, din, h, hs, gates, rh)
    return hs, gates, rh


def _bwd(dev, tw, hs, gates, dhs, din):
    from arx import ops
    L, B, h = dhs.shape
    dzg, dzc = _buf(dev, L * B, 2 * h), _buf(dev, L * B, h)
    ops.gru_bwd(tw[0], tw[2], hs, gates, _t(dev, dhs), L, B, din, h, dzg, dzc)
    return dzg, dzc


def _within(cid, path, what, got, ref, e_ref):
    if e_ref == 0.0 and not ref.any():      # identically zero in both precisions (rh at L = 1): no yardstick, so exact
        print("  %-8s reference identically zero: the kernel's array must be" % what)
        assert not got.any(), "%s %s: the reference is identically zero, the kernel's array is not" % (cid, what)
        return
    assert np.isfinite(e_ref) and e_ref > 0.0, (cid, what, e_ref)
    r, err = ratio(got, ref, e_ref)
    print("  %-8s e_ref %.3e  kernel err %.3e  ratio %.2f" % (what, e_ref, err, r))
    w = _WORST.setdefault(path, {})
    if r > w.get(what, (0.0, None))[0]:
        w[what] = (r, cid)
    assert r <= FACTOR, "%s %s: error %.3e is %.2f x (e_ref %.3e + 1e-6 |ref| / 8), more than %g" % (
        cid, what, err, r, e_ref, FACTOR)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d entries differ, first at %s" % (what, len(bad), bad[0].tolist()))


def _rows_independent(clean, dirty, rows, what):
    """Rows `rows` (axis 1) of `dirty` are all NaN; every other row is bit-equal to `clean`."""
    keep = np.setdiff1d(np.arange(clean.shape[1]), rows)
    assert np.all(np.isnan(dirty[:, rows])), "%s: a poisoned row came out with numbers in it" % what
    _same_bits(dirty[:, keep], clean[:, keep], what + " (rows beside the poisoned ones)")


_MATRIX = matrix()
FWD, BWD = ('hs', 'gates', 'rh'), ('dzg', 'dzc')


@pytest.mark.parametrize("cid,name,din,h,B,L,hot", _MATRIX, ids=[c[0] for c in _MATRIX])
def test_gru_case(dev, cid, name, din, h, B, L, hot):
    assert GP.on_path(name, din, h), (name, din, h, GP.path(din, h))
    path = GP.path(din, h)
    seed = [c[0] for c in _MATRIX].index(cid) + 1
    x, Wg, bg, Wc, bc, dhs = inputs(L, B, din, h, seed, hot)
    ref, e_ref, hs32, g32 = reference(x, Wg, bg, Wc, bc, dhs)
    print("\n%s: path %s" % (cid, path))
    tw = [_t(dev, a) for a in (Wg, bg, Wc, bc)]
    n = L * B
    # ---- forward: canaries, tolerance, determinism, row independence
    f = _fwd(dev, x, tw, h)
    out = {k: _live(t, L, B, k) for k, t in zip(FWD, f)}
    for k in ('gates', 'rh', 'hs'):
        _within(cid, path, k, out[k], ref[k], e_ref[k])
    for k, t2 in zip(FWD, _fwd(dev, x, tw, h)):
        _same_bits(_live(t2, L, B, k), out[k], k + ": second forward run")
    rows = poison_rows(B)
    if rows:
        xp = x.copy()
        xp[:, rows] = np.nan
        for k, t2 in zip(FWD, _fwd(dev, xp, tw, h)):
            _rows_independent(out[k], _live(t2, L, B, k + " (poisoned x)"), rows, k)
    # ---- backward, fed the kernel's own forward
    hs_t, g_t = f[0][:n], f[1][:n]
    b = {k: _live(t, L, B, k) for k, t in zip(BWD, _bwd(dev, tw, hs_t, g_t, dhs, din))}
    for k in BWD:
        _within(cid, path, k, b[k], ref[k], e_ref[k])
    for k, t2 in zip(BWD, _bwd(dev, tw, hs_t, g_t, dhs, din)):
        _same_bits(_live(t2, L, B, k), b[k], k + ": second backward run")
    if rows:
        dp = dhs.copy()
        dp[:, rows] = np.nan
        for k, t2 in zip(BWD, _bwd(dev, tw, hs_t, g_t, dp, din)):
            _rows_independent(b[k], _live(t2, L, B, k + " (poisoned dhs)"), rows, k)
    # ---- backward, fed the oracle's f32-rounded hs and gates
    fed = _bwd(dev, tw, _t(dev, hs32.reshape(n, h)), _t(dev, g32.reshape(n, 3 * h)), dhs, din)
    for k, t2 in zip(BWD, fed):
        _within(cid, path, k + '_fed', _live(t2, L, B, k + ' (oracle-fed)'), ref[k + '_fed'], e_ref[k + '_fed'])


_GRADS = [('wreg', 64, 64, 17), ('mfma', 68, 64, 33), ('generic', 64, 96, 3)]


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("name,din,h,B", _GRADS, ids=[g[0] for g in _GRADS])
def test_gru_grads(dev, name, din, h, B, L):
    """The node's gradient composition on plain tensors, behind the kernels' own forward and backward."""
    import torch
    from arx import ops
    from arx.lstm.seqModel import gru_grads
    assert GP.on_path(name, din, h)
    cid = "grads-%s-L%d" % (name, L)
    x, Wg, bg, Wc, bc, dhs = inputs(L, B, din, h, 100 + L + din, False)
    ref, e_ref, _, _ = reference(x, Wg, bg, Wc, bc, dhs)
    tw = [_t(dev, a) for a in (Wg, bg, Wc, bc)]
    n = L * B
    tx = _t(dev, x.reshape(n, din))
    hs, gates, rh = _buf(dev, n, h), _buf(dev, n, 3 * h), _buf(dev, n, h)
    ops.gru_fwd(tx, tw[0], tw[1], tw[2], tw[3], L, B, din, h, hs, gates, rh)
    dzg, dzc = _buf(dev, n, 2 * h), _buf(dev, n, h)
    ops.gru_bwd(tw[0], tw[2], hs, gates, _t(dev, dhs), L, B, din, h, dzg, dzc)

    def full(*shape):
        return torch.full(shape, SENT, dtype=torch.float32, device=dev)
    dx, dWg, dbg, dWc, dbc = full(n, din), full(din + h, 2 * h), full(2 * h), full(din + h, h), full(h)
    scratch = (full(2 * h, din + h), full(h, din + h))
    ws = ops.Workspace(dev)
    gru_grads(ws, tx, hs[:n], rh[:n], dzg[:n], dzc[:n], tw[0], tw[2], L, B, dWg, dbg, dWc, dbc, scratch,
              dx=dx, dx_beta=0.0)
    print("\n%s" % cid)
    got = {'dx': dx.cpu().numpy().reshape(L, B, din), 'dWg': dWg.cpu().numpy(), 'dbg': dbg.cpu().numpy(),
           'dWc': dWc.cpu().numpy(), 'dbc': dbc.cpu().numpy()}
    for k, a in got.items():
        assert not np.any(_bits(a) == _SENT_BITS), "%s: elements never written" % k
        _within(cid, 'grads', k, a, ref[k], e_ref[k])
    if L == 1:
        assert not got['dWg'][din:].any() and not got['dWc'][din:].any(), "h halves at L = 1 are not zero"
    # dx_beta = 1 adds onto what dx holds: started from the first result it ends at twice it (halving is exact)
    dx2 = dx.clone()
    gru_grads(ws, tx, hs[:n], rh[:n], dzg[:n], dzc[:n], tw[0], tw[2], L, B, dWg, dbg, dWc, dbc, scratch,
              dx=dx2, dx_beta=1.0)
    _within(cid, 'grads', 'dx', dx2.cpu().numpy().reshape(L, B, din) * F32(0.5), ref['dx'], e_ref['dx'])


_EMPTY = [('wreg', 64, 64), ('mfma', 68, 64), ('mfma', 64, 128), ('generic', 6, 64)]


@pytest.mark.parametrize("name,din,h", _EMPTY, ids=["%s-h%d" % (e[0], e[2]) for e in _EMPTY])
def test_empty_calls(dev, name, din, h):
    """L == 0 and B == 0: OK, nothing written."""
    import torch
    from arx import ops
    assert GP.on_path(name, din, h)
    Wg, bg, Wc, bc = inputs(1, 1, din, h, 3)[1:5]
    tw = [_t(dev, a) for a in (Wg, bg, Wc, bc)]
    some = torch.zeros((SPARE, max(din, 3 * h)), dtype=torch.float32, device=dev)    # never read: L * B == 0
    for L_, B_ in ((0, 17), (3, 0)):
        hs, gates, rh = _buf(dev, 0, h), _buf(dev, 0, 3 * h), _buf(dev, 0, h)
        dzg, dzc = _buf(dev, 0, 2 * h), _buf(dev, 0, h)
        ops.gru_fwd(some, tw[0], tw[1], tw[2], tw[3], L_, B_, din, h, hs, gates, rh)
        ops.gru_bwd(tw[0], tw[2], some, some, some, L_, B_, din, h, dzg, dzc)
        for k, t in (('hs', hs), ('gates', gates), ('rh', rh), ('dzg', dzg), ('dzc', dzc)):
            _live(t, 0, 0, "%s at L %d, B %d" % (k, L_, B_), written=False)


def test_zz_report():
    """Prints what the docstring records: the largest ratio per path and array."""
    print()
    for path in sorted(_WORST):
        print("  %-10s %s" % (path, "  ".join("%s %.2f" % (k, v[0]) for k, v in sorted(_WORST[path].items()))))
    print("  module wall time so far: %.1f s" % (time.time() - _T0))
