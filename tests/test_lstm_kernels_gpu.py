"""Every dispatch path of csrc/lstm.hip against the float64 oracle, at its edges.

arx_lstm_fwd / arx_lstm_bwd choose among five kernel pairs (tests/lstm_paths.py restates the rules); every case here
asserts through that module that it runs the pair it names, with the CU count read from the device.

The matrix (test_lstm_case; shapes from lstm_paths.table(), inputs and references from tests/lstm_cases.py):
  * reference: oracle.ref_lstm on float64 casts of the f32 inputs.  The same oracle on the f32 arrays is a plain f32
    restatement; e_ref = max |f32 restatement - f64| per output array, and the kernel's error against f64 may be at
    most 8 * e_ref + 1e-6 * |ref| elementwise (8: the accumulation order -- four interleaved partial chains over
    K <= 260 where numpy sums differently; 1e-6: the fast gate functions, below)
  * backward twice: fed the kernel's own forward (as the model does), and fed the oracle's f32-rounded cells and gates
    (so a backward error cannot hide behind a compensating forward one; this run passes wxt=None)
  * canaries: hs, cs, gates, dz carry 16 spare rows behind the last step, prefilled with a sentinel: the spare rows
    come back untouched and every live element has been overwritten
  * row independence: chosen rows of x (of dhs for backward) are NaN; exactly those rows come out NaN and every other
    row is bit-equal to the clean run -- the check for a wrong A-operand lane map or quad exchange in a tail tile
  * determinism: two runs are bit-equal
  * wxt given: equals W[:din].T exactly, on r4 (its kernel writes it) and elsewhere (a launch of its own)
  * forget_bias cycles through 0.0, 1.0, 2.5 on every path; one 'hot' variant per path has pre-activations up to
    |z| of about 100 (__expf overflow into rcp(inf), e = 0)
test_wreg_slice_matches_r4: 64 rows of the big wreg batch rerun alone take r4 and agree with the big call within the
  same tolerance.  Bit equality is NOT expected: wreg sums a pre-activation in one chain per 16x16x4 MFMA, r4 in four
  interleaved chains of 4x4x1 MFMAs.
test_wxt_empty_calls: at L == 0 and at B == 0 the calls return OK, wxt is still filled and every other output keeps
  its sentinel.
test_gate_functions / test_cell_tanh: sigmoidf_ / tanhf_ alone through one-hot weights (lstm_cases.onehot_case), on
  r4, mfma2 and generic -- every copy of the forward epilogue but wreg's, which shares the device functions.  Bound:
  1e-6 relative (just above 1/16, e = exp(-2x) is about 0.88 and one ulp of v_exp_f32 is amplified by e / (1 - e) of
  about 7.5 into 4.5e-7; the 1 + e sum and the rcp add about an ulp each).  Where the exact result is below 2^-126
  (sigmoid(-88) and beyond, tanh of a denormal) an f32 result is subnormal and carries no relative precision in any
  implementation -- v_exp_f32 / v_rcp_f32 flush there -- so those points are held to an absolute 2^-126 instead.
test_lds_boundary / test_lds_limit_raises: dynamic LDS at exactly 64 KB, just past it (the kernels are opted in with
  hipFuncAttributeMaxDynamicSharedMemorySize there; the ROCm 7.2 runtime also launched them without it), and past
  160 KB (an argument error ahead of any launch, outputs untouched).

MEASURED on an MI355X (256 CUs; test_zz_report prints these).  Largest err / (e_ref + 1e-6 |ref| / 8) per path and
array -- the check is "<= 8"; no correct kernel needed more, so 8 stands:
    path         gates   cs     hs     dz     dz (oracle-fed)
    r4           1.26    1.03   1.08   1.37   0.99
    wreg         1.08    1.08   1.40   1.60   0.63
    mfma1        1.87    1.79   2.19   1.91   1.96
    mfma2        3.86    3.62   5.57   2.67   2.37
    generic fwd  2.45    2.49   1.90   1.85   1.59      (k_lstm_fwd_generic, then k_lstm_bwd<TPG>)
    generic      2.66    2.97   3.71   2.66   3.71
    LDS mfma2    0.78    0.76   0.74   1.74   --        (K = 508 / 512)
    LDS generic  2.04    2.04   2.75   6.16   --        (h = 2731: dh sums 10924 terms in one fmaf chain)
Gate functions, largest relative error against float64, the same on r4, mfma2 and generic: sigmoidf_ 4.28e-7 at
x = -9.1; tanhf_ 3.55e-7 at x = 0.0647 (just above the seam) and 6.1e-8 below the seam; tanhf_ of the cell 4.11e-7 at
c = 0.06536.  All under the 5e-7 the source comment claims and the 1e-6 asserted here.
Wall time of the module: 7 s for 208 cases; slowest case 0.7 s (r4 at B = 32 cu - 16, L = 5: the oracle's share).
"""
import time

import numpy as np
import pytest

import lstm_cases as LC
import lstm_paths as LP

pytestmark = pytest.mark.gpu

SENT = 55.0                     # what every output element holds before a kernel writes it
SPARE = 16                      # spare rows behind the last step
_CASES = {}
_WORST = {}                     # path -> {array: (ratio, case id)}
_GATE_WORST = {}                # (path, function) -> (relative error, x)
_T0 = time.time()


def _cu():
    from arx import ops
    return int(ops.device_info()["cu_count"])


def _once(key, build):
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


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
    if n == 0:
        return None
    kept = int(np.count_nonzero(_bits(a[:n]) == _SENT_BITS))
    if written:
        assert kept == 0, "%s: %d live elements were never written" % (what, kept)
    else:
        assert kept == a[:n].size, "%s: %d elements written by a call that had nothing to do" % (what, a[:n].size - kept)
    return a[:n].reshape(L, B, -1)


def _fwd(dev, x, tW, tb, fb, h):
    from arx import ops
    L, B, din = x.shape
    hs, cs, gates = _buf(dev, L * B, h), _buf(dev, L * B, h), _buf(dev, L * B, 4 * h)
    ops.lstm_fwd(_t(dev, x), tW, tb, L, B, din, h, fb, hs, cs, gates)
    return hs, cs, gates


def _bwd(dev, tW, cs, gates, dhs, din, wxt):
    from arx import ops
    L, B, h = dhs.shape
    dz = _buf(dev, L * B, 4 * h)
    ops.lstm_bwd(tW, cs, cs, gates, _t(dev, dhs), L, B, din, h, dz, wxt=wxt)      # (hs is unused by the kernels)
    return dz


def _within(cid, path, what, got, ref, e_ref):
    r, err = LC.ratio(got, ref, e_ref)
    print("  %-8s e_ref %.3e  kernel err %.3e  ratio %.2f" % (what, e_ref, err, r))
    w = _WORST.setdefault(path, {})
    if r > w.get(what, (0.0, None))[0]:
        w[what] = (r, cid)
    assert r <= LC.FACTOR, "%s %s: error %.3e is %.2f x (e_ref %.3e + 1e-6 |ref| / 8), more than %g" % (
        cid, what, err, r, e_ref, LC.FACTOR)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d entries differ, first at %s" % (what, len(bad), bad[0].tolist()))


def _rows_independent(clean, dirty, rows, what):
    """Rows `rows` (axis 1) of `dirty` are all NaN; every other row is bit-equal to `clean`."""
    B = clean.shape[1]
    keep = np.setdiff1d(np.arange(B), rows)
    assert np.all(np.isnan(dirty[:, rows])), "%s: a poisoned row came out with numbers in it" % what
    _same_bits(dirty[:, keep], clean[:, keep], what + " (rows beside the poisoned ones)")


def _case(cid, name, din, h, tok, L, fb, hot):
    cu = _cu()
    B = LC.resolve_B(tok, cu)
    seed = [c[0] for c in LC.matrix()].index(cid) + 1

    def build():
        x, W, b, dhs = LC.inputs(L, B, din, h, seed, hot)
        ref, e_ref, cs32, g32 = LC.reference(x, W, b, dhs, fb)
        return x, W, b, dhs, ref, e_ref, cs32, g32
    return (cu, B) + (_once(cid, build) if name == 'wreg' and L == 3 and not hot else build())


@pytest.mark.parametrize("cid,name,din,h,tok,L,fb,hot", LC.matrix(), ids=[c[0] for c in LC.matrix()])
def test_lstm_case(dev, cid, name, din, h, tok, L, fb, hot):
    import torch
    cu, B, x, W, b, dhs, ref, e_ref, cs32, g32 = _case(cid, name, din, h, tok, L, fb, hot)
    assert LP.on_path(cu, name, B, din, h), (name, cu, B, din, h, LP.fwd_path(cu, B, din, h),
                                             LP.bwd_path(cu, B, din, h))
    for k, e in e_ref.items():
        assert np.isfinite(e) and e > 0.0, (k, e)
    print("\n%s: B %d, forward %s, backward %s" % (cid, B, LP.fwd_path(cu, B, din, h), LP.bwd_path(cu, B, din, h)))
    tW, tb = _t(dev, W), _t(dev, b)
    # ---- forward: canaries, tolerance, determinism, row independence
    hs, cs, gates = _fwd(dev, x, tW, tb, fb, h)
    out = {'hs': _live(hs, L, B, 'hs'), 'cs': _live(cs, L, B, 'cs'), 'gates': _live(gates, L, B, 'gates')}
    for k in ('gates', 'cs', 'hs'):
        _within(cid, name, k, out[k], ref[k], e_ref[k])
    again = _fwd(dev, x, tW, tb, fb, h)
    for k, t2 in zip(('hs', 'cs', 'gates'), again):
        _same_bits(_live(t2, L, B, k), out[k], k + ": second forward run")
    rows = LC.poison_rows(B)
    if rows:
        xp = x.copy()
        xp[:, rows] = np.nan
        for k, t2 in zip(('hs', 'cs', 'gates'), _fwd(dev, xp, tW, tb, fb, h)):
            _rows_independent(out[k], _live(t2, L, B, k + " (poisoned x)"), rows, k)
    # ---- backward, fed the kernel's own forward
    n = L * B
    wxt = torch.full((4 * h, din), SENT, dtype=torch.float32, device=dev)
    dz = _bwd(dev, tW, cs[:n], gates[:n], dhs, din, wxt)
    dz_a = _live(dz, L, B, 'dz')
    _within(cid, name, 'dz', dz_a, ref['dz'], e_ref['dz'])
    assert np.array_equal(wxt.cpu().numpy(), W[:din].T), "wxt is not W[:din].T"
    _same_bits(_live(_bwd(dev, tW, cs[:n], gates[:n], dhs, din, None), L, B, 'dz'), dz_a, "dz: second backward run")
    if rows:
        dp = dhs.copy()
        dp[:, rows] = np.nan
        _rows_independent(dz_a, _live(_bwd(dev, tW, cs[:n], gates[:n], dp, din, None), L, B, 'dz (poisoned dhs)'),
                          rows, 'dz')
    # ---- backward, fed the oracle's f32-rounded cells and gates; no wxt
    dz_f = _live(_bwd(dev, tW, _t(dev, cs32.reshape(n, h)), _t(dev, g32.reshape(n, 4 * h)), dhs, din, None),
                 L, B, 'dz (oracle-fed)')
    _within(cid, name, 'dz_fed', dz_f, ref['dz_fed'], e_ref['dz_fed'])


@pytest.mark.parametrize("tok,L", [('w', 3), ('w+24', 3)])
def test_wreg_slice_matches_r4(dev, tok, L):
    """64 rows of the big wreg batch, rerun alone on r4, against the rows of the big call (not bit-equal: see above)."""
    cid = [c[0] for c in LC.matrix() if c[1] == 'wreg' and c[4] == tok and c[5] == L and not c[7]][0]
    c = [c for c in LC.matrix() if c[0] == cid][0]
    cu, B, x, W, b, dhs, ref, e_ref, _, _ = _case(*c)
    fb, h, din, n = c[6], 64, 64, L * B
    lo = B - 64 - 8 if tok == 'w' else 40            # rows that straddle 16-row tiles of the big call
    sl = slice(lo, lo + 64)
    assert LP.on_path(cu, 'wreg', B, din, h) and LP.on_path(cu, 'r4', 64, din, h)
    tW, tb = _t(dev, W), _t(dev, b)
    hs, cs, gates = _fwd(dev, x, tW, tb, fb, h)
    dz = _bwd(dev, tW, cs[:n], gates[:n], dhs, din, None)
    xs, ds = np.ascontiguousarray(x[:, sl]), np.ascontiguousarray(dhs[:, sl])
    hs2, cs2, gates2 = _fwd(dev, xs, tW, tb, fb, h)
    dz2 = _bwd(dev, tW, cs2[:L * 64], gates2[:L * 64], ds, din, None)
    print()
    for k, big, small in (('hs', hs, hs2), ('cs', cs, cs2), ('gates', gates, gates2), ('dz', dz, dz2)):
        big_rows = _live(big, L, B, k)[:, sl]
        small_rows = _live(small, L, 64, k)
        r = ref[k][:, sl]
        _within(cid + '/r4-slice', 'r4', k, small_rows, r, e_ref[k])
        diff = np.abs(big_rows.astype(np.float64) - small_rows)
        worst = float(np.max(diff / (e_ref[k] + LC.REL * np.abs(r) / LC.FACTOR)))
        print("  %-8s wreg - r4: %.3e, %.2f x" % (k, float(diff.max()), worst))
        assert worst <= LC.FACTOR, (k, worst)


_EMPTY = [('r4', 64, 64, 5), ('wreg', 64, 64, 'w'), ('mfma1', 32, 64, 17), ('mfma2', 128, 128, 17),
          ('genfwd', 18, 64, 17), ('generic', 20, 24, 5)]


@pytest.mark.parametrize("name,din,h,tok", _EMPTY, ids=[e[0] for e in _EMPTY])
def test_wxt_empty_calls(dev, name, din, h, tok):
    """L == 0 and B == 0: OK, nothing written but wxt, which a launch of its own fills on every path."""
    import torch
    from arx import ops
    cu = _cu()
    B = LC.resolve_B(tok, cu)
    assert LP.on_path(cu, name, B, din, h)
    W = LC.inputs(1, 1, din, h, 3)[1]
    tW, tb = _t(dev, W), _t(dev, np.zeros(4 * h, np.float32))
    some = torch.zeros((SPARE, max(din, 4 * h)), dtype=torch.float32, device=dev)    # never read: L * B == 0
    for L_, B_ in ((0, B), (3, 0)):
        hs, cs, gates, dz = _buf(dev, 0, h), _buf(dev, 0, h), _buf(dev, 0, 4 * h), _buf(dev, 0, 4 * h)
        ops.lstm_fwd(some, tW, tb, L_, B_, din, h, 1.0, hs, cs, gates)
        for wxt in (None, torch.full((4 * h, din), SENT, dtype=torch.float32, device=dev)):
            ops.lstm_bwd(tW, some, some, some, some, L_, B_, din, h, dz, wxt=wxt)
        assert np.array_equal(wxt.cpu().numpy(), W[:din].T), (L_, B_)
        for k, t in (('hs', hs), ('cs', cs), ('gates', gates), ('dz', dz)):
            _live(t, 0, 0, "%s at L %d, B %d" % (k, L_, B_))


# ---------------------------------------------------------------------------------------------------------
# the gate functions alone
# ---------------------------------------------------------------------------------------------------------
GATE_BOUND = 1e-6
SERIES_BOUND = 2e-7             # tanhf_ below 1/16: ax * (1 + x2 * p) -- the series is exact to 1e-10, 1 + t rounds by at
#                                 most 3e-8 (half an ulp below 1), the product by 6e-8: 9e-8, held with a factor of 2
SEAM = 0.0625
_GATE_PATHS = [('r4', 64), ('mfma2', 128), ('generic', 32)]


def _gate_run(dev, path, h, g, bias=None):
    cu = _cu()
    x, W, b, vals, rows = LC.onehot_case(h, g, bias)
    B = x.shape[1]
    assert LP.fwd_path(cu, B, h, h) == path, (path, LP.fwd_path(cu, B, h, h))
    hs, cs, gates = _fwd(dev, x, _t(dev, W), _t(dev, b), 0.0, h)
    return (_live(hs, 1, B, 'hs')[0], _live(cs, 1, B, 'cs')[0], _live(gates, 1, B, 'gates')[0], vals, rows)


def _rel_ok(key, got, exact, xs, series=False):
    """|got - exact| <= GATE_BOUND * |exact|, or <= 2^-126 where the exact result is subnormal in f32; series=True
    (tanh): SERIES_BOUND below the 1/16 seam."""
    err = np.abs(got.astype(np.float64) - exact)
    normal = np.abs(exact) >= LC.FLT_MIN
    rel = np.where(normal, err / np.where(normal, np.abs(exact), 1.0), 0.0)
    if series:
        low = rel[np.abs(xs) < SEAM]
        print("  %s: largest relative error below the seam %.3e" % (key, low.max()))
        assert low.max() <= SERIES_BOUND, (key, float(low.max()))
    i = int(np.argmax(rel))
    print("  %s: largest relative error %.3e at x = %r" % (key, rel[i], float(xs[i])))
    if rel[i] > _GATE_WORST.get(key, (0.0, None))[0]:
        _GATE_WORST[key] = (float(rel[i]), float(xs[i]))
    assert rel[i] <= GATE_BOUND, (key, float(rel[i]), float(xs[i]))
    assert np.all(err[~normal] <= LC.FLT_MIN), (key, xs[~normal][err[~normal] > LC.FLT_MIN])
    sat = np.isin(exact.astype(np.float32), (0.0, 1.0, -1.0)) & (np.abs(xs) >= 8.0)
    assert np.array_equal(got[sat], exact.astype(np.float32)[sat]), (key, "not exact at saturation", xs[sat])


def _steps_ok(key, got, exact, xs):
    """Ascending xs: the output never steps down across the linspace grid, and no step differs from the true step by
    more than the bound (a jump at the 1/16 seam would)."""
    o = np.argsort(xs, kind='stable')
    g, e = got[o].astype(np.float64), exact[o]
    off = np.abs(np.diff(g) - np.diff(e))
    assert np.all(off <= GATE_BOUND * np.abs(e[1:])), (key, float(off.max()))
    coarse = o[np.concatenate([[True], np.diff(xs[o]) > 1e-5])]          # the grid without the seam's float neighbours
    assert np.all(np.diff(got[coarse]) > 0), (key, "not monotone")


@pytest.mark.parametrize("path,h", _GATE_PATHS, ids=[p[0] for p in _GATE_PATHS])
@pytest.mark.parametrize("g", [0, 1], ids=['sigmoid', 'tanh'])
def test_gate_functions(dev, path, h, g):
    _, _, gates, vals, rows = _gate_run(dev, path, h, g)
    n, nband = len(vals), LC.gate_sweep()[1]
    got = gates[:, g * h:(g + 1) * h].reshape(-1)[:n]
    v64 = vals.astype(np.float64)
    exact = np.tanh(v64) if g == 1 else 1.0 / (1.0 + np.exp(-v64))
    key = (path, 'tanh' if g == 1 else 'sigmoid')
    print()
    _rel_ok(key, got, exact, vals, series=g == 1)
    half = n // 2
    for s in (slice(0, nband), slice(half, half + nband)):              # the band and its mirror image
        _steps_ok(key, got[s], exact[s], vals[s])
    col = gates[:, g * h]
    if g == 1:
        nz = vals[:half] != 0
        _same_bits(got[half:][nz], -got[:half][nz], "tanh(-x) against -tanh(x)")
        assert np.all(_bits(gates[rows['pz'], h:2 * h]) == 0), "tanh(+0) is not +0"
        if path != 'r4':        # (r4 sums a pre-activation in four chains, three of them starting from +0: no input
            #                     makes it -0 there)
            assert np.all(_bits(gates[rows['nz'], h:2 * h]) == 0x80000000), "tanh(-0) is not -0"
        assert col[rows['pinf']] == 1.0 and col[rows['ninf']] == -1.0
    else:
        assert col[rows['pinf']] == 1.0 and col[rows['ninf']] == 0.0
    assert np.isnan(col[rows['nan']]), "NaN in, %r out" % float(col[rows['nan']])


@pytest.mark.parametrize("path,h", _GATE_PATHS, ids=[p[0] for p in _GATE_PATHS])
def test_cell_tanh(dev, path, h):
    """c's own tanhf_: gi, gf, go saturated to exactly 1 by a bias of 40, L = 1, so c = gj = tanhf_(sweep) and
    hs = tanhf_(c), with c as the kernel stored it; the band puts c on both sides of the 1/16 seam."""
    hs, cs, gates, vals, rows = _gate_run(dev, path, h, 1, bias=(40.0, -0.0, 40.0, 40.0))
    n, nband, fin = len(vals), LC.gate_sweep()[1], rows['pinf']
    assert np.all(gates[:fin, :h] == 1.0) and np.all(gates[:fin, 3 * h:] == 1.0)
    c = cs.reshape(-1)[:n]
    assert np.array_equal(c, gates[:, h:2 * h].reshape(-1)[:n]), "c is not gj"      # (1 * 0 + 1 * -0 is +0: values, not bits)
    assert c[:nband].min() < 0.0625 < c[:nband].max()
    got = hs.reshape(-1)[:n]
    print()
    _rel_ok((path, 'tanh(c)'), got, np.tanh(c.astype(np.float64)), c, series=True)
    _steps_ok((path, 'tanh(c)'), got[:nband], np.tanh(c[:nband].astype(np.float64)), c[:nband])


# ---------------------------------------------------------------------------------------------------------
# dynamic LDS: 64 KB, just past it, past 160 KB
# ---------------------------------------------------------------------------------------------------------
GEN_H = 2731                    # 6 * 2731 * 4 = 65544 bytes: the first h at which both generic kernels pass 64 KB
_LDS = [('mfma2', 380, 128, 17, 2), ('mfma2', 384, 128, 17, 2), ('generic', 4, GEN_H, 2, 2)]


@pytest.mark.parametrize("path,din,h,B,L", _LDS, ids=["%s-d%d-h%d" % c[:3] for c in _LDS])
def test_lds_boundary(dev, path, din, h, B, L):
    cu = _cu()
    assert LP.fwd_path(cu, B, din, h) == path and LP.bwd_path(cu, B, din, h) == path
    lds_f, lds_b = LP.fwd_lds_bytes(din, h, path), LP.bwd_lds_bytes(h, path)
    if (din, h) == (380, 128):
        assert lds_f == LP.LDS_DEFAULT
    elif path == 'mfma2':
        assert LP.LDS_DEFAULT < lds_f <= LP.LDS_LIMIT
    else:
        assert LP.LDS_DEFAULT < lds_b < lds_f <= LP.LDS_LIMIT and LP.bwd_lds_bytes(h - 1, path) <= LP.LDS_DEFAULT
    cid = "lds-%s-d%d-h%d" % (path, din, h)
    x, W, b, dhs = LC.inputs(L, B, din, h, 7)
    ref, e_ref, _, _ = LC.reference(x, W, b, dhs, 1.0)
    tW, tb = _t(dev, W), _t(dev, b)
    hs, cs, gates = _fwd(dev, x, tW, tb, 1.0, h)
    print()
    for k, t in (('gates', gates), ('cs', cs), ('hs', hs)):
        _within(cid, 'lds-' + path, k, _live(t, L, B, k), ref[k], e_ref[k])
    n = L * B
    _within(cid, 'lds-' + path, 'dz', _live(_bwd(dev, tW, cs[:n], gates[:n], dhs, din, None), L, B, 'dz'), ref['dz'],
            e_ref['dz'])


def test_lds_limit_raises(dev):
    """Past 160 KB of LDS: the library's argument error, ahead of any launch (outputs and wxt keep their sentinels).
    Every buffer has its full size, so a check that went missing would fail a launch, not read out of range."""
    import torch
    from arx import ops
    from arx._lib import ArxError
    cu = _cu()
    for path, din, h in (('mfma2', 1152, 128), ('generic', 4, 6827)):
        assert LP.fwd_path(cu, 1, din, h) == path and LP.fwd_lds_bytes(din, h, path) > LP.LDS_LIMIT
        W = torch.zeros((din + h, 4 * h), dtype=torch.float32, device=dev)
        z = torch.zeros((1, max(din, 4 * h)), dtype=torch.float32, device=dev)
        hs, cs, gates, dz = _buf(dev, 1, h), _buf(dev, 1, h), _buf(dev, 1, 4 * h), _buf(dev, 1, 4 * h)
        with pytest.raises(ArxError, match="arx_lstm_fwd: sizes exceed LDS"):
            ops.lstm_fwd(z, W, z, 1, 1, din, h, 1.0, hs, cs, gates)
        if path == 'generic':
            assert LP.bwd_path(cu, 1, din, h) == path and LP.bwd_lds_bytes(h, path) > LP.LDS_LIMIT
            wxt = torch.full((4 * h, din), SENT, dtype=torch.float32, device=dev)
            with pytest.raises(ArxError, match="arx_lstm_bwd: sizes exceed LDS"):
                ops.lstm_bwd(W, z, z, z, z, 1, 1, din, h, dz, wxt=wxt)
            assert bool((wxt == SENT).all())
        for k, t in (('hs', hs), ('cs', cs), ('gates', gates), ('dz', dz)):
            _live(t, 1, 1, k, written=False)


def test_zz_report():
    """Prints what the docstring records: the largest ratio per path and array, the gate functions' largest error."""
    print()
    for path in sorted(_WORST):
        print("  %-14s %s" % (path, "  ".join("%s %.2f" % (k, v[0]) for k, v in sorted(_WORST[path].items()))))
    for key in sorted(_GATE_WORST):
        print("  %-24s %.3e at x = %r" % (" ".join(key), _GATE_WORST[key][0], _GATE_WORST[key][1]))
    print("  module wall time so far: %.1f s" % (time.time() - _T0))
