"""Direct parity tests for the fused epilogues of the scorer GEMM (csrc/gemm_nt.hip k_gemm_nt_areg<KT, MODE>): the
candidate filter (with per-range log-sum-exp, with exclusion lists), the evaluation sums, the rank counts -- and for
what stands on them: arx_topk_mark_empty, TopKScan.run on plain tensors, the fused / chunked 'ce' evaluation, and the
target-fused 'mw' / 'mce' loss (arx_loss_{mw,mce}_fused_pos).

The oracle has two steps.  (1) L_dev = ops.gemm(A, Bm^T) + bias against float64 under the scale-relative GEMM bound
|err| <= 2e-6 * sum|a||b| + 1e-5.  (2) Every fused output against what numpy (tests/gemm_nt_oracle.py, itself checked
against brute force in test_gemm_nt_oracle_cpu.py) derives from L_dev: arx.h states that the filter's values are
bit-identical to arx_gemm_f32's, so survivor sets, their order, positions and values compare EXACTLY on random floats,
and again on dyadic tables (entries n/2, biases n/4: every score exact in fp32 in any summation order, with many
exact ties with the thresholds).  Per-range outputs are compared per range (arx.h: the range rule), never summed;
every output buffer is wider and taller than what the kernel may write and is compared whole, pre-fill included.

Tolerances: log-sum-exp RTOL 1e-4 / ATOL 1e-5 (what test_row_logsumexp grants the unfused kernel; the epilogue uses
__expf / __logf); margin sums exact on dyadic data, on random floats rtol 1e-5 on the sum over the ranges (the
rank-parts test's tolerance) and per range rtol 1e-5 plus ncols * 2^-22 * (max|L| + |t| + 1): every term is formed
with at most three fp32 roundings at that magnitude, and a range whose few active terms are tiny has no relative
accuracy to speak of.  Shapes come from ops.device_info() at run time so that the split edges (one tile per range,
an even and an odd >= 3 number of tiles, a shorter last range, one range, several row panels) all occur: asserted."""
import numpy as np
import pytest

import gemm_nt_oracle as O
from test_kernels_direct_gpu import (ATOL, RTOL, _canary_ok, _csr_keep, _grid, _oracle, _pos_csr, _scale_bound, _t,
                                     _wide)
from test_sharded_eval_gpu import _check_rank_parts, _dyadic

pytestmark = pytest.mark.gpu

KS = [32, 64, 128]
NEG = -np.inf


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        r, c = bad[0]
        raise AssertionError("%s: %d entries differ, first at [%d, %d]: got %r, want %r"
                             % (what, len(bad), r, c, got[r, c], want[r, c]))


# ---------------------------------------------------------------------------------------------------------
# the problem: operands as strided views, the device's own logits verified against float64
# ---------------------------------------------------------------------------------------------------------
class _Prob(object):
    pass


def _strided(dev, x, pad, fill=1000.0, extra_rows=2):
    """x [n, K] as the left columns of a [n + extra_rows, K + pad] tensor full of `fill`."""
    import torch
    n, K = x.shape
    base = torch.full((n + extra_rows, K + pad), fill, dtype=torch.float32, device=dev)
    view = base[:n, :K]
    view.copy_(_t(dev, x))
    return view


def _problem(dev, A, Bm, bias, col_base=0):
    """L (numpy float32) = the device's A . Bm^T + bias, checked against float64; -inf biases give exactly -inf."""
    import torch
    from arx import ops
    p = _Prob()
    p.M, p.K = A.shape
    p.N = Bm.shape[0]
    p.col_base = col_base
    p.At, p.Bt = _strided(dev, A, 4), _strided(dev, Bm, 8)
    p.bt = None if bias is None else _t(dev, bias)
    assert p.At.stride(0) == p.K + 4 and p.Bt.stride(0) == p.K + 8
    L = torch.empty((p.M, p.N), dtype=torch.float32, device=dev)
    ops.gemm(p.At, p.Bt, L, ops.Workspace(dev), transB=True, col_bias=p.bt)
    p.Lt = L
    p.L = L.cpu().numpy()
    b64 = np.zeros(p.N) if bias is None else bias.astype(np.float64)
    ref = A.astype(np.float64) @ Bm.astype(np.float64).T + b64
    off = np.isneginf(b64)
    assert np.array_equal(np.isneginf(p.L), np.broadcast_to(off, p.L.shape))
    scale = np.abs(A).astype(np.float64) @ np.abs(Bm).astype(np.float64).T + np.where(off, 0.0, np.abs(b64))
    _scale_bound(np.abs(np.where(off, 0.0, p.L - np.where(off, 0.0, ref))), scale)
    p.parts = ops.gemm_nt_topk_parts(p.M, p.N)
    assert p.parts == O.parts_for(ops.device_info()["cu_count"], p.M, p.N)
    p.tpb, p.ranges = O.split_ranges(p.N, p.parts)
    return p


def _tables(rng, M, N, K, dyadic, bias=True, scale=0.3):
    if dyadic:
        A, Bm = _dyadic(rng, M, K), _dyadic(rng, N, K)
        b = _dyadic(rng, N, lo=-4, hi=5, den=4.0) if bias else None
    else:
        A = (rng.standard_normal((M, K)) * scale).astype(np.float32)
        Bm = (rng.standard_normal((N, K)) * scale).astype(np.float32)
        b = (rng.standard_normal(N) * 0.1).astype(np.float32) if bias else None
    return A, Bm, b


# ---------------------------------------------------------------------------------------------------------
# runners: every output lives in a taller, wider, pre-filled buffer that is read back whole
# ---------------------------------------------------------------------------------------------------------
XROWS, XCOLS = 3, 5
LSE_FILL, RELU_FILL, CNT_FILL = 7.0, 9.0, 7


def _dev_ex(dev, ex):
    if ex is None:
        return None
    keys, key_rows, ptr, cols = ex
    assert len(cols) > 0
    i32 = np.int32
    return _t(dev, keys.astype(i32)), int(key_rows), _t(dev, ptr.astype(i32)), _t(dev, cols.astype(i32))


def _run_filter(dev, p, thr, capp, ex=None, lse=False, k=3):
    """-> cand_v, cand_i (whole buffers), the overflow flag with its two neighbours, lse buffer (whole) or None.
    thr travels as column k - 1 of a [M, k] tensor (ldthr = k), the way TopKScan passes it."""
    import torch
    from arx import ops
    M = p.M
    ld = p.parts * capp + XCOLS
    cv = torch.full((M + XROWS, ld), NEG, dtype=torch.float32, device=dev)
    ci = torch.full((M + XROWS, ld), O.IDX_FILL, dtype=torch.int32, device=dev)
    th = torch.full((M, k), 3e38, dtype=torch.float32, device=dev)
    th[:, k - 1] = _t(dev, np.asarray(thr, dtype=np.float32))
    ov = torch.tensor([5, 0, 5], dtype=torch.int32, device=dev)
    lp = torch.full((M + XROWS, p.parts + 2), LSE_FILL, dtype=torch.float32, device=dev) if lse else None
    lpv = lp[:M] if lse else None
    if ex is None:
        ops.gemm_nt_topk_filter(p.At, p.Bt, p.bt, th[:, k - 1], p.col_base, cv[:M], ci[:M], capp, ov[1:2], lse_part=lpv)
    else:
        ops.gemm_nt_topk_filter_excl(p.At, p.Bt, p.bt, th[:, k - 1], p.col_base, cv[:M], ci[:M], capp, ov[1:2],
                                     _dev_ex(dev, ex), lse_part=lpv)
    torch.cuda.synchronize()
    return cv.cpu().numpy(), ci.cpu().numpy(), ov.cpu().numpy().tolist(), (lp.cpu().numpy() if lse else None)


def _check_filter(p, got, thr, capp, excluded=None, what=""):
    """Whole candidate buffers against the oracle; overflow is 1 exactly when a segment was cut, else still 0."""
    cv, ci, ov, _ = got
    ld = p.parts * capp + XCOLS
    ev, ei, over = O.expected_segments(p.L, thr, p.ranges, capp, ld, p.col_base, excluded)
    ev = np.concatenate([ev, np.full((XROWS, ld), NEG, dtype=np.float32)])
    ei = np.concatenate([ei, np.full((XROWS, ld), O.IDX_FILL, dtype=np.int32)])
    _same_bits(cv, ev, what + " cand_v")
    _same_bits(ci, ei, what + " cand_i")
    assert ov == [5, int(over), 5], (what, ov, over)
    return over


def _lse_ranges(p):
    return np.stack([O.lse64(p.L[:, lo:hi]) for lo, hi in p.ranges], axis=1)


def _check_lse(p, lp, what=""):
    """lse_part [M, parts] per range against float64; the columns and rows around it untouched."""
    ref = _lse_ranges(p)
    got = lp[:p.M, :p.parts]
    assert (lp[:p.M, p.parts:] == LSE_FILL).all() and (lp[p.M:] == LSE_FILL).all(), what
    off = np.isneginf(ref)
    assert np.array_equal(np.isneginf(got), off), (what, np.argwhere(np.isneginf(got) != off)[:4].tolist(),
                                                   got[np.isneginf(got) != off][:4])
    assert not np.isnan(got).any(), (what, np.argwhere(np.isnan(got))[:4].tolist())
    np.testing.assert_allclose(got[~off], ref[~off], rtol=RTOL, atol=ATOL, err_msg=what)


def _run_eval(dev, p, t, want_lse, want_relu):
    import torch
    from arx import ops
    M = p.M
    lp = torch.full((M + XROWS, p.parts + 2), LSE_FILL, dtype=torch.float32, device=dev) if want_lse else None
    rp = torch.full((M + XROWS, p.parts + 2), RELU_FILL, dtype=torch.float32, device=dev) if want_relu else None
    ops.gemm_nt_eval_parts(p.At, p.Bt, p.bt, _t(dev, t) if want_relu else None, lp[:M] if want_lse else None,
                           rp[:M] if want_relu else None)
    torch.cuda.synchronize()
    return (lp.cpu().numpy() if want_lse else None), (rp.cpu().numpy() if want_relu else None)


def _check_relu(p, rp, t, dyadic, what=""):
    M = p.M
    assert (rp[:M, p.parts:] == RELU_FILL).all() and (rp[M:] == RELU_FILL).all(), what
    got = rp[:M, :p.parts]
    L64, t64 = p.L.astype(np.float64), t.astype(np.float64)[:, None]
    ref = np.stack([np.maximum(L64[:, lo:hi] - t64 + 1.0, 0.0).sum(1) for lo, hi in p.ranges], axis=1)
    if dyadic:
        _same_bits(got, ref.astype(np.float32), what + " relu_part (dyadic: exact)")
        return
    np.testing.assert_allclose(got.astype(np.float64).sum(1), ref.sum(1), rtol=1e-5, err_msg=what)
    fin = np.where(np.isfinite(p.L), np.abs(p.L), 0.0)
    mag = fin.max(1, keepdims=True).astype(np.float64) + np.abs(t64) + 1.0
    ncols = np.array([hi - lo for lo, hi in p.ranges], dtype=np.float64)[None, :]
    tol = 1e-5 * ref + ncols * 2.0 ** -22 * mag
    err = np.abs(got - ref)
    assert (err <= tol).all(), (what, float((err / tol).max()), np.argwhere(err > tol)[:4].tolist())


# ---------------------------------------------------------------------------------------------------------
# thresholds and exclusion lists that hit the edges
# ---------------------------------------------------------------------------------------------------------
def _thr_mix(L, shift):
    """One kind of threshold per row, eight kinds in every wave: the 10th best of a first chunk (few survivors, the
    production regime); the row maximum (ties lose: nothing survives); +inf; -inf (every column but a -inf logit
    survives: whole tiles of survivors); NaN (nothing survives); a low quantile (long lists); the largest value below
    the maximum (the maxima alone survive: lone survivors in their tiles); the median.  All but the infinities and
    NaN are existing logits of the row."""
    M, N = L.shape
    srt = np.sort(np.where(np.isneginf(L), np.float32(-3e38), L), axis=1)
    thr = np.empty(M, dtype=np.float32)
    for r in range(M):
        kind = (r + shift) % 8
        row = srt[r]
        if kind == 0:
            first = np.sort(L[r, :min(N, 1536)])
            thr[r] = first[max(0, len(first) - 10)]
        elif kind == 1:
            thr[r] = row[-1]
        elif kind == 2:
            thr[r] = np.inf
        elif kind == 3:
            thr[r] = -np.inf
        elif kind == 4:
            thr[r] = np.nan
        elif kind == 5:
            thr[r] = row[N // 4]
        elif kind == 6:
            below = row[row < row[-1]]
            thr[r] = below[-1] if len(below) else row[-1]
        else:
            thr[r] = row[N // 2]
    return thr


def _ex_lists(rng, p, thr):
    """Exclusion lists (row_keys, key_rows, ex_ptr, ex_cols) over absolute columns col_base + c.  key_rows < M where M
    allows (rows r and r + key_rows share a list); some keys < 0; per key, in turn: an empty list; the first and the
    last column of every range and of the ragged last tile, with columns below col_base and at / beyond col_base + N
    around them; the row's best column and a few more; every survivor of the row (nothing is left); several thousand
    columns (the in-loop binary search); only columns outside the launch."""
    M, N, base = p.M, p.N, p.col_base
    key_rows = M if M < 4 else M // 2 + 1
    outside = [base + N, base + N + 5] + ([0, base - 1] if base > 0 else [])
    lists = []
    for j in range(key_rows):
        kind = j % 6
        if kind == 0:
            c = []
        elif kind == 1:
            c = [x for lo, hi in p.ranges for x in (base + lo, base + hi - 1)]
            c += [base + (N - 1) // 64 * 64, base + N - 1] + outside
        elif kind == 2:
            c = [base + int(np.argmax(p.L[j]))] + (base + rng.integers(0, N, size=6)).tolist()
        elif kind == 3:
            with np.errstate(invalid='ignore'):
                c = (base + np.nonzero(p.L[j] > thr[j])[0]).tolist()
        elif kind == 4:
            c = (base + rng.choice(N, size=max(1, min(N * 3 // 5, 6000)), replace=False)).tolist()
        else:
            c = list(outside)
        lists.append(np.unique(np.asarray(c, dtype=np.int64)).astype(np.int32))
    lists.append(np.asarray(sorted(outside), dtype=np.int32))          # (never empty: ex_cols must be a pointer)
    keys = np.arange(key_rows, dtype=np.int32)
    keys[4::7] = -1
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return keys, key_rows, ptr, np.concatenate(lists).astype(np.int32)


def _ex_irrelevant(p):
    """Keys < 0, an empty list and a list of columns outside the launch: nothing of it may change an output."""
    base, N = p.col_base, p.N
    out = sorted([base + N, base + N + 9] + ([base - 1] if base > 0 else []))
    keys = np.array([-1, 0, 1], dtype=np.int32)
    ptr = np.array([0, 0, len(out)], dtype=np.int32)
    return keys, (3 if p.M >= 3 else 1), ptr, np.asarray(out, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------
# the shapes: M x N x split edges, chosen from the device's CU count
# ---------------------------------------------------------------------------------------------------------
SHAPES = ['m1_n1', 'm33_n5', 'm33_n63', 'm1_n577', 'm128_n640', 'm129_n127', 'm129_even', 'm300_even', 'm300_odd']


def _shape(name, cu):
    """-> (M, N, col_base, bias).  ns0 = the ranges one panel set would get: 'even' puts 2 tiles in a range, 'odd' 3
    (the pair loop's lone last tile), both with a last range of one tile."""
    def ns0(M):
        return -(-2 * cu // -(-M // 128))
    if name == 'm1_n1':
        return 1, 1, 0, True
    if name == 'm33_n5':
        return 33, 5, 17, True
    if name == 'm33_n63':
        return 33, 63, 0, False
    if name == 'm1_n577':
        return 1, 577, 64, True                                     # N % 64 == 1
    if name == 'm128_n640':
        return 128, 640, 0, False                                   # exactly one panel, N % 64 == 0
    if name == 'm129_n127':
        return 129, 127, 1000, True                                 # one row past a panel, N % 64 == 63
    if name == 'm129_even':
        n = ns0(129)
        return 129, 64 * (n + n // 2 + 1) - 1, 0, True              # N % 64 == 63
    if name == 'm300_even':
        n = ns0(300)
        return 300, 64 * (n + n // 2 + 1), 1000, True               # N % 64 == 0, col_base != 0
    if name == 'm300_odd':
        n = ns0(300)
        return 300, 64 * (2 * n + n // 2 + 1) - 63, 0, True         # N % 64 == 1
    raise KeyError(name)


def test_shape_list_covers_the_split_edges(dev):
    """Asserted, not assumed: on THIS device the shapes give one tile per range, an even number, an odd number >= 3,
    a last range shorter than the others, a single range, and ranges shared by more than one row panel; M covers a
    lone row, a ragged wave, one panel, one row past it and three panels; N % 64 covers 0, 1, 63 and N < 64."""
    from arx import ops
    cu = ops.device_info()["cu_count"]
    seen = set()
    for name in SHAPES:
        M, N, _, _ = _shape(name, cu)
        parts = ops.gemm_nt_topk_parts(M, N)
        assert parts == O.parts_for(cu, M, N), name
        tpb, ranges = O.split_ranges(N, parts)
        short = ranges[-1][1] - ranges[-1][0] < tpb * 64
        seen.add('tpb1' if tpb == 1 else 'even' if tpb % 2 == 0 else 'odd3')
        if short and parts > 1:
            seen.add('short_last')
        if short and parts > 1 and tpb > 1 and ranges[-1][1] - ranges[-1][0] <= (tpb - 1) * 64:
            seen.add('last_range_fewer_tiles')
        if parts == 1:
            seen.add('one_range')
        if M > 128 and parts > 1:
            seen.add('panels_share_ranges')
        seen.add('M%d' % M)
        seen.add('mod%d' % (N % 64) if N >= 64 else 'below64')
    for want in ('tpb1', 'even', 'odd3', 'short_last', 'last_range_fewer_tiles', 'one_range', 'panels_share_ranges',
                 'M1', 'M33', 'M128', 'M129', 'M300', 'mod0', 'mod1', 'mod63', 'below64'):
        assert want in seen, (want, sorted(seen))


@pytest.mark.parametrize("dyadic", [True, False])
@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("K", KS)
def test_fused_epilogues_against_device_logits(dev, K, name, dyadic):
    """Every fused mode on one problem.  Filter: whole candidate buffers exact at capp = a full range (overflow stays
    0), at capp 1 or 2 (long lists in the -inf / low-quantile rows only: the first capp in column order kept, flag
    set, neighbours intact) and with lone survivors at capp 1 (flag stays 0).  Exclusion lists: the same oracle with
    the listed columns removed before positions are counted; a list that names nothing relevant changes no bit.
    lse_part: per range against float64, bit-identical across the four kernels that produce it.  Evaluation sums:
    per range, the both-kernel bit-identical to the two single ones."""
    from arx import ops
    cu = ops.device_info()["cu_count"]
    M, N, col_base, bias = _shape(name, cu)
    rng = np.random.default_rng(K + 1000 * SHAPES.index(name) + 7 * dyadic)
    A, Bm, b = _tables(rng, M, N, K, dyadic, bias)
    p = _problem(dev, A, Bm, b, col_base)
    thr = _thr_mix(p.L, K // 32 + SHAPES.index(name))
    full = p.tpb * 64
    ex = _ex_lists(rng, p, thr)
    exm = O.excl_mask(M, N, col_base, ex)

    plain = _run_filter(dev, p, thr, full)
    assert not _check_filter(p, plain, thr, full, what="plain")
    with_lse = _run_filter(dev, p, thr, full, lse=True)
    _check_filter(p, with_lse, thr, full, what="topk|lse")
    _check_lse(p, with_lse[3], "topk|lse")
    nothing = _run_filter(dev, p, thr, full, ex=_ex_irrelevant(p), lse=True)
    for a, c, what in zip(nothing, with_lse, ("cand_v", "cand_i", "overflow", "lse_part")):
        if what == "overflow":
            assert a == c
        else:
            _same_bits(a, c, "irrelevant exclusion lists: " + what)
    excl = _run_filter(dev, p, thr, full, ex=ex, lse=True)
    assert not _check_filter(p, excl, thr, full, exm, what="topk|lse|excl")
    _same_bits(excl[3], with_lse[3], "lse_part stays over ALL columns under exclusion")
    excl_only = _run_filter(dev, p, thr, full, ex=ex)
    _check_filter(p, excl_only, thr, full, exm, what="topk|excl")

    small = 1 if K == 32 else 2
    over = _check_filter(p, _run_filter(dev, p, thr, small), thr, small, what="capp %d" % small)
    _check_filter(p, _run_filter(dev, p, thr, small, ex=ex, lse=True), thr, small, exm, what="capp %d excl" % small)
    if N > 64 * small and M >= 8:
        assert over                                                  # (the -inf rows' lists are longer than capp)

    # lone survivors: even rows keep their maxima only, odd rows nothing; capp 1
    srt = np.sort(p.L, axis=1)
    lone = srt[:, -1].copy()
    for r in range(0, M, 2):
        below = srt[r][srt[r] < srt[r, -1]]
        lone[r] = below[-1] if len(below) else srt[r, -1]
    over = _check_filter(p, _run_filter(dev, p, lone, 1), lone, 1, what="lone survivors")
    if not dyadic:
        assert not over                                              # (random floats: one maximum per row)

    # evaluation sums: targets are logits of the row (ties with t are exact), every fourth an unrelated value
    tcol = rng.integers(0, N, size=M)
    t = p.L[np.arange(M), tcol].copy()
    t[::4] = np.round(rng.standard_normal(len(t[::4])) * 2) / 4
    lse_only, _ = _run_eval(dev, p, t, True, False)
    _, relu_only = _run_eval(dev, p, t, False, True)
    both = _run_eval(dev, p, t, True, True)
    _check_lse(p, lse_only, "lse")
    _check_relu(p, relu_only, t, dyadic, "relu")
    _same_bits(both[0], lse_only, "lse|relu against lse")
    _same_bits(both[1], relu_only, "lse|relu against relu")
    _same_bits(with_lse[3], lse_only, "topk|lse against lse")


# ---------------------------------------------------------------------------------------------------------
# log-sum-exp: value regimes and -inf
# ---------------------------------------------------------------------------------------------------------
def _two_panel_even_N(cu, tail):
    n = -(-2 * cu // 2)
    return 64 * (n + n // 2 + 1) - tail


@pytest.mark.parametrize("K", KS)
def test_lse_part_value_regimes(dev, K):
    """Rows by r % 4: rising along the columns to +80 (the online update rescales on every step), falling from +80
    (it never does), O(1) logits, and one column that dominates the row by 60, in a different range per row.  A sum of
    exp without the running maximum would overflow at 80."""
    from arx import ops
    rng = np.random.default_rng(K)
    M, N = 130, _two_panel_even_N(ops.device_info()["cu_count"], 20)
    A = (rng.standard_normal((M, K)) * 0.05).astype(np.float32)
    Bm = (rng.standard_normal((N, K)) * 0.3).astype(np.float32)
    Bm[:, 0] = np.linspace(-8.0, 8.0, N)
    A[0::4, 0], A[1::4, 0], A[2::4, 0], A[3::4, 0] = 10.0, -10.0, 0.1, 0.0
    parts = ops.gemm_nt_topk_parts(M, N)
    tpb, ranges = O.split_ranges(N, parts)
    assert tpb == 2 and parts > K
    for j in range(K - 1):                                          # row r leads in column dom[r % (K - 1)]
        lo, hi = ranges[(7 * j) % parts]
        Bm[lo + (5 * j) % (hi - lo), 1 + j] = 60.0
    for r in range(3, M, 4):
        A[r, 1 + r % (K - 1)] = 1.0
    p = _problem(dev, A, Bm, (rng.standard_normal(N) * 0.1).astype(np.float32))
    assert np.abs(p.L).max() > 75 and (p.L[3::4].max(1) > 50).all()
    lse_only, _ = _run_eval(dev, p, None, True, False)
    _check_lse(p, lse_only, "lse")
    t = np.zeros(M, dtype=np.float32)
    _same_bits(_run_eval(dev, p, t, True, True)[0], lse_only, "lse|relu")
    thr = np.full(M, np.inf, dtype=np.float32)
    _same_bits(_run_filter(dev, p, thr, 1, lse=True)[3], lse_only, "topk|lse")
    _same_bits(_run_filter(dev, p, thr, 1, ex=_ex_irrelevant(p), lse=True)[3], lse_only, "topk|lse|excl")


def _rank_run(dev, p, t, tcol):
    import torch
    from arx import ops
    rp = torch.full((p.M, p.parts + 3), RELU_FILL, dtype=torch.float32, device=dev)
    cp = torch.full((p.M, p.parts + 3), CNT_FILL, dtype=torch.int32, device=dev)
    ops.gemm_nt_eval_rank_parts(p.At, p.Bt, p.bt, _t(dev, t), _t(dev, tcol.astype(np.int32)), rp, cp)
    rp, cp = rp.cpu().numpy(), cp.cpu().numpy()
    assert (rp[:, p.parts:] == RELU_FILL).all() and (cp[:, p.parts:] == CNT_FILL).all()
    return rp[:, :p.parts], cp[:, :p.parts]


@pytest.mark.parametrize("K", KS)
def test_neg_inf_bias_adds_nothing(dev, K):
    """Items switched off with a -inf bias: the first column of the launch and of a range, a whole tile, a whole
    range, the last column of the ragged tile.  The contract is arx_row_logsumexp's on the materialised logits: a -inf
    logit adds nothing.  lse_part is -inf for the range that holds nothing else and finite elsewhere (the fused
    epilogue used to start from (-inf, 0): a lane whose first column was -inf formed -inf - -inf = NaN and kept it),
    and the row's log-sum-exp over the parts equals the one over the logits.  The margin sums and the rank counts get
    the same columns: they add 0 and count 0.  Dyadic tables: sums and counts exact."""
    import torch
    from arx import ops
    rng = np.random.default_rng(K + 5)
    M, N = 130, _two_panel_even_N(ops.device_info()["cu_count"], 7)
    A, Bm, b = _tables(rng, M, N, K, True)
    parts = ops.gemm_nt_topk_parts(M, N)
    tpb, ranges = O.split_ranges(N, parts)
    assert tpb == 2 and parts > 8
    b[0] = NEG
    b[ranges[3][0]] = NEG
    b[ranges[5][0] + 64:ranges[5][0] + 128] = NEG
    b[ranges[7][0]:ranges[7][1]] = NEG
    b[ranges[9][0] + 31:ranges[9][0] + 34] = NEG                      # both column halves of a first tile
    b[N - 1] = NEG
    p = _problem(dev, A, Bm, b)
    ref = _lse_ranges(p)
    assert np.isneginf(ref[:, 7]).all() and np.isfinite(np.delete(ref, 7, axis=1)).all()
    tcol = rng.integers(0, N, size=M)
    tcol[:6] = [0, ranges[3][0], ranges[5][0] + 70, ranges[7][0] + 3, N - 1, N]    # targets on switched-off items
    t = np.where(tcol < N, p.L[np.arange(M), np.minimum(tcol, N - 1)], 0.25).astype(np.float32)
    t[np.isneginf(t)] = 0.5
    lse_only, _ = _run_eval(dev, p, t, True, False)
    _check_lse(p, lse_only, "lse")
    both = _run_eval(dev, p, t, True, True)
    _same_bits(both[0], lse_only, "lse|relu")
    _check_relu(p, both[1], t, True, "relu with -inf columns")
    thr = _thr_mix(p.L, 0)
    got = _run_filter(dev, p, thr, tpb * 64, lse=True)
    _check_filter(p, got, thr, tpb * 64, what="topk|lse with -inf columns")      # thr = -inf rows: -inf never survives
    _same_bits(got[3], lse_only, "topk|lse")
    ex = _ex_lists(rng, p, thr)
    got = _run_filter(dev, p, thr, tpb * 64, ex=ex, lse=True)
    _check_filter(p, got, thr, tpb * 64, O.excl_mask(M, N, 0, ex), what="topk|lse|excl with -inf columns")
    _same_bits(got[3], lse_only, "topk|lse|excl")
    # the rows' log-sum-exp over the parts: finite, float64's, and arx_row_logsumexp's over the logits themselves
    out_p = torch.empty(M, dtype=torch.float32, device=dev)
    out_l = torch.empty(M, dtype=torch.float32, device=dev)
    ops.row_logsumexp(_t(dev, lse_only[:M, :p.parts]), out_p)
    ops.row_logsumexp(p.Lt, out_l)
    np.testing.assert_allclose(out_p.cpu().numpy(), O.lse64(p.L), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out_p.cpu().numpy(), out_l.cpu().numpy(), rtol=RTOL, atol=ATOL)
    # rank counts: exact on dyadic data; the target column adds (1, 0) even where its item is switched off
    rp, cp = _rank_run(dev, p, t, tcol)
    L64, t64 = p.L.astype(np.float64), t.astype(np.float64)[:, None]
    hit = np.zeros((M, N), dtype=bool)
    on = tcol < N
    hit[np.nonzero(on)[0], tcol[on]] = True
    marg = np.where(hit, 1.0, np.maximum((L64 - t64) + 1.0, 0.0))
    cnt = (L64 > t64) & ~hit
    for q, (lo, hi) in enumerate(p.ranges):
        np.testing.assert_array_equal(cp[:, q], cnt[:, lo:hi].sum(1))
        np.testing.assert_allclose(rp[:, q], marg[:, lo:hi].sum(1), rtol=1e-5, atol=0)
    assert (cp[:, 7] == 0).all() and rp[3, 7] == 1.0              # (row 3's target sits in the switched-off range)

    # every column of a launch switched off: -inf parts, and the chunked twin's NaN-for-NaN over parts and logits
    N2 = 200
    p2 = _problem(dev, A, Bm[:N2].copy(), np.full(N2, NEG, dtype=np.float32))
    lse2, relu2 = _run_eval(dev, p2, t, True, True)
    assert np.isneginf(lse2[:M, :p2.parts]).all() and (relu2[:M, :p2.parts] == 0).all()
    assert (lse2[:M, p2.parts:] == LSE_FILL).all()
    ops.row_logsumexp(_t(dev, lse2[:M, :p2.parts]), out_p)
    ops.row_logsumexp(p2.Lt, out_l)
    np.testing.assert_array_equal(out_p.cpu().numpy(), out_l.cpu().numpy())
    rp2, cp2 = _rank_run(dev, p2, t, np.full(M, -1))
    assert (rp2 == 0).all() and (cp2 == 0).all()


# ---------------------------------------------------------------------------------------------------------
# rank counts at the shape edges (the checker and its assertions are test_sharded_eval_gpu.py's)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dyadic", [True, False])
@pytest.mark.parametrize("name", ['m1_n577', 'm33_n5', 'm129_n127', 'm129_even', 'm300_odd'])
@pytest.mark.parametrize("K", KS)
def test_rank_parts_shape_edges(dev, K, name, dyadic):
    """M 1 / 33 / 129 / 300, N 5 / N % 64 in {1, 63}, even and odd tiles per range; targets in the ragged last tile,
    in the first and the last column of a range, and two rows of one wave with their targets in one tile."""
    from arx import ops
    M, N, _, _ = _shape(name, ops.device_info()["cu_count"])
    tpb, ranges = O.split_ranges(N, ops.gemm_nt_topk_parts(M, N))
    rng = np.random.default_rng(K + 3 * dyadic + len(name))
    tcol = rng.integers(0, N, size=M).astype(np.int32)
    edge = [N - 1, (N - 1) // 64 * 64, ranges[-1][0], ranges[0][1] - 1, ranges[len(ranges) // 2][0],
            ranges[len(ranges) // 2][1] - 1, min(N - 1, 70), min(N - 1, 75)]
    n = min(M, len(edge))
    tcol[:n] = edge[:n]
    if M >= 40:
        tcol[32:36] = [N - 1, N - 2 if N > 1 else 0, -1, N]           # a second wave: two targets in the last tile
    _check_rank_parts(dev, K, dyadic, M, N, tcol, np.random.default_rng(K + 11),
                      np.nonzero((tcol < 0) | (tcol >= N))[0])


# ---------------------------------------------------------------------------------------------------------
# arx_topk_mark_empty
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,k", [(1, 1), (7, 1), (33, 100), (3, 1024), (130, 257)])
def test_topk_mark_empty(dev, B, k):
    """indices = -1 exactly where values == -inf: in the middle and at the tail of a row; +inf, NaN, -FLT_MAX and -0.0
    are values like any other.  values / indices are views into wider canary-filled tensors (ldv != ldi)."""
    import torch
    from arx import ops
    rng = np.random.default_rng(B + k)
    v = rng.standard_normal((B, k)).astype(np.float32)
    special = np.array([np.inf, np.nan, -np.finfo(np.float32).max, -0.0, NEG], dtype=np.float32)
    pick = rng.random((B, k))
    v[pick < 0.4] = special[rng.integers(0, 5, size=int((pick < 0.4).sum()))]
    v[:, -1] = NEG if k > 1 else v[:, -1]
    v[0, 0] = NEG
    if k > 2:
        v[B // 2, k // 2] = NEG
        v[B // 2, k // 2 + 1] = -np.finfo(np.float32).max
    idx = rng.integers(0, 1 << 20, size=(B, k)).astype(np.int32)
    vbase, V = _wide(dev, B, k, 50.0, off=3, pad=5)
    V.copy_(_t(dev, v))
    ibase = torch.full((B, k + 11), -9, dtype=torch.int32, device=dev)
    I = ibase[:, 2:2 + k]
    I.copy_(_t(dev, idx))
    ops.topk_mark_empty(V, I)
    torch.cuda.synchronize()
    want = np.where(np.isneginf(v), -1, idx)
    np.testing.assert_array_equal(I.cpu().numpy(), want)
    assert (want == -1).any() and (want[~np.isneginf(v)] >= 0).all()
    ib = ibase.cpu().numpy()
    assert (ib[:, :2] == -9).all() and (ib[:, 2 + k:] == -9).all()
    assert _canary_ok(vbase, k, 50.0, off=3)
    _same_bits(V.cpu().numpy(), v, "values are read only")


# ---------------------------------------------------------------------------------------------------------
# TopKScan.run on plain tensors
# ---------------------------------------------------------------------------------------------------------
def _scan_tables(rng, B, V, d, dyadic, bias, chunk):
    U, P, b = _tables(rng, B, V, d, dyadic, bias)
    if dyadic:
        # blocks of identical pool rows (and biases) across the chunk boundary and the range boundaries behind it:
        # exact ties whose order only the lower-column rule decides
        for c in [chunk] + [chunk + 64 * j for j in (1, 2, 5)]:
            if c + 3 <= V:
                P[c - 3:c + 3] = P[c - 3]
                if b is not None:
                    b[c - 3:c + 3] = b[c - 3]
    return U, P, b


def _scan_ex(rng, B, V, k, short_rows):
    """Per-row lists (key_rows = B): random thirds of the vocabulary, an empty list, a key < 0; short_rows: row 1 keeps
    fewer than k eligible columns (its result ends in (-inf, -1))."""
    lists = []
    for r in range(B):
        if r % 5 == 4:
            c = np.empty(0, dtype=np.int64)
        else:
            c = rng.choice(V, size=V // 3, replace=False)
        if short_rows and r == 1:
            c = np.setdiff1d(np.arange(V), rng.choice(V, size=max(1, k // 2), replace=False))
        lists.append(np.unique(c).astype(np.int32))
    lists.append(np.array([V + 3], dtype=np.int32))
    keys = np.arange(B, dtype=np.int32)
    keys[3::11] = -1
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return keys, B, ptr, np.concatenate(lists).astype(np.int32)


def _scan(dev, Ut, Pt, bt, B, V, d, k, chunk, want_lse, ex, fused):
    import torch
    from arx import ops
    from arx.hmf.hmf_model import TopKScan
    scan = TopKScan(B, V, d, k, dev, chunk=chunk, want_lse=want_lse)
    assert scan.fused, "the fused scan is the default at d in {32, 64, 128}"
    scan.fused = fused
    vals = torch.full((B, k), 5.0, dtype=torch.float32, device=dev)
    idx = torch.full((B, k), -5, dtype=torch.int32, device=dev)
    scan.run(Ut, Pt, bt, ops.Workspace(dev), vals, idx, _dev_ex(dev, ex))
    torch.cuda.synchronize()
    return scan, vals.cpu().numpy(), idx.cpu().numpy(), (scan.lse.cpu().numpy() if want_lse else None)


def _scan_expected_overflow(p, scan, k, chunk, exm):
    """What the fused run's flag must be, from the oracle: thresholds = the k-th best eligible column of the first
    chunk, the scan's own capp, the ranges of the remaining columns."""
    capp, parts = scan._cand[1], scan._cand[5]
    rest = p.L[:, chunk:]
    tpb, ranges = O.split_ranges(rest.shape[1], parts)
    v0, _ = O.topk_tf(p.L[:, :chunk], k, None if exm is None else exm[:, :chunk])
    _, _, over = O.expected_segments(rest, v0[:, k - 1], ranges, capp, parts * capp, chunk,
                                     None if exm is None else exm[:, chunk:])
    return over


SCAN_CASES = [  # B, d, V, k, bias, want_lse, ex, dyadic
    (1, 32, 3 * 1536 + 77, 1, False, False, False, True),
    (130, 64, 6000, 100, True, True, True, True),
    (300, 128, 5000, 1024, True, True, False, False),
    (130, 32, 4000, 1024, False, False, True, True),
    (1, 128, 3333, 100, True, True, True, False),
    (300, 64, 4700, 1, True, False, False, True),
    (300, 32, 1536 + 64 * 200 + 1, 100, True, True, True, True),      # two tiles per range behind the first chunk
]


@pytest.mark.parametrize("B,d,V,k,bias,want_lse,ex,dyadic", SCAN_CASES)
def test_topk_scan_equals_stable_argsort(dev, B, d, V, k, bias, want_lse, ex, dyadic):
    """TopKScan.run, fused and chunked, index for index against numpy's stable argsort of the negated device logits
    (value descending, lower column first), excluded columns removed, (-inf, -1) tails for short rows; values are the
    device logits bit for bit; lse against float64 over all V.  chunk 1536 with a ragged tail (narrower than k where
    k = 1024).  The fused run must not overflow -- and the oracle says so too."""
    chunk = 1536
    rng = np.random.default_rng(B + d + V + k)
    U, P, b = _scan_tables(rng, B, V, d, dyadic, bias, chunk)
    p = _problem(dev, U, P, b)
    exl = _scan_ex(rng, B, V, k, short_rows=(k >= 100)) if ex else None
    exm = O.excl_mask(B, V, 0, exl) if ex else None
    want_v, want_i = O.topk_tf(p.L, k, exm)
    if ex and k >= 100 and B > 1:
        assert (want_i[1] == -1).any() and (want_i[1] >= 0).any()
    for fused in (True, False):
        scan, vals, idx, lse = _scan(dev, p.At, p.Bt, p.bt, B, V, d, k, chunk, want_lse, exl, fused)
        what = "fused" if fused else "chunked"
        if fused:
            assert not _scan_expected_overflow(p, scan, k, chunk, exm)
            assert not scan.overflowed()
        np.testing.assert_array_equal(idx, want_i, err_msg=what)
        _same_bits(vals, want_v, what + " values")
        if want_lse:
            np.testing.assert_allclose(lse, O.lse64(p.L), rtol=RTOL, atol=ATOL, err_msg=what)


@pytest.mark.parametrize("d", KS)
def test_topk_scan_overflow_then_chunked_rerun(dev, d):
    """Scores rising along the vocabulary: every later column beats the first chunk's k-th best, the candidate
    segments overflow, overflowed() says so, and the chunked rerun (what LatentProductModel.step does then) equals the
    oracle."""
    from arx import ops
    B, k, chunk = 300, 10, 1536
    ns0 = -(-2 * ops.device_info()["cu_count"] // 3)
    V = chunk + 64 * (2 * ns0 + ns0 // 2) + 5                       # three tiles per range: longer than a segment
    rng = np.random.default_rng(d)
    U, P, _ = _tables(rng, B, V, d, True, False)
    b = (np.arange(V) * 0.25).astype(np.float32)
    p = _problem(dev, U, P, b)
    want_v, want_i = O.topk_tf(p.L, k)
    scan, _, _, _ = _scan(dev, p.At, p.Bt, p.bt, B, V, d, k, chunk, False, None, True)
    assert _scan_expected_overflow(p, scan, k, chunk, None)
    assert scan.overflowed()
    _, vals, idx, _ = _scan(dev, p.At, p.Bt, p.bt, B, V, d, k, chunk, False, None, False)
    np.testing.assert_array_equal(idx, want_i)
    _same_bits(vals, want_v, "chunked rerun")


@pytest.mark.parametrize("d", KS)
def test_topk_scan_lse_with_switched_off_items(dev, d):
    """-inf biases on some items (the first column behind the first chunk, the first columns of further ranges, a
    whole tile, a few in the first chunk): the fused scan's lse equals the chunked scan's and float64's, and the
    winners are the oracle's."""
    B, V, k, chunk = 130, 6000, 20, 1536
    rng = np.random.default_rng(d + 1)
    U, P, b = _tables(rng, B, V, d, False, True)
    for c in (5, 700, chunk, chunk + 33, chunk + 64, chunk + 64 * 7, V - 1):
        b[c] = NEG
    b[chunk + 64 * 3:chunk + 64 * 4] = NEG
    p = _problem(dev, U, P, b)
    want_v, want_i = O.topk_tf(p.L, k)
    out = {}
    for fused in (True, False):
        scan, vals, idx, lse = _scan(dev, p.At, p.Bt, p.bt, B, V, d, k, chunk, True, None, fused)
        assert not scan.overflowed()
        np.testing.assert_array_equal(idx, want_i)
        _same_bits(vals, want_v, "values")
        np.testing.assert_allclose(lse, O.lse64(p.L), rtol=RTOL, atol=ATOL, err_msg="fused %s" % fused)
        out[fused] = lse
    np.testing.assert_allclose(out[True], out[False], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("d", KS)
def test_ce_eval_fused_equals_chunked_with_switched_off_items(dev, d):
    """StreamEvalLoss's two 'ce' forms on the ops: ONE pass of arx_gemm_nt_eval_parts + arx_row_logsumexp over the
    parts (ARX_EVAL_FUSED=1) against chunks of logits folded by arx_eval_chunk_accum (=0), a few items switched off
    with a -inf bias -- equal to each other and to float64's logsumexp - t."""
    import torch
    from arx import ops
    B, V, chunk = 48, 5000, 96 * 7
    rng = np.random.default_rng(d + 2)
    U, P, b = _tables(rng, B, V, d, False, True)
    for c in (0, 1, 64, 640, 641, 4999):
        b[c] = NEG
    b[1280:1344] = NEG
    p = _problem(dev, U, P, b)
    t = p.L[np.arange(B), rng.integers(2, 60, size=B)].copy()
    tt = _t(dev, t)
    f32 = dict(dtype=torch.float32, device=dev)
    a0, a1, out_f, out_c = (torch.empty(B, **f32) for _ in range(4))
    parts = torch.empty((B, p.parts), **f32)
    ops.gemm_nt_eval_parts(p.At, p.Bt, p.bt, None, parts, None)
    ops.row_logsumexp(parts, a0)
    ops.fill_f32(a1, 1.0)
    ops.eval_finish(0, a0, a1, tt, out_f)
    buf = torch.empty((B, chunk), **f32)
    ws = ops.Workspace(dev)
    for c0 in range(0, V, chunk):
        c1 = min(V, c0 + chunk)
        lg = buf[:, :c1 - c0]
        ops.gemm(p.At, p.Bt[c0:c1], lg, ws, transB=True, col_bias=p.bt[c0:c1])
        ops.eval_chunk_accum(lg, tt, 0, c0 == 0, a0, a1)
    ops.eval_finish(0, a0, a1, tt, out_c)
    ref = O.lse64(p.L) - t.astype(np.float64)
    np.testing.assert_allclose(out_f.cpu().numpy(), ref, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out_c.cpu().numpy(), ref, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out_f.cpu().numpy(), out_c.cpu().numpy(), rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------
# arx_loss_{mw,mce}_fused_pos
# ---------------------------------------------------------------------------------------------------------
def _fused_pos_inputs(rng, B, S, d, mask_rows):
    """-> users [mask_rows], pos_ptr, pos_items, item2slot: users with 0 / 3 / 17 / 1 / 70 positives, some of them
    without a column, and a last user whose positives are ALL the S sampled columns (s = 0: zero loss and gradients);
    row 0 is that user's where there is more than one row."""
    nu, n_items = mask_rows + 2, S + 40
    ptr, items = _pos_csr(rng, nu, n_items, [0, 3, 17, 1, 70])
    items = items[:ptr[-1]]
    item2slot = np.full(n_items, -1, dtype=np.int32)
    slots = rng.permutation(n_items)[:S].astype(np.int32)
    item2slot[slots] = np.arange(S, dtype=np.int32)
    ptr = np.concatenate([ptr, [ptr[-1] + S]]).astype(np.int32)
    items = np.concatenate([items, slots]).astype(np.int32)
    users = rng.integers(0, nu, size=mask_rows).astype(np.int32)
    if mask_rows > 1:
        users[0] = nu
    return users, ptr, items, item2slot, nu + 1


FUSED_POS_CASES = [  # B, S, d, mask_rows (0: B), row_w, packed
    (1, 4, 4, 0, False, True), (33, 128, 32, 0, True, True), (300, 2048, 64, 0, False, False),
    (33, 2048, 256, 11, True, True), (300, 128, 128, 100, True, False), (33, 4, 256, 0, False, False),
]


@pytest.mark.parametrize("kind", ['mw', 'mce'])
@pytest.mark.parametrize("B,S,d,mask_rows,row_w,packed", FUSED_POS_CASES)
def test_loss_fused_pos(dev, kind, B, S, d, mask_rows, row_w, packed):
    """t = U . T + tbias in float64, then the loss and gradients of the unfused *_fwdbwd_pos entry with that t (the
    oracle's compute_loss / compute_loss_bwd under the mask the positives CSR stands for), dT = dt * U and dU = dt * T
    WRITTEN over a canary.  packed: tbias is the bias column of packed [B, d + 1] rows and dtscore the same column of
    the gradient rows (element r at [r * (d + 1)], as arx.dist passes them); else contiguous.  Dyadic U / T and grid
    logits / biases: t is exact in fp32, so the hinge's active set is the same in fp32 and float64."""
    import torch
    from arx import ops
    rng = np.random.default_rng(B * 7 + S + d + len(kind))
    mr = mask_rows or B
    users, ptr, items, item2slot, _ = _fused_pos_inputs(rng, B, S, d, mr)
    U, T = _dyadic(rng, B, d), _dyadic(rng, B, d)
    tb = _grid(rng, (B,), 1.0)
    logits = _grid(rng, (B, S), 3.0 if kind == 'mce' else 4.0)
    rw = (rng.integers(1, 9, size=B) / 8.0).astype(np.float32) if row_w else None
    gscale = 0.25
    t64 = (U.astype(np.float64) * T.astype(np.float64)).sum(1) + tb.astype(np.float64)
    keep = _csr_keep(users[np.arange(B) % mr], ptr, items, item2slot, B, S)
    assert B == 1 or not keep[0].any()
    e = _oracle()
    bl, cache = e.compute_loss(logits.astype(np.float64), t64, kind, keep)
    w = np.full(B, gscale) * (1.0 if rw is None else rw.astype(np.float64))
    dl, dt = e.compute_loss_bwd(cache, w)

    f32 = dict(dtype=torch.float32, device=dev)
    Ut, Tt = _strided(dev, U, 4), _strided(dev, T, 8)
    if packed:
        pk = torch.full((B, d + 1), 3.0, **f32)
        pk[:, d] = _t(dev, tb)
        tbt = pk[:, d]
        gpk = torch.full((B, d + 1), 11.0, **f32)
        dtt = gpk[:, d]
    else:
        tbt = _t(dev, tb)
        dtt = torch.full((B,), 11.0, **f32)
    out_l, t_out = torch.full((B,), 11.0, **f32), torch.full((B,), 11.0, **f32)
    dbase, D = _wide(dev, B, S, 7.0)
    ubase, dU = _wide(dev, B, d, 7.0, off=4, pad=8)
    tbase, dT = _wide(dev, B, d, 7.0, off=8, pad=12)
    dU.fill_(13.0)
    dT.fill_(13.0)
    ops.loss_mw_fused_pos(_t(dev, logits), Ut, Tt, tbt, _t(dev, users), _t(dev, ptr), _t(dev, items),
                          _t(dev, item2slot), out_l, D, t_out, dtt, dU, dT, gscale,
                          row_w=None if rw is None else _t(dev, rw), mask_rows=mask_rows, kind=kind)
    torch.cuda.synchronize()
    scale = (np.abs(U).astype(np.float64) * np.abs(T)).sum(1) + np.abs(tb)
    _scale_bound(np.abs(t_out.cpu().numpy() - t64), scale)
    np.testing.assert_allclose(out_l.cpu().numpy(), bl, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(D.cpu().numpy(), dl, rtol=RTOL, atol=1e-7)
    np.testing.assert_allclose(dtt.cpu().numpy(), dt, rtol=RTOL, atol=1e-7)
    np.testing.assert_allclose(dT.cpu().numpy(), dt[:, None] * U.astype(np.float64), rtol=RTOL, atol=1e-7)
    np.testing.assert_allclose(dU.cpu().numpy(), dt[:, None] * T.astype(np.float64), rtol=RTOL, atol=1e-7)
    if B > 1:
        assert abs(out_l.cpu().numpy()[0]) <= ATOL
        assert (D.cpu().numpy()[0] == 0).all() and (dU.cpu().numpy()[0] == 0).all()
    assert np.abs(dt).max() > 0 and np.abs(dl).max() > 0
    assert _canary_ok(dbase, S, 7.0) and _canary_ok(ubase, d, 7.0, off=4) and _canary_ok(tbase, d, 7.0, off=8)
    if packed:
        assert (pk.cpu().numpy()[:, :d] == 3.0).all() and (gpk.cpu().numpy()[:, :d] == 11.0).all()


@pytest.mark.parametrize("kind", ['mw', 'mce'])
@pytest.mark.parametrize("S,d", [(128, 6), (128, 260), (2052, 64), (6, 64)])
def test_loss_fused_pos_refusals(dev, kind, S, d):
    """d % 4 != 0, d > 256, S > 2048 and S % 4 != 0 return ARX_EUNSUPPORTED (-4) and leave every output untouched."""
    import torch
    from arx import ops
    from arx._lib import ArxError
    B = 5
    rng = np.random.default_rng(S + d)
    users, ptr, items, item2slot, _ = _fused_pos_inputs(rng, B, S, d, B)
    f32 = dict(dtype=torch.float32, device=dev)
    ld = (d + 3) // 4 * 4                                             # 16-byte rows: the refusal is the shape's
    U, T = torch.ones((B, ld), **f32)[:, :d], torch.ones((B, ld), **f32)[:, :d]
    outs = [torch.full(s, 7.0, **f32) for s in ((B,), (B, S), (B,), (B,), (B, ld), (B, ld))]
    out_l, D, t_out, dtt, dU, dT = outs
    with pytest.raises(ArxError, match=r"arx_loss_%s_fused_pos failed \(-4\)" % kind):
        ops.loss_mw_fused_pos(_t(dev, _grid(rng, (B, S))), U, T, torch.zeros(B, **f32), _t(dev, users), _t(dev, ptr),
                              _t(dev, items), _t(dev, item2slot), out_l, D, t_out, dtt, dU[:, :d], dT[:, :d], 0.5,
                              kind=kind)
    torch.cuda.synchronize()
    for o in outs:
        assert (o.cpu().numpy() == 7.0).all()
