"""Direct tests of the similar_items kernels through the C ABI (csrc/similar.hip and the cosine form of the fused
filter GEMM, csrc/gemm_nt.hip kNtCos / kNtSelf): arx_rows_inv_norm, arx_gather_rows_unit, arx_cos_chunk_finish and
arx_gemm_nt_topk_filter_cos.

Exact data (tests/similar_oracle.py) compares bit for bit; Gaussian data under the float32 running-error bound of a
length-d sum of squares and its 1 / sqrt: |rel err| <= (d / 2 + 2) * 2^-24, granted twice.  The fused filter is compared
with the numpy restatement of tests/gemm_nt_oracle.py (expected_segments, the self column as the one excluded column of
its row) on exact data: values, columns and their order, whole buffers with their pre-fill."""
import numpy as np
import pytest

import gemm_nt_oracle as O
import similar_oracle as S
from test_kernels_direct_gpu import _canary_ok, _t, _wide

pytestmark = pytest.mark.gpu

NEG = -np.inf


def _padded(dev, x, pad, fill=1000.0):
    """x [n, d] as the left columns of a [n + 2, d + pad] tensor full of `fill`."""
    import torch
    n, d = x.shape
    base = torch.full((n + 2, d + pad), fill, dtype=torch.float32, device=dev)
    view = base[:n, :d]
    if n:
        view.copy_(_t(dev, x))
    return view


def _bits_equal(got, want, what=""):
    g = np.ascontiguousarray(got, dtype=np.float32).view(np.int32)
    w = np.ascontiguousarray(want, dtype=np.float32).view(np.int32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d entries differ, first at %s: got %r, want %r"
                             % (what, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---------------------------------------------------------------------------------------------------------
# arx_rows_inv_norm
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 7, 32, 128, 200])
def test_rows_inv_norm_gaussian(dev, d):
    import torch
    from arx import ops
    rng = np.random.default_rng(d)
    for n in (0, 1, 65, 1000):
        for pad in ((4, 3) if d % 4 == 0 else (3,)):        # the float4 path (ld % 4 == 0) and the scalar one
            x = (rng.standard_normal((n, d)) * 3.0).astype(np.float32)
            if n > 1:
                x[n // 2] = 0.0                             # a zero row
            E = _padded(dev, x, pad)
            assert E.stride(0) == d + pad > d
            out = torch.full((n + 2,), 7.0, dtype=torch.float32, device=dev)
            ops.rows_inv_norm(E, out[1:1 + n])
            got = out.cpu().numpy()
            assert got[0] == 7.0 and got[-1] == 7.0, (n, pad)
            want = S.inv_norm64(x)
            tol = 2.0 * (d / 2.0 + 2.0) * 2.0 ** -24
            assert np.all(np.abs(got[1:1 + n] - want) <= tol * want), (n, pad)
            if n > 1:
                assert got[1 + n // 2] == 0.0 and not np.signbit(got[1 + n // 2])


@pytest.mark.parametrize("d", [16, 32, 64, 128])
def test_rows_inv_norm_exact(dev, d):
    import torch
    from arx import ops
    x = S.exact_table(np.random.default_rng(d), 65, d)
    for pad in (4, 1):
        out = torch.empty(65, dtype=torch.float32, device=dev)
        ops.rows_inv_norm(_padded(dev, x, pad), out)
        _bits_equal(out.cpu().numpy(), S.inv_norm64(x).astype(np.float32), "inv norm d=%d pad=%d" % (d, pad))


# ---------------------------------------------------------------------------------------------------------
# arx_gather_rows_unit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,exact,pad", [(64, True, 4), (128, True, 8), (16, True, 3), (7, False, 1), (200, False, 4)])
def test_gather_rows_unit(dev, d, exact, pad):
    from arx import ops
    rng = np.random.default_rng(d)
    n = 40
    x = S.exact_table(rng, n, d) if exact else (rng.standard_normal((n, d)) * 2.0).astype(np.float32)
    x[S.ZERO_ROW] = 0.0
    rows = np.array([3, -1, 0, 3, -5, n - 1, S.ZERO_ROW, 17], dtype=np.int32)      # negatives, a row twice, a zero row
    base, out = _wide(dev, len(rows), d, 55.0, off=4, pad=12)                       # ldo = d + 12 > d
    ops.gather_rows_unit(_padded(dev, x, pad), _t(dev, rows), out)
    assert _canary_ok(base, d, 55.0)
    got = out.cpu().numpy()
    want = np.where((rows >= 0)[:, None], x[np.maximum(rows, 0)].astype(np.float64) *
                    S.inv_norm64(x)[np.maximum(rows, 0)][:, None], 0.0)
    assert not got[rows < 0].any() and not got[rows == S.ZERO_ROW].any()
    if exact:
        _bits_equal(got + np.float32(0.0), (want + 0.0).astype(np.float32), "unit rows")
        assert np.array_equal(got[0], got[3])
    else:
        tol = 2.0 * (d / 2.0 + 3.0) * 2.0 ** -24
        assert np.all(np.abs(got - want) <= tol * np.abs(want) + 1e-30)
        np.testing.assert_allclose((got.astype(np.float64) ** 2).sum(1)[rows >= 0][[0, 1, 2, 3, 5]], 1.0,
                                   atol=4.0 * (d + 4) * 2.0 ** -24)


# ---------------------------------------------------------------------------------------------------------
# arx_cos_chunk_finish
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_self", [True, False])
def test_cos_chunk_finish(dev, with_self):
    from arx import ops
    rng = np.random.default_rng(5)
    B, ncols, col0 = 6, 70, 130
    L = rng.standard_normal((B, ncols)).astype(np.float32)
    L[2, 5] = -1.5
    scale = rng.random(col0 + ncols).astype(np.float32)
    scale[col0 + 5] = 0.0                                                            # a zero column: -1.5 * 0 -> +0
    sc = np.array([col0, col0 + 20, col0 + ncols - 1, col0 - 1, col0 + ncols, S.KEY_NONE], dtype=np.int32)
    base, lg = _wide(dev, B, ncols, 9.0)
    lg.copy_(_t(dev, L))
    ops.cos_chunk_finish(lg, col0, _t(dev, scale), _t(dev, sc) if with_self else None)
    assert _canary_ok(base, ncols, 9.0)
    want = (L * scale[None, col0:] + np.float32(0.0)).astype(np.float32)
    if with_self:
        want[0, 0] = want[1, 20] = want[2, ncols - 1] = NEG                          # inside, inside, the last column
    got = lg.cpu().numpy()
    _bits_equal(got, want, "finished chunk")
    assert got[2, 5] == 0.0 and not np.signbit(got[2, 5])


# ---------------------------------------------------------------------------------------------------------
# arx_gemm_nt_topk_filter_cos
# ---------------------------------------------------------------------------------------------------------
XROWS, XCOLS = 3, 5
COL_BASE = 1000


def _filter_case(dev, rng, M, N, K, capp, all_survive=False, with_self=True):
    import torch
    from arx import ops
    Eq, Bm = S.exact_table(rng, max(M, 8), K)[:M], S.exact_table(rng, max(N, 8), K)[:N]
    A = (Eq * S.inv_norm64(Eq).astype(np.float32)[:, None]).astype(np.float32)        # unit rows: exact
    scale = S.inv_norm64(Bm).astype(np.float32)
    V = ((A.astype(np.float64) @ Bm.astype(np.float64).T) * scale.astype(np.float64) + 0.0).astype(np.float32)
    assert np.array_equal(V.astype(np.float64), S.cos64(Eq, Bm))                       # exact data: no rounding at all
    thr = np.empty(M, dtype=np.float32)
    for r in range(M):
        # (a column's own value: an exact tie with the threshold, which must lose)
        thr[r] = NEG if (all_survive or r % 4 == 0) else np.sort(V[r])[int(0.7 * (N - 1))]
    sc = np.full(M, S.KEY_NONE, dtype=np.int32)
    for r in range(M):
        if r % 3 == 0:
            sc[r] = COL_BASE + r % min(N, 64)                                        # in the first tile
        elif r % 3 == 1:
            sc[r] = COL_BASE + N - 1                                                 # in the last (partial) tile
        elif r % 5 == 0:
            sc[r] = COL_BASE - 1 if r % 2 else COL_BASE + N                          # just outside the launch
    excluded = np.zeros((M, N), dtype=bool)
    if with_self:
        inside = (sc >= COL_BASE) & (sc < COL_BASE + N)
        excluded[np.nonzero(inside)[0], sc[inside] - COL_BASE] = True
    parts = ops.gemm_nt_topk_parts(M, N)
    assert parts == O.parts_for(ops.device_info()["cu_count"], M, N)
    _, ranges = O.split_ranges(N, parts)
    ld = parts * capp + XCOLS
    cv = torch.full((M + XROWS, ld), NEG, dtype=torch.float32, device=dev)
    ci = torch.full((M + XROWS, ld), O.IDX_FILL, dtype=torch.int32, device=dev)
    th = torch.full((M, 3), 3e38, dtype=torch.float32, device=dev)
    th[:, 2] = _t(dev, thr)
    ov = torch.tensor([5, 0, 5], dtype=torch.int32, device=dev)
    ops.gemm_nt_topk_filter_cos(_padded(dev, A, 4), _padded(dev, Bm, 8), _t(dev, scale),
                                _t(dev, sc) if with_self else None, th[:, 2], COL_BASE, cv[:M], ci[:M], capp, ov[1:2])
    torch.cuda.synchronize()
    ev, ei, over = O.expected_segments(V, thr, ranges, capp, ld, COL_BASE, excluded)
    ev = np.concatenate([ev, np.full((XROWS, ld), NEG, dtype=np.float32)])
    ei = np.concatenate([ei, np.full((XROWS, ld), O.IDX_FILL, dtype=np.int32)])
    what = "M=%d N=%d K=%d capp=%d" % (M, N, K, capp)
    _bits_equal(cv.cpu().numpy(), ev, what + " cand_v")
    assert np.array_equal(ci.cpu().numpy(), ei), what + " cand_i"
    assert ov.cpu().numpy().tolist() == [5, int(over), 5], (what, over)
    return over, parts


@pytest.mark.parametrize("M", [1, 33, 130])
@pytest.mark.parametrize("K", [32, 64, 128])
def test_filter_cos_exact(dev, K, M):
    rng = np.random.default_rng(1000 * K + M)
    seen_parts = set()
    for N in (1, 63, 64, 65, 1500):
        over, parts = _filter_case(dev, rng, M, N, K, capp=max(N, 1))              # a segment can hold its whole range
        assert not over
        seen_parts.add(parts)
    assert max(seen_parts) > 1                                                       # N = 1500: several ranges
    _filter_case(dev, rng, M, 1500, K, capp=1500, with_self=False)                   # NULL self_col: nothing dropped


@pytest.mark.parametrize("K", [32, 64, 128])
def test_filter_cos_overflow(dev, K):
    """thr = -inf and two slots per range: every range overflows, the flag is raised, the slots hold the first two
    eligible columns of the range (a row's self column takes none)."""
    rng = np.random.default_rng(K)
    over, _ = _filter_case(dev, rng, 33, 1500, K, capp=2, all_survive=True)
    assert over
