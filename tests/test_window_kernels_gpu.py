"""Direct C-ABI parity of the fused context window (csrc/window.hip): arx_gather_window_fwd against an fp64 numpy
restatement and arx_sparse_site_window bit for bit, at a batch that is no multiple of the rows a wave serves
(mb = 37), windows below / at / above the four-loads-in-flight unroll (n = 1, 2, 5), row widths of one lane, a
non-power-of-two lane group and the headline d = 128, a non-identity cat_map, ids repeated inside a window and
across rows, ldo > d, and with / without the user half (base).  Tolerance: the one of the one-hot gather's direct
tests (RTOL / ATOL of tests/test_kernels_direct_gpu.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-4
ATOL = 1e-5
MB = 37


def _t(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _case(n, d, seed):
    rng = np.random.default_rng(seed)
    Vf, N = 211, 150
    E = rng.standard_normal((Vf, d)).astype(np.float32)
    cmap = rng.permutation(Vf)[:N].astype(np.int32)            # non-identity, one-to-one
    cmap[7] = cmap[3]                                          # ... and two ids of one row
    ids = rng.integers(0, N, size=(n, MB)).astype(np.int32)
    if n > 1:
        ids[1, :5] = ids[0, :5]                                # an id repeated inside a window
    ids[:, 9] = ids[:, 8]                                      # two rows with the same window
    ids[0, 20:30] = ids[0, 20]                                 # one id across many rows
    base = rng.standard_normal((MB, d)).astype(np.float32)
    return E, cmap, ids, base


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("d", [4, 36, 128])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_gather_window_fwd(dev, n, d, with_base):
    import torch
    from arx import _lib
    E, cmap, ids, base = _case(n, d, seed=100 * n + d)
    scale, base_scale = 0.5 / n, 0.5
    ldo, fill = d + 8, 7.0
    tE, tc, ti = _t(dev, E), _t(dev, cmap), _t(dev, ids.reshape(-1))
    tb = torch.full((MB, d + 4), 3.0, dtype=torch.float32, device=dev)          # ldb > d as well
    tb[:, :d] = _t(dev, base)
    out = torch.full((MB, ldo), fill, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call("arx_gather_window_fwd", tE.data_ptr(), tc.data_ptr(), ti.data_ptr(), n, MB, d, scale,
              tb.data_ptr() if with_base else 0, d + 4, base_scale, out.data_ptr(), ldo, stream)
    got = out.cpu().numpy()
    want = scale * E.astype(np.float64)[cmap[ids]].sum(0)
    if with_base:
        want = want + base_scale * base.astype(np.float64)
    np.testing.assert_allclose(got[:, :d], want, rtol=RTOL, atol=ATOL)
    assert np.all(got[:, d:] == fill)                          # nothing past column d of a row
    # identity map: cat_map = NULL reads E[ids]
    out2 = torch.empty((MB, d), dtype=torch.float32, device=dev)
    rows = _t(dev, cmap[ids].reshape(-1))
    _lib.call("arx_gather_window_fwd", tE.data_ptr(), 0, rows.data_ptr(), n, MB, d, scale,
              tb.data_ptr() if with_base else 0, d + 4, base_scale, out2.data_ptr(), d, stream)
    np.testing.assert_array_equal(out2.cpu().numpy(), got[:, :d])
    # the same launch again gives the same bits (one lane sums a window in ascending t, no atomics)
    out3 = torch.empty((MB, d), dtype=torch.float32, device=dev)
    _lib.call("arx_gather_window_fwd", tE.data_ptr(), 0, rows.data_ptr(), n, MB, d, scale,
              tb.data_ptr() if with_base else 0, d + 4, base_scale, out3.data_ptr(), d, stream)
    np.testing.assert_array_equal(out3.cpu().numpy(), out2.cpu().numpy())


def test_gather_window_matches_ops_wrapper_and_one_hot_gather(dev):
    """n = 1 without base is the plain one-hot gather: the same bits as arx_gather_onehot_fwd."""
    import torch
    from arx import ops
    E, cmap, ids, _ = _case(1, 36, seed=5)
    tE, tc, ti = _t(dev, E), _t(dev, cmap), _t(dev, ids.reshape(-1))
    a = torch.empty((MB, 36), dtype=torch.float32, device=dev)
    b = torch.empty((MB, 36), dtype=torch.float32, device=dev)
    ops.gather_window(tE, tc, ti, 1, a, scale=0.25)
    ops.gather_onehot(tE, None, tc, ti, b, scale=0.25)
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("d", [4, 36, 128])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_sparse_site_window(dev, n, d):
    import torch
    from arx import _lib, ops
    _, cmap, ids, _ = _case(n, d, seed=100 * n + d)
    ids = ids.copy()
    ids[0, 4] = -1                                             # an empty slot: no update
    flat = ids.reshape(-1)
    row_base, coef = 1000, 0.5 / n
    ti, tc = _t(dev, flat), _t(dev, cmap)
    keys = torch.full((n * MB + 3,), -7, dtype=torch.int32, device=dev)
    src = torch.full((n * MB + 3,), -7, dtype=torch.int32, device=dev)
    cf = torch.full((n * MB + 3,), -7.0, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call("arx_sparse_site_window", tc.data_ptr(), ti.data_ptr(), n, MB, row_base, coef, keys.data_ptr(),
              src.data_ptr(), cf.data_ptr(), stream)
    want_keys = np.where(flat < 0, ops.KEY_NONE, cmap[np.maximum(flat, 0)]).astype(np.int32)
    want_src = (row_base + np.arange(n * MB) % MB).astype(np.int32)
    np.testing.assert_array_equal(keys.cpu().numpy()[:n * MB], want_keys)
    np.testing.assert_array_equal(src.cpu().numpy()[:n * MB], want_src)
    np.testing.assert_array_equal(cf.cpu().numpy()[:n * MB], np.full(n * MB, np.float32(coef)))
    for t in (keys, src, cf):
        assert np.all(t.cpu().numpy()[n * MB:] == -7)           # nothing past n * mb entries
    # identity map, no src / coef outputs
    keys2 = torch.empty((n * MB,), dtype=torch.int32, device=dev)
    _lib.call("arx_sparse_site_window", 0, ti.data_ptr(), n, MB, 0, 1.0, keys2.data_ptr(), 0, 0, stream)
    np.testing.assert_array_equal(keys2.cpu().numpy(), np.where(flat < 0, ops.KEY_NONE, flat).astype(np.int32))


def test_window_kernels_refuse_bad_arguments(dev):
    import torch
    from arx import _lib
    lib = _lib.lib
    E = torch.zeros((8, 8), dtype=torch.float32, device=dev)
    ids = torch.zeros((8,), dtype=torch.int32, device=dev)
    out = torch.zeros((4, 8), dtype=torch.float32, device=dev)
    keys = torch.zeros((8,), dtype=torch.int32, device=dev)
    e, i, o, k = E.data_ptr(), ids.data_ptr(), out.data_ptr(), keys.data_ptr()
    assert lib.arx_gather_window_fwd(None, None, i, 2, 4, 8, 1.0, None, 0, 0.0, o, 8, None) != 0
    assert lib.arx_gather_window_fwd(e, None, i, 0, 4, 8, 1.0, None, 0, 0.0, o, 8, None) != 0      # n < 1
    assert lib.arx_gather_window_fwd(e, None, i, 2, 4, 6, 1.0, None, 0, 0.0, o, 8, None) != 0      # d % 4
    assert lib.arx_gather_window_fwd(e, None, i, 2, 4, 8, 1.0, None, 0, 0.0, o, 6, None) != 0      # ldo < d
    assert lib.arx_gather_window_fwd(e, None, i, 2, 4, 8, 1.0, e, 6, 0.5, o, 8, None) != 0         # ldb < d
    assert lib.arx_sparse_site_window(None, None, 2, 4, 0, 1.0, k, None, None, None) != 0
    assert lib.arx_sparse_site_window(None, i, 0, 4, 0, 1.0, k, None, None, None) != 0
    assert lib.arx_gather_window_fwd(e, None, i, 2, 0, 8, 1.0, None, 0, 0.0, o, 8, None) == 0      # mb = 0: nothing
