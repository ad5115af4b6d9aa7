"""The helpers behind tests/test_lstm_kernels_gpu.py, checked without a GPU: the dispatch restatement of
tests/lstm_paths.py, the one-hot-weight construction that puts the gate functions under test, and the tolerance's
e_ref on every row of the shape table."""
import numpy as np
import pytest

import lstm_cases as LC
import lstm_paths as LP
from oracle import ref_lstm


@pytest.mark.parametrize("cu", [256, 64])
def test_table_shapes_reach_their_paths(cu):
    for name, ((want_f, want_b), shapes, Bs, _) in LP.table(cu).items():
        for din, h in shapes:
            for B in Bs:
                wb = want_b if want_b != 'mfma' else ('mfma1' if h == 64 else 'mfma2')
                assert LP.fwd_path(cu, B, din, h) == want_f, (name, cu, B, din, h)
                assert LP.bwd_path(cu, B, din, h) == wb, (name, cu, B, din, h)
                assert LP.on_path(cu, name, B, din, h)
    # forward and backward disagree exactly where h is an MFMA size and din is no multiple of 4
    assert LP.fwd_path(cu, 17, 18, 64) == 'generic' and LP.bwd_path(cu, 17, 18, 64) == 'mfma1'
    assert LP.fwd_path(cu, 17, 63, 128) == 'generic' and LP.bwd_path(cu, 17, 63, 128) == 'mfma2'
    assert LP.fwd_path(cu, 17, 64, 192) == LP.bwd_path(cu, 17, 64, 192) == 'generic'


@pytest.mark.parametrize("cu", [256, 64, 1])
def test_r4_wreg_boundary(cu):
    w = LP.wreg_min_B(cu)
    assert w == 32 * cu - 15
    for f in (LP.fwd_path, LP.bwd_path):
        assert f(cu, w - 1, 64, 64) == 'r4' and f(cu, w, 64, 64) == 'wreg'
        assert f(cu, 1, 64, 64) == 'r4' and f(cu, 10 * w, 64, 64) == 'wreg'
        assert f(cu, w, 32, 64) == 'mfma1' and f(cu, w, 64, 128) == 'mfma2'      # the rule is din == h == 64 only
    assert -(-(w - 1) // LP.ROWS) == 2 * cu - 1 and -(-w // LP.ROWS) == 2 * cu and w % LP.ROWS == 1


def test_matrix_tokens_and_coverage():
    m = LC.matrix()
    assert len({c[0] for c in m}) == len(m)
    by = {}
    for _, name, din, h, tok, L, fb, hot in m:
        by.setdefault(name, []).append((tok, fb, hot))
    assert set(by) == set(LP.table(256))
    for name, rows in by.items():
        assert {fb for _, fb, hot in rows if not hot} == set(LC.FORGET_BIASES), name
        assert sum(hot for _, _, hot in rows) == 1, name
    assert {t for t, _, _ in by['wreg']} == {'w', 'w+15', 'w+24'} and 'w-1' in {t for t, _, _ in by['r4']}
    assert [LC.resolve_B(t, 256) for t in ('w-1', 'w', 'w+15', 'w+24', 7)] == [8176, 8177, 8192, 8201, 7]


def test_lds_bytes():
    assert LP.fwd_lds_bytes(380, 128, 'mfma2') == 65536 and LP.fwd_lds_bytes(384, 128, 'mfma2') == 65536 + 512
    assert LP.fwd_lds_bytes(1148, 128, 'mfma2') == LP.LDS_LIMIT < LP.fwd_lds_bytes(1152, 128, 'mfma2')
    assert LP.bwd_lds_bytes(2730, 'generic') <= LP.LDS_DEFAULT < LP.bwd_lds_bytes(2731, 'generic')
    assert LP.fwd_lds_bytes(4, 6826, 'generic') <= LP.LDS_LIMIT < LP.bwd_lds_bytes(6827, 'generic')


@pytest.mark.parametrize("h", [32, 64])
@pytest.mark.parametrize("g", [0, 1, 3])
def test_onehot_construction(h, g):
    """In float64 the oracle's gate g of step 0 is exactly the gate function of the sweep: the inputs are right
    before they meet a kernel."""
    x, W, b, vals, rows = LC.onehot_case(h, g)
    pos, nband = LC.gate_sweep()
    assert np.array_equal(vals[:len(pos)], pos) and np.array_equal(vals[len(pos):], -pos)
    assert np.all(np.diff(pos[:nband]) > 0) and pos[0] == np.float32(0.05) and pos[nband - 1] == np.float32(0.08)
    seam = np.float32(0.0625)
    for v in (seam, np.nextafter(seam, np.float32(0)), np.nextafter(seam, np.float32(1))):
        assert v in pos[:nband]
    assert np.count_nonzero(W) == h and np.all(W[h:] == 0) and np.all(np.signbit(b))
    with np.errstate(invalid='ignore', over='ignore'):          # the inf and NaN rows: 0 * inf
        _, _, gates = ref_lstm.lstm_fwd(x.astype(np.float64), W.astype(np.float64), b.astype(np.float64), 0.0)
    n, v64 = len(vals), vals.astype(np.float64)
    got = gates[0][:, g * h:(g + 1) * h].reshape(-1)[:n]
    want = np.tanh(v64) if g == 1 else 1.0 / (1.0 + np.exp(-v64))
    assert np.array_equal(got, want)
    col = gates[0][:, g * h]
    assert col[rows['pinf']] == 1.0 and col[rows['ninf']] == (-1.0 if g == 1 else 0.0) and np.isnan(col[rows['nan']])
    if g == 1:
        z = gates[0][:, h:2 * h]
        assert not np.signbit(z[rows['pz']]).any() and np.all(z[rows['nz']] == 0) and np.signbit(x[0, rows['nz']]).all()


def test_onehot_cell_construction():
    """With gi, gf, go saturated by a bias of 40 the f64 oracle's c is tanh(sweep) and hs is go * tanh(c)."""
    h = 32
    x, W, b, vals, rows = LC.onehot_case(h, 1, bias=(40.0, -0.0, 40.0, 40.0))
    with np.errstate(invalid='ignore', over='ignore'):
        hs, cs, gates = ref_lstm.lstm_fwd(x.astype(np.float32), W, b, np.float32(0.0))
    fin = rows['pinf']
    assert np.all(gates[0][:fin, :h] == 1.0) and np.all(gates[0][:fin, 3 * h:] == 1.0)      # exactly 1 in f32
    assert np.array_equal(cs[0][:fin], gates[0][:fin, h:2 * h])
    assert np.array_equal(hs[0][:fin], np.tanh(cs[0][:fin]))


def test_e_ref_is_usable():
    """e_ref of every array is finite and non-zero on the inputs of every case of the matrix (the hot variants too),
    so the tolerance can collapse neither to zero nor to infinity."""
    for cid, name, din, h, tok, L, fb, hot in LC.matrix():
        B = LC.resolve_B(tok, 4)                    # (4 CUs: the wreg rows at B of about 120)
        x, W, b, dhs = LC.inputs(L, B, din, h, 1, hot)
        ref, e_ref, cs32, g32 = LC.reference(x, W, b, dhs, fb)
        assert set(e_ref) == {'hs', 'cs', 'gates', 'dz', 'dz_fed'}
        for k, e in e_ref.items():
            assert np.isfinite(e) and e > 0.0, (cid, k, e)
            assert np.all(np.isfinite(ref[k])), (cid, k)
        assert cs32.dtype == np.float32 and g32.dtype == np.float32
        if hot:
            z = np.concatenate([x[0], np.zeros((B, h), np.float32)], 1).astype(np.float64) @ W + b
            assert 30.0 <= np.abs(z).max() <= 200.0, (cid, float(np.abs(z).max()))


def test_ratio_and_poison_rows():
    ref = np.array([1.0, -2.0, 0.0])
    r, err = LC.ratio((ref + np.array([8e-7 + 1e-6, 0.0, 0.0])).astype(np.float64), ref, 1e-7)
    assert abs(r - LC.FACTOR) < 1e-6 and abs(err - 1.8e-6) < 1e-12       # err = 8 e_ref + 1e-6 |ref| sits on the bound
    assert LC.poison_rows(1) == [] and LC.poison_rows(2) == [] and LC.poison_rows(3) == [1]
    assert LC.poison_rows(5) == [1, 2, 3] and LC.poison_rows(33) == [1, 6, 16, 31]
    for B in (3, 4, 5, 7, 15, 16, 17, 33, 66, 8177, 8201):
        rows = LC.poison_rows(B)
        assert rows and 0 not in rows and B - 1 not in rows
