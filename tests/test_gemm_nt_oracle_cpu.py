"""The numpy oracle of test_gemm_nt_fused_gpu.py (tests/gemm_nt_oracle.py) against brute force: the range split, the
candidate segments with and without exclusion lists and a capacity, tf.nn.top_k's order and the chunk + merge
composition.  No GPU, no library."""
import numpy as np
import pytest

import gemm_nt_oracle as O


@pytest.mark.parametrize("N,parts", [(1, 1), (5, 1), (64, 1), (65, 2), (65, 1), (1000, 16), (1000, 6), (25601, 134),
                                     (16385, 129)])
def test_split_ranges_partition(N, parts):
    tpb, ranges = O.split_ranges(N, parts)
    assert len(ranges) == parts and ranges[0][0] == 0 and ranges[-1][1] == N
    for p, (lo, hi) in enumerate(ranges):
        assert lo < hi and lo == p * tpb * 64 and hi - lo <= tpb * 64
        assert p == 0 or ranges[p - 1][1] == lo
        assert p == parts - 1 or hi - lo == tpb * 64


def test_split_ranges_refuses_a_count_the_kernel_cannot_report():
    with pytest.raises(AssertionError):
        O.split_ranges(64 * 10, 7)            # tpb = 2 covers the 10 tiles with 5 ranges, never 7


@pytest.mark.parametrize("cu,M,N,want", [(256, 1, 64 * 512, 512), (256, 1, 64 * 513, 257), (256, 300, 25601, 134),
                                         (256, 129, 5, 1), (8, 128, 64 * 40 + 1, 14), (304, 300, 20011, 157)])
def test_parts_for_matches_the_launch_rule(cu, M, N, want):
    """ns = min(ceil(2 cu / panels), tiles), tpb = ceil(tiles / ns), parts = ceil(tiles / tpb), by hand."""
    assert O.parts_for(cu, M, N) == want
    O.split_ranges(N, want)


def _ex_case(rng, M, N, col_base):
    keys = rng.integers(-1, 4, size=5).astype(np.int32)
    lists = [np.unique(rng.integers(col_base - 3, col_base + N + 3, size=n)).astype(np.int32) for n in (0, 7, N, 2)]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return keys, 5, ptr, np.concatenate(lists).astype(np.int32)


def test_excl_mask_brute():
    rng = np.random.default_rng(0)
    M, N, base = 13, 40, 100
    ex = _ex_case(rng, M, N, base)
    got = O.excl_mask(M, N, base, ex)
    keys, kr, ptr, cols = ex
    for r in range(M):
        key = keys[r % kr]
        listed = set() if key < 0 else set(int(c) for c in cols[ptr[key]:ptr[key + 1]])
        for c in range(N):
            assert got[r, c] == ((base + c) in listed)
    assert not O.excl_mask(M, N, base, None).any()


@pytest.mark.parametrize("capp", [1, 2, 5, 200])
@pytest.mark.parametrize("with_ex", [False, True])
def test_expected_segments_brute(capp, with_ex):
    rng = np.random.default_rng(capp + 10 * with_ex)
    M, N, base, parts = 9, 333, 1000, 3
    L = (rng.integers(-4, 5, size=(M, N)) / 2.0).astype(np.float32)
    L[2, 7] = -np.inf
    thr = np.array([0.5, -np.inf, np.inf, np.nan, 2.0, 1.5, -2.0, 0.0, 1.0], dtype=np.float32)
    tpb, ranges = O.split_ranges(N, parts)
    exm = O.excl_mask(M, N, base, _ex_case(rng, M, N, base)) if with_ex else None
    ld = parts * capp + 2
    cv, ci, over = O.expected_segments(L, thr, ranges, capp, ld, base, exm)
    bv = np.full((M, ld), -np.inf, dtype=np.float32)
    bi = np.full((M, ld), O.IDX_FILL, dtype=np.int32)
    bover = False
    for r in range(M):
        for p, (lo, hi) in enumerate(ranges):
            n = 0
            for c in range(lo, hi):
                if not (L[r, c] > thr[r]) or (exm is not None and exm[r, c]):
                    continue
                if n < capp:
                    bv[r, p * capp + n], bi[r, p * capp + n] = L[r, c], base + c
                else:
                    bover = True
                n += 1
    np.testing.assert_array_equal(cv, bv)
    np.testing.assert_array_equal(ci, bi)
    assert over == bover
    assert (ci[2] != base + 7).all() and (ci[3] == O.IDX_FILL).all() and (ci[2] == O.IDX_FILL).all()


@pytest.mark.parametrize("k", [1, 7, 50])
def test_topk_tf_brute_and_chunk_merge(k):
    rng = np.random.default_rng(k)
    M, N = 6, 41
    L = (rng.integers(-3, 4, size=(M, N)) / 2.0).astype(np.float32)          # many ties
    exm = rng.random((M, N)) < 0.3
    exm[1, :] = True                                                          # nothing eligible
    exm[2, 3:] = True                                                         # three eligible columns
    for ex in (None, exm):
        v, i = O.topk_tf(L, k, ex)
        for r in range(M):
            cols = [c for c in range(N) if ex is None or not ex[r, c]]
            cols.sort(key=lambda c: (-float(L[r, c]), c))
            cols = cols[:k]
            assert i[r, :len(cols)].tolist() == cols
            assert v[r, :len(cols)].tolist() == [float(L[r, c]) for c in cols]
            assert (i[r, len(cols):] == -1).all() and np.isneginf(v[r, len(cols):]).all()
    if k <= N:
        v, i = O.topk_tf(L, k)
        for chunk in (max(k, 8), max(k, 13), 41, 64):
            cv, ci = O.topk_chunked(L, k, chunk)
            np.testing.assert_array_equal(cv, v)
            np.testing.assert_array_equal(ci, i)


def test_lse64_handles_neg_inf():
    x = np.array([[0.0, -np.inf, 1.0], [-np.inf, -np.inf, -np.inf], [700.0, 710.0, -np.inf]])
    got = O.lse64(x)
    assert np.isneginf(got[1])
    np.testing.assert_allclose(got[0], np.log(1 + np.e))
    np.testing.assert_allclose(got[2], 710.0 + np.log1p(np.exp(-10.0)))


def _online_lse(x, start_max):
    """The kNtLse epilogue of csrc/gemm_nt.hip restated in float32 numpy for one row: lane l of 32 folds columns
    l, 32 + l, 64 + l, ... with (lm, ls) <- v by dd = v - lm, ex = exp(-|dd|), ls = dd > 0 ? ls * ex + 1 : ls + ex,
    lm = max(lm, v), starting from (start_max, 0); the lanes then meet by a butterfly that gives a (-inf, .) side no
    weight."""
    f = np.float32
    lm = np.full(32, start_max, dtype=f)
    ls = np.zeros(32, dtype=f)
    with np.errstate(invalid='ignore', over='ignore'):
        for c0 in range(0, len(x), 32):
            v = np.full(32, np.nan, dtype=f)
            n = min(32, len(x) - c0)
            v[:n] = x[c0:c0 + n]
            dd = v - lm
            ex = np.exp(-np.abs(dd)).astype(f)
            new = np.where(dd > 0, ls * ex + f(1), ls + ex).astype(f)
            live = np.arange(32) < n
            ls = np.where(live, new, ls)
            lm = np.where(live, np.fmax(lm, v), lm)
        o = 16
        while o:
            m2, s2 = lm[np.arange(32) ^ o], ls[np.arange(32) ^ o]
            mn = np.fmax(lm, m2)
            ls = (np.where(np.isneginf(lm), f(0), ls * np.exp(lm - mn)) +
                  np.where(np.isneginf(m2), f(0), s2 * np.exp(m2 - mn))).astype(f)
            lm = mn
            o >>= 1
    with np.errstate(divide='ignore'):
        return float(lm[0] + np.log(ls[0]))


def test_online_lse_recurrence_start_state():
    """Why the epilogue starts from (-FLT_MAX, 0): from (-inf, 0) a lane whose first column is -inf forms
    -inf - -inf = NaN and keeps it through every later rescale; from the lowest finite float a -inf logit adds
    nothing in every state, the first finite logit still gives ex = 0, ls = 1, and a range of nothing but -inf ends
    as -FLT_MAX + log(0) = -inf."""
    rng = np.random.default_rng(0)
    fmax = np.finfo(np.float32).max
    plain = (rng.standard_normal(192) * 3).astype(np.float32)
    cases = {'plain': plain.copy(), 'first': plain.copy(), 'tile': plain.copy(), 'ragged': plain[:70].copy(),
             'all': np.full(128, -np.inf, dtype=np.float32), 'big': (plain * 25).astype(np.float32)}
    cases['first'][[0, 33]] = -np.inf
    cases['tile'][:64] = -np.inf
    cases['ragged'][[0, 69]] = -np.inf
    for name, x in cases.items():
        want = float(O.lse64(x[None, :])[0])
        got = _online_lse(x, -fmax)
        if np.isneginf(want):
            assert np.isneginf(got), name
        else:
            np.testing.assert_allclose(got, want, rtol=1e-5, err_msg=name)
    assert np.isnan(_online_lse(cases['first'], -np.inf)) and np.isnan(_online_lse(cases['tile'], -np.inf))
    np.testing.assert_allclose(_online_lse(plain, -np.inf), _online_lse(plain, -fmax), rtol=0)
