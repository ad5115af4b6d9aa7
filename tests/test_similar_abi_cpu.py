"""The host half of similar_items (csrc/similar.hip, arx_gemm_nt_topk_filter_cos): argument validation of the four new
exports without a device, and the exact-data premise of the GPU tests -- on tests/similar_oracle.py's dyadic tables a
float32 numpy evaluation of the cosine formula and the float64 oracle agree bit for bit."""
import numpy as np

import similar_oracle as S


def test_similar_exports_validate_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib
    EINVAL = -1

    def err():
        m = lib.arx_last_error()
        return m.decode() if m else ""
    # (pointers are only compared with NULL and checked for alignment before the first HIP call: multiples of 16
    # stand in for them)
    P = 4096

    def norm(E=P, ld=64, n=8, d=64, out=P):
        return lib.arx_rows_inv_norm(E, ld, n, d, out, None)
    for kw in (dict(E=None), dict(out=None), dict(n=-1), dict(d=0), dict(ld=63)):
        assert norm(**kw) == EINVAL and "arx_rows_inv_norm" in err(), kw
    assert norm(n=0) == 0

    def unit(E=P, ld=64, rows=P, B=8, d=64, out=P, ldo=64):
        return lib.arx_gather_rows_unit(E, ld, rows, B, d, out, ldo, None)
    for kw in (dict(E=None), dict(rows=None), dict(out=None), dict(B=-1), dict(d=0), dict(ld=60), dict(ldo=60)):
        assert unit(**kw) == EINVAL and "arx_gather_rows_unit" in err(), kw
    assert unit(B=0) == 0

    def fin(lg=P, ld=64, B=4, col0=0, ncols=64, scale=P, sc=None):
        return lib.arx_cos_chunk_finish(lg, ld, B, col0, ncols, scale, sc, None)
    for kw in (dict(lg=None), dict(scale=None), dict(B=-1), dict(ncols=-1), dict(ld=63), dict(col0=-1),
               dict(col0=2 ** 31 - 10)):
        assert fin(**kw) == EINVAL and "arx_cos_chunk_finish" in err(), kw
    assert fin(B=0) == 0 and fin(ncols=0) == 0 and fin(B=0, sc=P) == 0

    def cos(A=P, lda=64, M=8, Bm=P, ldb=64, N=100, K=64, scale=P, sc=None, thr=P, col_base=0, cv=P, ci=P, ldcand=64,
            capp=32, ov=P):
        return lib.arx_gemm_nt_topk_filter_cos(A, lda, M, Bm, ldb, N, K, scale, sc, thr, 1, col_base, cv, ci, ldcand,
                                               capp, ov, None)
    for kw in (dict(A=None), dict(Bm=None), dict(scale=None), dict(thr=None), dict(cv=None), dict(ci=None),
               dict(ov=None), dict(M=0), dict(M=-1), dict(N=0), dict(N=-5), dict(capp=0), dict(ldcand=0),
               dict(K=16), dict(K=48), dict(K=256), dict(A=P + 4), dict(Bm=P + 8), dict(lda=66), dict(ldb=130),
               dict(lda=32), dict(col_base=-1), dict(col_base=2 ** 31 - 50)):
        assert cos(**kw) == EINVAL and "arx_gemm_nt_topk_filter_cos" in err(), kw


def test_exact_data_float32_and_float64_agree_bit_for_bit():
    for d in (16, 32, 64, 128):
        E = S.exact_table(np.random.default_rng(d), 200, d)
        assert np.array_equal(E[1], E[0]) and not E[S.ZERO_ROW].any()
        s = (E.astype(np.float64) ** 2).sum(1)
        assert set(np.unique(np.sqrt(s[s > 0]) / 2.0 ** np.floor(np.log2(np.sqrt(s[s > 0])))).tolist()) == {1.0}
        c32, c64 = S.cos32(E, E), S.cos64(E, E)
        assert np.array_equal(c32.astype(np.float64), c64)
        assert np.array_equal(np.signbit(c32), np.signbit(c64))           # no -0 on either side
        assert c64[0, 1] == 1.0 and c64[0, 2] == 1.0 and c64[0, 3] == -1.0 and c64[2, 2] == 1.0
        assert not c64[S.ZERO_ROW].any() and not c64[:, S.ZERO_ROW].any()
        # the tie rule and the self column: the query 0 sees 1 and 2 first (cosine 1), its negative last
        v, i = S.topk_cos(c64, 200, self_ids=np.arange(200))
        assert i[0, 0] == 1 and i[0, 1] == 2 and i[0, 198] == 3 and i[0, 199] == -1 and v[0, 199] == -np.inf
        v, i = S.topk_cos(c64, 3)
        assert i[0].tolist() == [0, 1, 2]


def test_random_rule_accepts_the_oracle_and_refuses_a_wrong_list():
    import pytest
    rng = np.random.default_rng(0)
    E = rng.standard_normal((50, 8)).astype(np.float32)
    C = S.cos64(E, E)
    me = np.arange(50)
    v, i = S.topk_cos(C, 5, me)
    assert S.check_random(i, v, C, 5, me, S.cos_atol(8)) == 0.0
    bad = i.copy()
    bad[7, 4] = np.argmin(C[7])
    with pytest.raises(AssertionError):
        S.check_random(bad, v, C, 5, me, S.cos_atol(8))
    with pytest.raises(AssertionError):
        S.check_random(S.topk_cos(C, 5)[1], S.topk_cos(C, 5)[0], C, 5, me, S.cos_atol(8))    # holds the query itself
