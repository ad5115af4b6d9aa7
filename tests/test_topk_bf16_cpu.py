"""recommend(scan_dtype='bf16'): the host half (no GPU).

 1. the error bound the filter's margin rests on (topk.bf16_margin_coeff), against numpy's
    emulation of round-to-nearest-even bf16, and the numpy oracle's filter-then-rescore against the float64 top-k;
 2. the C ABI: the header, its table, argument validation before any HIP call;
 3. where the option may not stand.
"""
import os

import numpy as np
import pytest

import topk_bf16_oracle as O

EINVAL, EUNSUPPORTED = -1, -4


def _err(lib):
    m = lib.arx_last_error()
    return m.decode() if m else ""


# ---------------------------------------------------------------- 1. the bound
def _skewed(rng, V, d, ratio=10.0):
    """item rows whose norms spread over `ratio` x the median (a popular head, a long tail)"""
    P = rng.standard_normal((V, d)).astype(np.float32)
    scale = np.exp(rng.standard_normal(V) * 0.8)
    scale[:: max(1, V // 20)] *= ratio
    return (P * scale[:, None]).astype(np.float32)


def _adversarial_rows(d):
    """rows made to round badly: entries just below and just above a bf16 rounding midpoint, all of one sign (no
    cancellation hides the error), and magnitudes from 2^-20 to 2^20 inside one row"""
    lo = np.float32(1 + 2.0 ** -8 - 2.0 ** -20)          # rounds DOWN to 1
    hi = np.float32(1 + 2.0 ** -8 + 2.0 ** -20)          # rounds UP to 1 + 2^-7
    mid_even = np.float32(1 + 2.0 ** -8)                 # the tie: to the even significand, 1
    mid_odd = np.float32(1 + 3 * 2.0 ** -8)              # the tie: to the even significand, 1 + 2^-6
    mags = (2.0 ** np.linspace(-20, 20, d)).astype(np.float32)
    rows = [np.full(d, lo), np.full(d, hi), -np.full(d, lo), np.full(d, mid_even), np.full(d, mid_odd),
            np.where(np.arange(d) % 2 == 0, lo, hi), mags * lo, mags * hi, mags[::-1] * hi,
            np.where(np.arange(d) % 2 == 0, 1, -1) * mags * lo, np.zeros(d)]
    return np.asarray(rows, dtype=np.float32)


def test_bf16_rounding_emulation_is_round_to_nearest_even():
    x = np.array([1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20,
                  -(1 + 2.0 ** -8), 0.0, -0.0, 2.0 ** -130, np.nan], dtype=np.float32)
    got = O.bf16_round(x)
    exp = np.array([1.0, 1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 1.0, -1.0, 0.0, -0.0, 2.0 ** -130, np.nan],
                   dtype=np.float32)
    np.testing.assert_array_equal(got, exp)
    assert O.bf16_bits(np.array([np.nan], dtype=np.float32))[0] == 0x7fc0
    assert np.signbit(got[7]) and not np.signbit(got[6])


@pytest.mark.parametrize("d", [32, 64, 128])
def test_margin_bounds_the_bf16_error_for_every_pair(d):
    """|float64 exact - bf16 product summed in float32| <= bf16_margin_coeff(d) |u| |p| for every (row, column): random
    data, skewed item norms, the adversarial rows against each other and against the random ones."""
    from arx.topk import bf16_margin_coeff, bf16_margin_coeff_f32
    c = bf16_margin_coeff(d)
    assert c == 2.0 ** -7 * (1 + 2.0 ** -9) + (d + 8) * 2.0 ** -22
    assert c <= bf16_margin_coeff_f32(d) <= c * (1 + 2.0 ** -22)
    assert np.float32(bf16_margin_coeff_f32(d)) == bf16_margin_coeff_f32(d)        # (a float32: the kernel's argument)
    rng = np.random.default_rng(d)
    adv = _adversarial_rows(d)
    U = np.concatenate([rng.standard_normal((48, d)).astype(np.float32), adv])
    P = np.concatenate([_skewed(rng, 3000, d), adv, rng.standard_normal((500, d)).astype(np.float32)])
    err = np.abs(O.exact_dot(U, P) - O.approx_dot(U, P).astype(np.float64))
    lim = c * O.norms(U)[:, None] * O.norms(P)[None, :]
    worst = float((err / np.where(lim > 0, lim, 1.0)).max())
    print("d=%d: largest error / margin = %.3f" % (d, worst))
    assert (err <= lim).all()
    assert worst > 0.05                                      # (not vacuous: the data does reach into the margin)


@pytest.mark.parametrize("d", [32, 64, 128])
def test_oracle_filter_then_rescore_returns_the_float64_topk(d):
    """Skewed norms, a bias, eligibility at ~50 %: every column of the true top-k survives the widened filter, so the
    oracle's result IS the float64 top-k; and the filter is a filter -- it drops most of the tail."""
    from arx.topk import bf16_margin_coeff
    rng = np.random.default_rng(10 + d)
    B, V, n0, k = 24, 6000, 2000, 20
    U = rng.standard_normal((B, d)).astype(np.float32)
    P = _skewed(rng, V, d)
    bias = (rng.standard_normal(V) * 0.5).astype(np.float32)
    for eligible in (None, rng.random((B, V)) < 0.5):
        v, i, n = O.filter_then_rescore(U, P, bias, k, n0, bf16_margin_coeff(d), eligible)
        ev, ei, _ = O.exact_topk(U, P, bias, k, eligible)
        np.testing.assert_array_equal(i, ei)
        np.testing.assert_array_equal(v, ev)
        assert (i >= n0).any() and n.max() < (V - n0) // 4
    # without the margin the same filter LOSES winners on data made for it: tail columns 1 + 2^-9 (image 1.0) against a
    # threshold of 1 + 2^-10 per entry
    U1 = np.ones((2, d), dtype=np.float32)
    P1 = np.zeros((40, d), dtype=np.float32)
    P1[:k] = 1 + 2.0 ** -10
    P1[30:] = 1 + 2.0 ** -9
    _, i0, _ = O.filter_then_rescore(U1, P1, None, k, 30, 0.0)
    _, i1, _ = O.filter_then_rescore(U1, P1, None, k, 30, bf16_margin_coeff(d))
    assert (i0 < 30).all() and sorted(i1[0][:10].tolist()) == list(range(30, 40))


# ---------------------------------------------------------------- 2. the C ABI without a GPU
def test_header_and_its_table_stay_in_step():
    """include/arx_topk_bf16.h against TOPK_BF16_PROTOTYPES of arx/_lib.py by TYPE, with the parser and the comparator
    of tests/test_abi_signatures_cpu.py; the names are exported, arx.h includes the header, PROTOTYPES keeps its size."""
    import test_abi_signatures_cpu as A
    from arx import _lib
    decls = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_topk_bf16.h")).read())
    names = ["arx_cand_rescore", "arx_gemm_nt_topk_filter_bf16", "arx_rows_bf16_norm"]
    assert sorted(decls) == names
    lines = open(os.path.join(A.ROOT, "a-recsys_amd", "arx", "_lib.py")).read().split("\n")
    end = next(i for i, l in enumerate(lines) if l.startswith("class ArxError"))
    ns = {"__file__": "_lib.py"}
    exec(compile("\n".join(l for l in lines[:end] if not l.startswith("import torch")), "_lib.py(bf16)", "exec"), ns)
    protos = ns["TOPK_BF16_PROTOTYPES"]
    assert sorted(protos) == names == sorted(_lib.TOPK_BF16_PROTOTYPES)
    bad = [m for name in names for m in A.mismatches(name, decls[name], protos[name])]
    assert not bad, "\n".join(bad)
    # not vacuous: the float coefficient taken for an int is reported
    res, args = protos["arx_gemm_nt_topk_filter_bf16"]
    kf = next(k for k, a in enumerate(args) if a is A.C.c_float)
    wrong = list(args)
    wrong[kf] = A.C.c_int
    assert A.mismatches("arx_gemm_nt_topk_filter_bf16", decls["arx_gemm_nt_topk_filter_bf16"], (res, wrong))
    for name in names:
        assert hasattr(_lib.lib, name) and name not in _lib.PROTOTYPES
        assert getattr(_lib.lib, name).argtypes == list(protos[name][1])
    assert '#include "arx_topk_bf16.h"' in open(os.path.join(A.ROOT, "include", "arx.h")).read()
    assert len(_lib.PROTOTYPES) == A.N_ENTRY_POINTS


def test_rows_bf16_norm_argument_validation_without_gpu():
    from arx import _lib
    lib = _lib.lib
    P = 256                                   # stands in for a device pointer: only compared with NULL / its alignment
    f = lib.arx_rows_bf16_norm
    #        P  ldp  N  K  img ldi norms stream
    assert f(None, 128, 4, 128, P, 128, P, None) == EINVAL and "arx_rows_bf16_norm" in _err(lib)
    assert f(P, 128, 4, 128, None, 128, P, None) == EINVAL
    assert f(P, 128, 4, 128, P, 128, None, None) == EINVAL
    assert f(P, 128, -1, 128, P, 128, P, None) == EINVAL
    assert f(P, 128, 4, 0, P, 128, P, None) == EINVAL
    assert f(P, 100, 4, 100, P, 104, P, None) == EUNSUPPORTED and "K %" in _err(lib)       # K % 8
    assert f(P, 1024, 4, 520, P, 1024, P, None) == EUNSUPPORTED                            # K > 512
    assert f(P, 64, 4, 128, P, 128, P, None) == EINVAL and "ldp" in _err(lib)              # ldp < K
    assert f(P, 130, 4, 128, P, 128, P, None) == EINVAL                                    # ldp % 4
    assert f(P, 128, 4, 128, P, 132, P, None) == EINVAL                                    # ldi % 8
    assert f(P + 4, 128, 4, 128, P, 128, P, None) == EINVAL and "aligned" in _err(lib)
    assert f(P, 128, 4, 128, P + 8, 128, P, None) == EINVAL and "aligned" in _err(lib)
    assert f(P, 128, 0, 128, P, 128, P, None) == 0                                         # nothing to do


def test_filter_bf16_argument_validation_without_gpu():
    from arx import _lib
    lib = _lib.lib
    P = 256
    f = lib.arx_gemm_nt_topk_filter_bf16
    # (host only: the column split needs the CU count, which a GPU-less box does not have -- so only the checks that
    # come before it are exercised here)
    args = dict(A=P, lda=128, M=256, img=P, ldbi=128, coln=P, N=100000, K=128, coeff=0.0079, bias=None, thr=P,
                ldthr=100, col_base=65536, cv=P, ci=P, ldc=4096, capp=32, ovf=P, keys=P, key_rows=256, ptr=P, cols=P,
                tags=P, any=P, all=P, want_rows=256)

    def call(**kw):
        a = dict(args)
        a.update(kw)
        return f(*a.values(), None)
    for k in ("A", "img", "coln", "thr", "cv", "ci", "ovf"):
        assert call(**{k: None}) == EINVAL, k
        assert "arx_gemm_nt_topk_filter_bf16" in _err(lib)
    for k in (96, 16, 256):
        assert call(K=k, lda=256, ldbi=256) == EUNSUPPORTED and "K must be" in _err(lib)
    assert call(M=0) == EINVAL and call(N=0) == EINVAL and call(capp=0) == EINVAL and call(ldc=0) == EINVAL
    assert call(lda=64) == EINVAL and call(ldbi=64) == EINVAL                     # < K
    for bad in (-1.0, float('inf'), float('nan')):
        assert call(coeff=bad) == EINVAL and "coeff" in _err(lib)
    for k in ("keys", "ptr", "cols"):                                              # optional, but only all together
        assert call(**{k: None}) == EINVAL, k
        assert "row_keys" in _err(lib)
    assert call(key_rows=0) == EINVAL
    for k in ("tags", "any", "all"):
        assert call(**{k: None}) == EINVAL, k
        assert "col_tags" in _err(lib)
    assert call(want_rows=0) == EINVAL
    assert call(col_base=-1) == EINVAL
    assert call(col_base=2 ** 31 - 50) == EINVAL and "2^31" in _err(lib)
    assert call(A=P + 4) == EINVAL and "aligned" in _err(lib)
    assert call(img=P + 8) == EINVAL and "aligned" in _err(lib)
    assert call(lda=130) == EINVAL and call(ldbi=132) == EINVAL


def test_cand_rescore_argument_validation_without_gpu():
    from arx import _lib
    lib = _lib.lib
    P = 256
    f = lib.arx_cand_rescore
    #        U  ldu  B  P  ldp pbias V   d   cv ci ldcand ncand stream
    assert f(None, 64, 4, P, 64, P, 100, 64, P, P, 32, 32, None) == EINVAL and "arx_cand_rescore" in _err(lib)
    assert f(P, 64, 4, None, 64, P, 100, 64, P, P, 32, 32, None) == EINVAL
    assert f(P, 64, 4, P, 64, P, 100, 64, None, P, 32, 32, None) == EINVAL
    assert f(P, 64, 4, P, 64, P, 100, 64, P, None, 32, 32, None) == EINVAL
    assert f(P, 64, -1, P, 64, P, 100, 64, P, P, 32, 32, None) == EINVAL
    assert f(P, 64, 4, P, 64, P, 2 ** 31, 64, P, P, 32, 32, None) == EINVAL and "2^31" in _err(lib)
    assert f(P, 64, 4, P, 64, P, 100, 6, P, P, 32, 32, None) == EINVAL                     # d % 4
    assert f(P, 512, 4, P, 512, P, 100, 260, P, P, 32, 32, None) == EUNSUPPORTED and "d=260" in _err(lib)
    assert f(P, 32, 4, P, 64, P, 100, 64, P, P, 32, 32, None) == EINVAL                    # ldu < d
    assert f(P, 64, 4, P, 66, P, 100, 64, P, P, 32, 32, None) == EINVAL                    # ldp % 4
    assert f(P + 4, 64, 4, P, 64, P, 100, 64, P, P, 32, 32, None) == EINVAL and "aligned" in _err(lib)
    assert f(P, 64, 4, P, 64, P, 100, 64, P, P, 16, 32, None) == EINVAL and "ldcand" in _err(lib)
    assert f(P, 64, 2 ** 20, P, 64, P, 100, 64, P, P, 2 ** 12, 2 ** 12, None) == EINVAL    # B * ncand >= 2^31
    assert f(P, 64, 0, P, 64, None, 100, 64, P, P, 32, 32, None) == 0                      # nothing to do
    assert f(P, 64, 4, P, 64, None, 100, 64, P, P, 32, 0, None) == 0


# ---------------------------------------------------------------- 3. where the option may not stand
def test_scan_dtype_rules():
    from arx import topk
    assert topk.check_scan_dtype(None, True, None, False) is False
    assert topk.check_scan_dtype('f32', True, 0.5, True) is False
    assert topk.check_scan_dtype(None, False, None, False) is False
    assert topk.check_scan_dtype('bf16', True, None, False) is True
    with pytest.raises(ValueError):
        topk.check_scan_dtype('fp8', True, None, False)
    with pytest.raises(ValueError):
        topk.check_scan_dtype('bf16', False, None, False)
    with pytest.raises(NotImplementedError, match="sample_temperature"):
        topk.check_scan_dtype('bf16', True, 0.5, False)
    with pytest.raises(NotImplementedError, match="sample_temperature"):
        topk.check_scan_dtype('bf16', True, 0.0, False)            # a temperature of 0 is still the sampled call
    with pytest.raises(NotImplementedError, match="return_logprob"):
        topk.check_scan_dtype('bf16', True, 0.5, True)
    topk.no_scan_dtype("x", None)
    topk.no_scan_dtype("x", 'f32')
    with pytest.raises(NotImplementedError, match="SeqModel.step_recommend: scan_dtype"):
        topk.no_scan_dtype("SeqModel.step_recommend", 'bf16')
    with pytest.raises(ValueError):
        topk.no_scan_dtype("x", 'half')
    # the plan keys: a bf16 plan beside the f32 plan of the same filters; none for a sampled call
    assert [topk.recommend_key(e, t, bf16=True) for e in (False, True) for t in (False, True)] == \
        ['recommend_bf16', 'recommend_tags_bf16', 'recommend_ex_bf16', 'recommend_ex_tags_bf16']
    assert topk.recommend_key(True, False) == 'recommend_ex'
    with pytest.raises(ValueError):
        topk.recommend_key(False, False, sampled=True, bf16=True)


def test_models_refuse_scan_dtype_where_it_does_not_go():
    """The entries themselves, before they touch a device: a sample, return_logprob, SeqModel.step_recommend and
    similar_items raise NotImplementedError naming the option."""
    from arx.attributes.embed_attribute import EmbeddingAttribute
    from arx.hmf.hmf_model import LatentProductModel
    from arx.lstm.seqModel import SeqModel
    from arx.word2vec.linear_seq import LinearSeq
    hmf = object.__new__(LatentProductModel)
    hmf.loss_function = 'ce'
    lin = object.__new__(LinearSeq)
    lin.att_emb, lin.loss_function = None, 'ce'
    for model in (hmf, lin):
        with pytest.raises(NotImplementedError, match="sample_temperature"):
            model.step(None, [0], None, recommend=True, sample_temperature=0.5, scan_dtype='bf16')
        with pytest.raises(NotImplementedError, match="return_logprob"):
            model.step(None, [0], None, recommend=True, sample_temperature=0.5, return_logprob=True,
                       scan_dtype='bf16')
        with pytest.raises(ValueError):
            model.step(None, [0], None, recommend=True, scan_dtype='int8')
        with pytest.raises(ValueError):
            model.step(None, [0], None, scan_dtype='bf16')          # without recommend
    with pytest.raises(NotImplementedError, match="scan_dtype"):
        hmf.step_async(None, [0], None, recommend=True, sample_temperature=0.5, scan_dtype='bf16')
    with pytest.raises(NotImplementedError, match="SeqModel.step_recommend: scan_dtype='bf16'"):
        SeqModel.step_recommend(object.__new__(SeqModel), None, [0], [[0]], [0], 0, scan_dtype='bf16')
    with pytest.raises(NotImplementedError, match="similar_items: scan_dtype='bf16'"):
        EmbeddingAttribute.similar_items(object.__new__(EmbeddingAttribute), [0], 5, scan_dtype='bf16')
