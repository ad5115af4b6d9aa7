"""Sampled recommend (sample_temperature / sample_seed): the host half (no GPU).

 1. the numpy restatement of the noise (tests/sample_oracle.py) reproduces the known answers of the hash;
 2. the law of the oracle: first picks follow softmax(score / tau), top-3 inclusion counts the exact Plackett-Luce
    inclusion probabilities;
 3. topk.sample_params, every ValueError;
 4. the three C ABI entries: header, binding, and the argument checks that come before any HIP call;
 5. the new keywords exist.
"""
import inspect

import numpy as np
import pytest

import sample_oracle as S

EINVAL = -1

KNOWN = [   # seed, row, b0, b1, x at col 0 / 1 / 592 / 999999
    (0, 0, 0xfaed1b10, 0x8209b480, (0x3239eb80, 0xa689faf4, 0x3cea1552, 0x81084fce)),
    (1, 0, 0xe7e786b2, 0x2d0f28c7, (0x8f33de04, 0x73c6f2d3, 0x83ed8c5c, 0x132e3d2f)),
    (1, 129, 0x41ba3c46, 0x74f9b97c, (0x37932f15, 0x7a0a7f9e, 0xdf580f18, 0xf1f0ec8f)),
    (2 ** 63 - 1, 4095, 0x66784503, 0xafc01896, (0x8d7934ab, 0x0ca0ccc5, 0x70eb8dbb, 0x23e19432)),
]
COLS = (0, 1, 592, 999999)


# ---------------------------------------------------------------- 1. the hash
@pytest.mark.parametrize("seed,row,b0,b1,xs", KNOWN)
def test_hash_known_answers(seed, row, b0, b1, xs):
    assert S.row_words(seed, row) == (b0, b1)
    assert tuple(int(v) for v in S.bits(seed, [row], COLS)[0]) == xs


def test_gumbel_known_values_and_range():
    g = S.gumbel64(S.bits(1, [129], COLS))[0]
    np.testing.assert_allclose(g, [-0.4235965, 0.29999707, 1.99169183, 2.87381435], rtol=0, atol=5e-8)
    ends = np.array([0, 0xffffffff], dtype=np.uint32)          # m = 0 and m = 2^23 - 1
    u = S.u_of(ends, np.float32)
    assert u[0] == np.float32(2.0 ** -24) and u[1] == np.float32(1 - 2.0 ** -24) and 0 < u[0] and u[1] < 1
    np.testing.assert_allclose(S.gumbel64(ends), [-2.8116, 16.6356], atol=1e-4)
    x = S.bits(1, range(4), range(1000))
    np.testing.assert_array_equal(S.m_of_u(S.u_of(x, np.float32)), x >> np.uint32(9))


def test_noise_statistics():
    """Rows 0..127 x columns 0..99999 of seed 1: mean gamma, variance pi^2 / 6 (5 sigma of the sample variance is
    0.005 here), no row-to-row or lag-1 structure."""
    g = S.gumbel64(S.bits(1, range(128), range(100000)))
    n = g.size
    assert abs(g.mean() - 0.5772157) < 5 * np.sqrt(1.645 / n)
    assert abs(g.var() - np.pi ** 2 / 6) < 0.005
    z = (g - g.mean(1, keepdims=True)) / g.std(1, keepdims=True)
    sub = z[:, ::5]                                               # 20000 columns
    c = sub @ sub.T / sub.shape[1]
    np.fill_diagonal(c, 0)
    assert np.abs(c).max() < 0.04                                 # (5.7 sigma of 1 / sqrt(20000); 8 128 pairs)
    assert abs((z[:, 1:] * z[:, :-1]).mean()) < 5 / np.sqrt(n)


# ---------------------------------------------------------------- 2. the law
SCORES = [2, 1.5, 1, .5, 0, -.5, -1, 3]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_law_of_the_oracle(seed):
    ids = S.oracle_draws(seed, 4096, SCORES, 1.0, 3)
    assert all(len(set(r)) == 3 for r in ids.tolist())
    chi2, z = S.law_stats(ids, SCORES, 1.0)
    print("seed %d: chi2 %.2f, inclusion %.2f sigma" % (seed, chi2, z))
    assert chi2 < 24.32                                           # the 0.1 % point of chi^2 with 7 degrees
    assert z < 4.5


def test_inclusion_probabilities_are_exact():
    inc = S.pl_inclusion(SCORES, 1.0, 3)
    assert abs(inc.sum() - 3) < 1e-12 and inc.argmax() == 7
    np.testing.assert_allclose(S.pl_inclusion([0.0] * 5, 1.0, 2), [0.4] * 5)
    p = np.exp(SCORES) / np.exp(SCORES).sum()
    np.testing.assert_allclose(S.pl_inclusion(SCORES, 1.0, 1), p)


# ---------------------------------------------------------------- 3. sample_params
def test_sample_params_forms_and_errors():
    from arx.topk import recommend_key, sample_params
    tau, w = sample_params(0.5, 7, 4)
    assert tau.dtype == np.float32 and tau.tolist() == [0.5] * 4 and w.dtype == np.int32 and w.tolist() == [7, 0]
    tau, w = sample_params([0, 1, 2.5, 4], 2 ** 63 - 1, 4)
    assert tau.tolist() == [0, 1, 2.5, 4]
    assert w.view(np.uint32).tolist() == [0xffffffff, 0x7fffffff]
    tau, w = sample_params(np.arange(4), (5 << 32) | 0x80000001, 4)
    assert tau.tolist() == [0, 1, 2, 3] and w.view(np.uint32).tolist() == [0x80000001, 5]
    assert sample_params(1, np.int64(3), 2)[1].tolist() == [3, 0]
    for bad in (-0.1, float('nan'), float('inf'), True, [1, 2, 3], [1] * 5, [1, 1, 1, -1], [1, 1, float('nan'), 1],
                np.ones((4, 1)), [True] * 4, 'hot', 1e39):
        with pytest.raises(ValueError):
            sample_params(bad, 0, 4)
    for bad in (-1, 2 ** 63, 1.0, True, None, '3'):
        with pytest.raises(ValueError):
            sample_params(1.0, bad, 4)
    assert [recommend_key(e, t, True) for e in (False, True) for t in (False, True)] == \
        ['recommend_sample', 'recommend_tags_sample', 'recommend_ex_sample', 'recommend_ex_tags_sample']
    assert recommend_key(True, True) == 'recommend_ex_tags' and recommend_key(False, False, False) == 'recommend'


# ---------------------------------------------------------------- 4. the C ABI without a GPU
def _err(lib):
    m = lib.arx_last_error()
    return m.decode() if m else ""


def test_sample_header_and_its_table_stay_in_step():
    import os
    import test_abi_signatures_cpu as A
    from arx import _lib
    decls = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_sample.h")).read())
    names = ["arx_gemm_nt_topk_filter_sample", "arx_topk_gumbel_add", "arx_topk_gumbel_strip"]
    assert sorted(decls) == names
    lines = open(os.path.join(A.ROOT, "a-recsys_amd", "arx", "_lib.py")).read().split("\n")
    end = next(i for i, l in enumerate(lines) if l.startswith("class ArxError"))
    ns = {"__file__": "_lib.py"}
    exec(compile("\n".join(l for l in lines[:end] if not l.startswith("import torch")), "_lib.py(sample)", "exec"), ns)
    protos = ns["SAMPLE_PROTOTYPES"]
    assert sorted(protos) == names == sorted(_lib.SAMPLE_PROTOTYPES)
    bad = [m for name in names for m in A.mismatches(name, decls[name], protos[name])]
    assert not bad, "\n".join(bad)
    res, args = protos["arx_topk_gumbel_add"]                     # not vacuous: one i64 narrowed is reported
    k64 = next(k for k, a in enumerate(args) if a is A.C.c_int64)
    narrowed = list(args)
    narrowed[k64] = A.C.c_int32
    assert A.mismatches("arx_topk_gumbel_add", decls["arx_topk_gumbel_add"], (res, narrowed))
    for name in names:
        assert hasattr(_lib.lib, name)
        assert all(name not in t for t in (_lib.PROTOTYPES, _lib.TAGS_PROTOTYPES, _lib.SLATE_PROTOTYPES,
                                           _lib.DIVERSE_PROTOTYPES))
        assert getattr(_lib.lib, name).argtypes == list(protos[name][1])
    assert '#include "arx_sample.h"' in open(os.path.join(A.ROOT, "include", "arx.h")).read()


def test_gumbel_add_and_strip_argument_validation_without_gpu():
    from arx import _lib
    lib = _lib.lib
    P = 256                                   # stands in for a device pointer: only compared with NULL
    f = lib.arx_topk_gumbel_add
    #        logits ld  M  col0 ncols tau tau_rows seed stream
    assert f(None, 10, 4, 0, 10, P, 4, P, None) == EINVAL and "arx_topk_gumbel_add" in _err(lib)
    assert f(P, 10, 4, 0, 10, None, 4, P, None) == EINVAL
    assert f(P, 10, 4, 0, 10, P, 4, None, None) == EINVAL
    assert f(P, 10, 4, 0, 10, P, 0, P, None) == EINVAL and "tau_rows" in _err(lib)
    assert f(P, 10, -1, 0, 10, P, 4, P, None) == EINVAL
    assert f(P, 10, 4, -5, 10, P, 4, P, None) == EINVAL
    assert f(P, 10, 4, 0, -1, P, 4, P, None) == EINVAL
    assert f(P, 8, 4, 0, 10, P, 4, P, None) == EINVAL and "ld < ncols" in _err(lib)
    assert f(P, 2 ** 31, 4, 2 ** 31 - 5, 10, P, 4, P, None) == EINVAL and "2^31" in _err(lib)
    assert f(P, 10, 0, 0, 10, P, 4, P, None) == 0                 # nothing to do launches nothing
    assert f(P, 10, 4, 1500, 0, P, 4, P, None) == 0
    g = lib.arx_topk_gumbel_strip
    #        values ldv idx ldi B  k  tau tau_rows seed stream
    assert g(None, 5, P, 5, 4, 5, P, 4, P, None) == EINVAL and "arx_topk_gumbel_strip" in _err(lib)
    assert g(P, 5, None, 5, 4, 5, P, 4, P, None) == EINVAL
    assert g(P, 5, P, 5, 4, 5, None, 4, P, None) == EINVAL
    assert g(P, 5, P, 5, 4, 5, P, 4, None, None) == EINVAL
    assert g(P, 5, P, 5, 4, 0, P, 4, P, None) == EINVAL
    assert g(P, 5, P, 5, 4, 5, P, 0, P, None) == EINVAL
    assert g(P, 4, P, 5, 4, 5, P, 4, P, None) == EINVAL           # ldv < k
    assert g(P, 5, P, 4, 4, 5, P, 4, P, None) == EINVAL           # ldi < k
    assert g(P, 5, P, 5, 0, 5, P, 4, P, None) == 0


def test_filter_sample_argument_validation_without_gpu():
    from arx import _lib
    lib = _lib.lib
    P = 256
    f = lib.arx_gemm_nt_topk_filter_sample
    args = dict(A=P, lda=128, M=256, Bm=P, ldb=128, N=100000, K=128, bias=None, thr=P, ldthr=100, col_base=65536,
                cv=P, ci=P, ldc=4096, capp=32, ovf=P, lse=None, ldl=0, keys=P, key_rows=256, ptr=P, cols=P,
                tags=P, any=P, all=P, want_rows=256, tau=P, tau_rows=256, seed=P)

    def call(**kw):
        a = dict(args)
        a.update(kw)
        return f(*a.values(), None)
    for k in ("A", "Bm", "thr", "cv", "ci", "ovf", "tau", "seed"):
        assert call(**{k: None}) == EINVAL, k
        assert "arx_gemm_nt_topk_filter_sample" in _err(lib)
    assert call(tau_rows=0) == EINVAL and "tau_rows" in _err(lib)
    for k in ("tags", "any", "all"):                                # each group is optional, but only all together
        assert call(**{k: None}) == EINVAL, k
        assert "col_tags" in _err(lib)
    assert call(want_rows=0) == EINVAL
    for k in ("keys", "ptr", "cols"):
        assert call(**{k: None}) == EINVAL, k
        assert "row_keys" in _err(lib)
    assert call(key_rows=0) == EINVAL
    assert call(M=0) == EINVAL and call(N=0) == EINVAL and call(capp=0) == EINVAL and call(ldc=0) == EINVAL
    assert call(lda=64) == EINVAL
    assert call(col_base=-1) == EINVAL
    assert call(col_base=2 ** 31 - 50) == EINVAL and "2^31" in _err(lib)
    assert call(K=96) == EINVAL and "K must be" in _err(lib)
    assert call(A=P + 4) == EINVAL and "aligned" in _err(lib)
    assert call(ldb=130) == EINVAL and "aligned" in _err(lib)


# ---------------------------------------------------------------- 5. the keywords
def test_the_new_keywords_exist():
    from arx import ops, topk
    from arx.attributes.embed_attribute import EmbeddingAttribute
    from arx.hmf.hmf_model import LatentProductModel
    from arx.lstm.seqModel import SeqModel, TopKSoftmax
    from arx.word2vec.linear_seq import LinearSeq
    has = lambda f, *names: all(n in inspect.signature(f).parameters for n in names)
    assert has(LatentProductModel.step, 'sample_temperature', 'sample_seed')
    assert has(LatentProductModel.step_async, 'sample_temperature', 'sample_seed')
    assert has(LinearSeq.step, 'sample_temperature', 'sample_seed')
    assert has(SeqModel.step_recommend, 'sample_temperature', 'sample_seed')
    for node in (topk.TopK, topk.StreamTopK, TopKSoftmax):
        assert has(node.__init__, 'sample')
    assert has(topk.TopKScan.run, 'sample') and has(topk.excluding_twin, 'sample_args')
    assert has(topk.recommend_key, 'sampled')
    assert inspect.signature(LatentProductModel.step).parameters['sample_temperature'].default is None
    for name in ('feed_sample', 'sample_args', 'next_sample_seed'):
        assert callable(getattr(EmbeddingAttribute, name))
    for name in ('topk_gumbel_add', 'topk_gumbel_strip', 'gemm_nt_topk_filter_sample'):
        assert callable(getattr(ops, name))
