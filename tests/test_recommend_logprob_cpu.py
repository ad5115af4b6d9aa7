"""recommend(sample_temperature=, return_logprob=True) without a GPU: the self-checks of the float64 oracle
(tests/recommend_logprob_oracle.py), the ABI of include/arx_sample_logp.h against SAMPLE_LOGP_PROTOTYPES by type,
argument validation of the four entries before any HIP call, recommend_key and the refusals of the models."""
import itertools
import os

import numpy as np
import pytest

import recommend_logprob_oracle as RL

NAMES = ["arx_gemm_nt_rest_mass", "arx_rest_mass_chunk", "arx_sample_logp_finish", "arx_sample_logp_sort"]
EINVAL, EUNSUPPORTED = -1, -4


# ---------------------------------------------------------------- 1. the oracle
def test_oracle_law_sums_to_one_and_last_pick_of_a_full_row_is_certain():
    V, k = 6, 3
    L = np.array([[0.3, -1.2, 2.0, 0.7, -0.4, 1.1]], dtype=np.float32)
    tags = np.array([1, 1, 1, 1, 2, 1], dtype=np.uint32)             # column 4 fails want_any = 1
    elig = RL.eligible(L, tags, np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint32), [[1]])
    assert elig.tolist() == [[True, False, True, True, False, True]]
    for tau in (0.25, 1.0, 4.0):
        total = 0.0
        for order in itertools.permutations(np.nonzero(elig[0])[0], k):
            lp = RL.logp(L, elig, np.array([order]), np.array([tau]))
            assert (lp <= 0).all()
            total += np.exp(lp.sum())
        assert abs(total - 1) <= 1e-12, (tau, total)
    # k == the eligible count: REST is empty and the last pick is certain; -1 columns and tau == 0 rows give 0
    full = np.array([[5, 0, 3, 2, -1]])
    lp = RL.logp(L, elig, full, np.array([0.5]))
    assert lp[0, 3] == 0 and lp[0, 4] == 0 and (lp[0, :3] < 0).all() and np.isfinite(lp).all()
    assert (RL.logp(L, elig, full, np.array([0.0])) == 0).all()
    tol = RL.tolerance(L, elig, np.array([0.5]), lp)
    assert (tol[0] >= 2.0 ** -20 * (1 + 1.7 / 0.5)).all() and (RL.tolerance(L, elig, np.array([0.0]), lp) == 0).all()
    assert RL.worst(lp.astype(np.float32), lp, tol) <= 1


# ---------------------------------------------------------------- 2. the ABI
def test_sample_logp_header_and_its_table_stay_in_step():
    import test_abi_signatures_cpu as A
    from arx import _lib
    decls = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_sample_logp.h")).read())
    assert sorted(decls) == NAMES
    protos = _lib.SAMPLE_LOGP_PROTOTYPES
    assert sorted(protos) == NAMES
    bad = [m for name in NAMES for m in A.mismatches(name, decls[name], protos[name])]
    assert not bad, "\n".join(bad)
    for name in NAMES:                                               # not vacuous: one i64 narrowed to i32 is reported
        res, args = protos[name]
        k64 = next(k for k, a in enumerate(args) if a is A.C.c_int64)
        narrowed = list(args)
        narrowed[k64] = A.C.c_int32
        assert any("parameter %d " % k64 in m for m in A.mismatches(name, decls[name], (res, narrowed)))
        assert hasattr(_lib.lib, name) and getattr(_lib.lib, name).argtypes == list(args)
        assert all(name not in t for t in (_lib.PROTOTYPES, _lib.SAMPLE_PROTOTYPES, _lib.SLATE_SAMPLE_PROTOTYPES))
    assert '#include "arx_sample_logp.h"' in open(os.path.join(A.ROOT, "include", "arx.h")).read()


# ---------------------------------------------------------------- 3. argument validation
def _err(lib):
    m = lib.arx_last_error()
    return m.decode() if m else ""


def test_entries_validate_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib
    A = 4096                                  # stands in for a device pointer: only compared with NULL / alignment

    def sort(idx=A, ldi=8, B=4, k=8, pc=A, ps=A, ldp=8):
        return lib.arx_sample_logp_sort(idx, ldi, B, k, pc, ps, ldp, None)
    for kw in (dict(idx=None), dict(pc=None), dict(ps=None), dict(B=-1), dict(k=0), dict(k=1025, ldi=2000, ldp=2000),
               dict(ldi=7), dict(ldp=7)):
        assert sort(**kw) == EINVAL and "arx_sample_logp_sort" in _err(lib), kw
    assert sort(B=0) == 0

    def chunk(lg=A, ld=100, B=4, col0=0, ncols=100, tau=A, tau_rows=4, pc=A, ps=A, ldp=8, k=8, first=1, m=A, s=A,
              sc=A, ldps=8):
        return lib.arx_rest_mass_chunk(lg, ld, B, col0, ncols, tau, tau_rows, pc, ps, ldp, k, first, m, s, sc, ldps, None)
    for kw in (dict(lg=None), dict(tau=None), dict(pc=None), dict(ps=None), dict(m=None), dict(s=None), dict(sc=None),
               dict(B=-1), dict(ncols=-1), dict(ld=99), dict(tau_rows=0), dict(col0=-1), dict(col0=2 ** 31 - 50),
               dict(k=0), dict(k=1025, ldp=2000, ldps=2000), dict(ldp=7), dict(ldps=7)):
        assert chunk(**kw) == EINVAL and "arx_rest_mass_chunk" in _err(lib), kw
    assert chunk(B=0) == 0

    def fin(idx=A, ldi=8, sc=A, ldps=8, m=A, s=A, ldl=3, P=3, tau=A, tau_rows=4, B=4, k=8, lp=A, ldo=8, v=A, ldv=8):
        return lib.arx_sample_logp_finish(idx, ldi, sc, ldps, m, s, ldl, P, tau, tau_rows, B, k, lp, ldo, v, ldv, None)
    for kw in (dict(idx=None), dict(sc=None), dict(m=None), dict(s=None), dict(tau=None), dict(lp=None), dict(B=-1),
               dict(tau_rows=0), dict(k=0), dict(k=1025, ldi=2000, ldps=2000, ldo=2000, ldv=2000), dict(P=0),
               dict(ldl=2), dict(ldi=7), dict(ldps=7), dict(ldo=7), dict(ldv=7)):
        assert fin(**kw) == EINVAL and "arx_sample_logp_finish" in _err(lib), kw
    assert fin(B=0) == 0 and fin(B=0, v=None, ldv=0) == 0

    def rest(a=A, lda=64, M=4, b=A, ldb=64, N=300, K=64, bias=A, col_base=0, tau=A, tau_rows=4, keys=None, key_rows=0,
             ptr=None, cols=None, tags=None, wa=None, wl=None, want_rows=0, pc=A, ps=A, ldp=8, k=8, m=A, s=A, ldl=64,
             sc=A, ldps=8):
        return lib.arx_gemm_nt_rest_mass(a, lda, M, b, ldb, N, K, bias, col_base, tau, tau_rows, keys, key_rows, ptr,
                                         cols, tags, wa, wl, want_rows, pc, ps, ldp, k, m, s, ldl, sc, ldps, None)
    for kw in (dict(a=None), dict(b=None), dict(tau=None), dict(pc=None), dict(ps=None), dict(m=None), dict(s=None),
               dict(sc=None), dict(M=-1), dict(N=0), dict(lda=60), dict(ldb=60), dict(tau_rows=0), dict(keys=A),
               dict(keys=A, ptr=A, cols=A, key_rows=0), dict(tags=A), dict(tags=A, wa=A, wl=A, want_rows=0),
               dict(col_base=-1), dict(col_base=2 ** 31 - 100), dict(k=0), dict(k=1025, ldp=2000, ldps=2000),
               dict(ldp=7), dict(ldps=7), dict(a=A + 4), dict(lda=66)):
        assert rest(**kw) == EINVAL and "arx_gemm_nt_rest_mass" in _err(lib), kw
    for K in (16, 48, 256):
        assert rest(K=K, lda=256, ldb=256) == EUNSUPPORTED and "32, 64 or 128" in _err(lib), K
    assert rest(M=0) == 0 and rest(M=0, bias=None) == 0


# ---------------------------------------------------------------- 4. keys and refusals
def test_recommend_key_and_the_refusals():
    from arx.topk import check_return_logprob as chk, excluding_twin, no_return_logprob, recommend_key
    assert recommend_key(False, False, True, True) == 'recommend_sample_logp'
    assert recommend_key(True, True, True, True) == 'recommend_ex_tags_sample_logp'
    assert recommend_key(True, False, True) == 'recommend_ex_sample' and recommend_key(False, True) == 'recommend_tags'
    with pytest.raises(ValueError):
        recommend_key(False, False, False, True)
    with pytest.raises(ValueError, match='sample_temperature'):
        chk(True, True, None)
    with pytest.raises(ValueError, match='recommend'):
        chk(True, False, 1.0)
    assert chk(False, False, None) is None and chk(True, True, 0.5) is None and chk(False, True, None) is None
    with pytest.raises(ValueError):
        excluding_twin(None, object(), exclusion_args=lambda: None, logp=True)
    assert no_return_logprob('x', False) is None
    with pytest.raises(NotImplementedError, match='x: return_logprob'):
        no_return_logprob('x', True)


# ---------------------------------------------------------------- 5. the law, on the oracle's own draws
LAW_SCORES = np.linspace(-1.5, 1.5, 12).astype(np.float32)
LAW_ROWS, LAW_K, LAW_TAU = 4096, 3, 1.0


def test_law_bound_is_the_slate_test_s_quantile():
    from test_slate_sample_cpu import LAW_BOUND
    assert abs(RL.chi2_quantile(29) - LAW_BOUND) < 0.01              # 58.30: the 0.999 quantile at 29 degrees
    assert 270 < RL.chi2_quantile(206) < 276


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_law_statistic_on_the_oracle_s_own_draws(seed):
    """Seeds 0-2 are fair seeds independently of the device: the float64 restatement's own draws, with its own
    log-probabilities, stay under the bound the GPU test holds the device to."""
    L = np.tile(LAW_SCORES, (LAW_ROWS, 1))
    elig = np.ones(L.shape, dtype=bool)
    tau = np.full(LAW_ROWS, LAW_TAU, dtype=np.float32)
    ids = RL.draw(L, elig, tau, seed, LAW_K)
    assert (ids >= 0).all() and all(len(set(r)) == LAW_K for r in ids.tolist())
    lp = RL.logp(L, elig, ids, tau)
    chi2, cells, bound = RL.law_chi2(ids, lp, LAW_SCORES, LAW_TAU)
    print("seed %d: chi2 = %.2f over %d cells, bound %.2f" % (seed, chi2, cells, bound))
    assert cells > 100 and chi2 < bound
