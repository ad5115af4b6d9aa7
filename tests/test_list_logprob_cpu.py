"""list_logprob without a GPU: the float64 oracle (tests/list_logprob_oracle.py) against brute force, the ABI of
include/arx_list_logp.h against LIST_LOGP_PROTOTYPES by type, argument validation of the two entries before any HIP
call, arx.utils.ope on hand-made numbers, and the host-side checks of the public call (arx.topk)."""
import itertools
import os

import numpy as np
import pytest

import list_logprob_oracle as LL

NAMES = ["arx_list_logp_prepare", "arx_list_logp_stamp"]
EINVAL = -1


# ---------------------------------------------------------------- 1. the oracle against brute force
def _brute(scores, elig, triple, tau):
    """the probability that sequential softmax draws over the eligible columns give exactly `triple`, or 0"""
    left = set(int(c) for c in np.nonzero(elig)[0])
    p = 1.0
    for c in triple:
        if c not in left:
            return 0.0
        w = {j: np.exp(np.float64(scores[j]) / tau) for j in left}
        p *= w[c] / sum(w.values())
        left.discard(c)
    return p


def test_oracle_against_brute_force_v6_k3():
    V, k = 6, 3
    L = np.array([[0.3, -1.2, 2.0, 0.7, -0.4, 1.1]], dtype=np.float32)
    tags = np.array([1, 1, 1, 1, 2, 1], dtype=np.uint32)             # column 4 fails want_any = 1
    wa, wl = np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint32)
    ex = [[1]]
    elig = np.array([True, False, True, True, False, True])
    for tau in (0.3, 1.0, 4.0):
        total = 0.0
        for triple in itertools.product(range(V), repeat=k):          # every ordered triple, impossible ones included
            lp, codes, _ = LL.logp(L, np.array([triple]), np.array([tau]), tags, wa, wl, ex)
            exact = _brute(L[0], elig, triple, tau)
            got = float(np.exp(lp.sum()))
            assert abs(got - exact) <= 1e-12, (tau, triple, got, exact)
            assert (exact == 0) == (codes >= LL.RANGE).any()
            total += got
        assert abs(total - 1) <= 1e-12, (tau, total)


def test_oracle_codes_and_absent_entries():
    L = np.array([[0.3, -1.2, 2.0, 0.7, -np.inf, 1.1]], dtype=np.float32)
    tags = np.array([1, 1, 1, 2, 1, 1], dtype=np.uint32)             # column 3 fails want_any = 1
    wa, wl = np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint32)
    lists = np.array([[2, -1, -7, 6, 1, 3, 2, 4, 4, 0, 2 ** 31 - 1, 1]])
    lp, codes, tol = LL.logp(L, lists, np.array([0.5]), tags, wa, wl, [[1]])
    assert codes.tolist() == [[0, 1, 2, 2, 3, 4, 5, 6, 5, 0, 2, 3]]
    assert lp[0, 1] == 0 and np.isneginf(lp[0, [2, 3, 4, 5, 6, 7, 8, 10, 11]]).all() and np.isfinite(lp[0, [0, 9]]).all()
    assert (tol[0, [0, 9]] > 0).all() and (tol[0, [1, 2, 3]] == 0).all()
    # the non-drawable entries are ABSENT: the drawable ones read as the list [2, 0] alone does
    alone, _, _ = LL.logp(L, np.array([[2, 0]]), np.array([0.5]), tags, wa, wl, [[1]])
    np.testing.assert_array_equal(lp[0, [0, 9]], alone[0])
    # REST empty: eligible are {0, 2, 5}; the last drawable entry is certain
    full, codes, _ = LL.logp(L, np.array([[5, 0, -1, 2]]), np.array([2.0]), tags, wa, wl, [[1]])
    assert codes.tolist() == [[0, 0, 1, 0]] and full[0, 3] == 0 and full[0, 2] == 0 and (full[0, :2] < 0).all()


# ---------------------------------------------------------------- 2. the ABI
def test_list_logp_header_and_its_table_stay_in_step():
    import test_abi_signatures_cpu as A
    from arx import _lib
    decls = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_list_logp.h")).read())
    assert sorted(decls) == NAMES
    protos = _lib.LIST_LOGP_PROTOTYPES
    assert sorted(protos) == NAMES
    bad = [m for name in NAMES for m in A.mismatches(name, decls[name], protos[name])]
    assert not bad, "\n".join(bad)
    others = [getattr(_lib, t) for t in dir(_lib) if t.endswith("PROTOTYPES") and t != "LIST_LOGP_PROTOTYPES"]
    assert len(others) >= 8 and _lib.PROTOTYPES in others
    for name in NAMES:                                               # not vacuous: one i64 narrowed to i32 is reported
        res, args = protos[name]
        k64 = next(k for k, a in enumerate(args) if a is A.C.c_int64)
        narrowed = list(args)
        narrowed[k64] = A.C.c_int32
        assert any("parameter %d " % k64 in m for m in A.mismatches(name, decls[name], (res, narrowed)))
        assert hasattr(_lib.lib, name) and getattr(_lib.lib, name).argtypes == list(args)
        assert all(name not in t for t in others)
    assert len(_lib.PROTOTYPES) == A.N_ENTRY_POINTS
    arx_h = open(os.path.join(A.ROOT, "include", "arx.h")).read()
    assert '#include "arx_list_logp.h"' in arx_h
    codes = dict(OK=0, EMPTY=1, RANGE=2, EXCLUDED=3, TAGS=4, REPEAT=5, NOSCORE=6)
    text = open(os.path.join(A.ROOT, "include", "arx_list_logp.h")).read()
    for name, code in codes.items():                                 # the reason codes are part of the ABI
        assert "#define ARX_LIST_%s %d " % (name, code) in text and getattr(LL, name) == code


# ---------------------------------------------------------------- 3. argument validation
def _err(lib):
    m = lib.arx_last_error()
    return m.decode() if m else ""


def test_entries_validate_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib
    A = 4096                                  # stands in for a device pointer: only compared with NULL

    def prep(ls=A, ldl=8, B=4, k=8, V=100, keys=None, key_rows=0, ptr=None, cols=None, tags=None, wa=None, wl=None,
             want_rows=0, cl=A, ldc=8, why=A, ldw=8, pc=A, ps=A, ldp=8):
        return lib.arx_list_logp_prepare(ls, ldl, B, k, V, keys, key_rows, ptr, cols, tags, wa, wl, want_rows, cl, ldc,
                                         why, ldw, pc, ps, ldp, None)
    wide = dict(ldl=2000, ldc=2000, ldw=2000, ldp=2000)
    for kw, text in ((dict(ls=None), "null"), (dict(cl=None), "null"), (dict(why=None), "null"), (dict(pc=None), "null"),
                     (dict(ps=None), "null"), (dict(B=-1), "B >= 0"), (dict(k=0), "1 <= k <= 1024"),
                     (dict(k=1025, **wide), "1 <= k <= 1024"), (dict(ldl=7), ">= k"), (dict(ldc=7), ">= k"),
                     (dict(ldw=7), ">= k"), (dict(ldp=7), ">= k"), (dict(V=0), "0 < V"), (dict(V=-5), "0 < V"),
                     (dict(V=2 ** 31), "0 < V"), (dict(keys=A), "go together"), (dict(ptr=A, cols=A), "go together"),
                     (dict(keys=A, ptr=A, cols=A, key_rows=0), "key_rows > 0"), (dict(tags=A), "go together"),
                     (dict(wa=A, wl=A), "go together"), (dict(tags=A, wa=A, wl=A, want_rows=0), "want_rows > 0")):
        assert prep(**kw) == EINVAL, kw
        assert "arx_list_logp_prepare" in _err(lib) and text in _err(lib), (kw, _err(lib))
    assert prep(B=0) == 0 and prep(B=0, k=1024, **wide) == 0
    assert prep(B=0, keys=A, ptr=A, cols=A, key_rows=4, tags=A, wa=A, wl=A, want_rows=4) == 0

    def stamp(cl=A, ldc=8, sc=A, ldps=8, B=4, k=8, why=A, ldw=8, lp=A, ldo=8, v=A, ldv=8):
        return lib.arx_list_logp_stamp(cl, ldc, sc, ldps, B, k, why, ldw, lp, ldo, v, ldv, None)
    for kw, text in ((dict(cl=None), "null"), (dict(sc=None), "null"), (dict(why=None), "null"), (dict(lp=None), "null"),
                     (dict(B=-1), "B >= 0"), (dict(k=0), "1 <= k <= 1024"),
                     (dict(k=1025, ldc=2000, ldps=2000, ldw=2000, ldo=2000, ldv=2000), "1 <= k <= 1024"),
                     (dict(ldc=7), ">= k"), (dict(ldps=7), ">= k"), (dict(ldw=7), ">= k"), (dict(ldo=7), ">= k"),
                     (dict(ldv=7), ">= k")):
        assert stamp(**kw) == EINVAL, kw
        assert "arx_list_logp_stamp" in _err(lib) and text in _err(lib), (kw, _err(lib))
    assert stamp(B=0) == 0 and stamp(B=0, v=None, ldv=0) == 0


# ---------------------------------------------------------------- 4. arx.utils.ope
def test_ope_on_hand_made_numbers():
    from arx.utils.ope import ips, list_weights, snips
    ninf = -np.inf
    target = np.log(np.array([[0.5, 0.5], [0.25, 1.0], [1.0, 1.0], [0.5, 1.0]]))
    target[2, 1] = ninf                                              # the target policy cannot produce list 2
    logged = np.log(np.array([[0.25, 0.5], [0.5, 1.0], [0.5, 0.5], [0.5, 1.0]]))
    w = list_weights(target, logged)
    assert w.dtype == np.float64
    np.testing.assert_allclose(w, [2.0, 0.5, 0.0, 1.0], rtol=1e-15)
    assert w[2] == 0 and w[3] == 1.0
    np.testing.assert_array_equal(list_weights(target, logged, clip=1.5), [1.5, 0.5, 0.0, 1.0])
    z = np.zeros((3, 2), dtype=np.float32)
    assert (list_weights(z, z) == 1.0).all()                          # an EMPTY entry (logp 0) on both sides
    bad = logged.copy()
    bad[1, 0] = ninf
    with pytest.raises(ValueError, match="row 1"):
        list_weights(target, bad)
    with pytest.raises(ValueError):
        list_weights(target, logged[:3])
    with pytest.raises(ValueError):
        list_weights(np.full((1, 2), np.nan), np.zeros((1, 2)))
    rewards = np.array([1.0, 0.0, 1.0, 2.0])
    assert ips(rewards, w) == pytest.approx((2.0 + 0 + 0 + 2.0) / 4)
    assert snips(rewards, w) == pytest.approx((2.0 + 2.0) / 3.5)
    with pytest.raises(ValueError):
        snips(rewards, np.zeros(4))


# ---------------------------------------------------------------- 5. the host-side checks of the public call
def test_keys_lists_and_temperatures():
    import torch
    from arx.topk import check_lists, list_logp_key, list_taus
    assert [list_logp_key(e, t) for e in (False, True) for t in (False, True)] == \
        ['list_logp', 'list_logp_tags', 'list_logp_ex', 'list_logp_ex_tags']
    a, k = check_lists([[1, -1, 2 ** 40], [-2 ** 40, 0, 7]], 2)
    assert k == 3 and a.dtype == np.int32 and a.tolist() == [[1, -1, 2 ** 31 - 1], [-2 ** 31, 0, 7]]
    a, k = check_lists(np.arange(8, dtype=np.int64).reshape(2, 4), 2)
    assert k == 4 and a.dtype == np.int32 and a.flags['C_CONTIGUOUS']
    t, k = check_lists(torch.tensor([[5, 2 ** 33], [-1, -2 ** 33]], dtype=torch.int64), 2)
    assert k == 2 and t.dtype == torch.int32 and t.tolist() == [[5, 2 ** 31 - 1], [-1, -2 ** 31]]
    for bad in (np.zeros((3, 4), dtype=np.int32), np.zeros((2, 0), dtype=np.int32), np.zeros((2, 1025), dtype=np.int32),
                np.zeros(2, dtype=np.int32), np.zeros((2, 2)), np.zeros((2, 2), dtype=bool), torch.zeros((2, 2)),
                torch.zeros((2, 1025), dtype=torch.int32)):
        with pytest.raises(ValueError):
            check_lists(bad, 2)
    assert check_lists(np.zeros((2, 1024), dtype=np.int32), 2)[1] == 1024
    tau = list_taus(0.5, 3)
    assert tau.dtype == np.float32 and tau.tolist() == [0.5, 0.5, 0.5]
    assert list_taus([1, 2.5, 1e-30], 3).shape == (3,)
    with pytest.raises(ValueError, match="row 1 "):
        list_taus([1.0, 0.0, 0.0], 3)
    with pytest.raises(ValueError, match="row 0 "):
        list_taus(0, 3)
    with pytest.raises(ValueError, match="row 2 "):
        list_taus([1.0, 1.0, 1e-60], 3)                               # 0 as float32
    for bad in (-1.0, float('nan'), float('inf'), [1.0, 2.0], True, 'x', None):
        with pytest.raises(ValueError):
            list_taus(bad, 3)
