"""Recommend without each user's seen items: the host half (no GPU).

 1. exclusion_csr, the per-user lists of logit columns built from {user: items} dicts or (ptr, items) CSR pairs;
 2. the new C ABI entries refuse bad arguments with ARX_EINVAL and a message before any HIP call.
"""
import time

import numpy as np
import pytest

EINVAL = -1


def _lists(ptr, cols):
    return [cols[ptr[u]:ptr[u + 1]].tolist() for u in range(len(ptr) - 1)]


def _item2logit(n_items):
    """item i -> logit n_items - 1 - i for even items, no logit (-1) for odd ones"""
    m = np.full(n_items + 2, -1, dtype=np.int32)
    ev = np.arange(0, n_items, 2)
    m[ev] = n_items - 1 - ev
    return m


# ---------------------------------------------------------------- 1. host CSR builder
def test_exclusion_csr_from_dict_maps_drops_sorts_dedupes():
    from arx.attributes.embed_attribute import exclusion_csr
    i2l = _item2logit(10)          # 0->9, 2->7, 4->5, 6->3, 8->1; odd items and 10, 11 have no logit
    sets = {0: [4, 0, 2, 0, 4],    # duplicates, unsorted
            1: [1, 3, 5],          # no item has a logit: empty list
            3: {8, 6, 7},          # a set; 7 dropped
            4: [],                 # explicitly empty
            5: [2, -1, 99],        # negative item and one past the map dropped
            9: [0],                # user past the table (n_keys = 6): dropped
            -2: [0]}               # negative user: dropped
    ptr, cols = exclusion_csr(sets, 6, i2l)
    assert ptr.dtype == np.int32 and cols.dtype == np.int32
    assert len(ptr) == 7 and ptr[0] == 0
    assert _lists(ptr, cols) == [[5, 7, 9], [], [], [1, 3], [], [7]]


def test_exclusion_csr_from_csr_pair_matches_dict_form():
    from arx.attributes.embed_attribute import exclusion_csr
    rng = np.random.default_rng(3)
    n_users, n_items = 40, 300
    i2l = _item2logit(n_items)
    sets = {u: rng.integers(0, n_items, rng.integers(0, 25)).tolist() for u in range(n_users) if u % 7}
    ptr_in = np.zeros(n_users + 1, dtype=np.int64)
    for u in range(n_users):
        ptr_in[u + 1] = ptr_in[u] + len(sets.get(u, []))
    items_in = np.concatenate([np.asarray(sets.get(u, []), dtype=np.int64) for u in range(n_users)])
    a = exclusion_csr(sets, n_users + 1, i2l)
    b = exclusion_csr((ptr_in, items_in), n_users + 1, i2l)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    for u, lst in enumerate(_lists(*a)):
        exp = sorted({int(i2l[i]) for i in sets.get(u, []) if i2l[i] >= 0})
        assert lst == exp, u
    assert _lists(*a)[n_users] == []           # a user without a list


def test_exclusion_csr_short_and_long_ptr():
    """A CSR pair shorter than the table leaves the remaining users empty; one longer drops the users past it."""
    from arx.attributes.embed_attribute import exclusion_csr
    i2l = _item2logit(10)
    ptr, cols = exclusion_csr((np.array([0, 2, 3]), np.array([0, 2, 4])), 5, i2l)
    assert _lists(ptr, cols) == [[7, 9], [5], [], [], []]
    ptr, cols = exclusion_csr((np.array([0, 1, 2, 3, 4]), np.array([0, 2, 4, 6])), 2, i2l)
    assert _lists(ptr, cols) == [[9], [7]]
    ptr, cols = exclusion_csr({}, 3, i2l)
    assert ptr.tolist() == [0, 0, 0, 0] and len(cols) >= 1     # (a valid, unused buffer)
    with pytest.raises(ValueError):
        exclusion_csr((np.array([0, 3, 2]), np.array([0, 2, 4])), 3, i2l)
    with pytest.raises(ValueError):
        exclusion_csr([1, 2], 3, i2l)


def test_exclusion_csr_million_users_is_vectorised():
    """1 M users x 20 items in the CSR form: built by sorting, not by a Python loop over users."""
    from arx.attributes.embed_attribute import exclusion_csr
    n_users, per, n_items = 1_000_000, 20, 200_000
    rng = np.random.default_rng(0)
    i2l = np.arange(n_items, dtype=np.int32)[::-1].copy()
    ptr = np.arange(n_users + 1, dtype=np.int64) * per
    items = rng.integers(0, n_items, n_users * per)
    t0 = time.perf_counter()
    p, c = exclusion_csr((ptr, items), n_users + 1, i2l)
    dt = time.perf_counter() - t0
    assert dt < 30.0, dt
    assert len(p) == n_users + 2 and p[-1] == len(c) and len(c) <= n_users * per
    for u in (0, 1, 12345, n_users - 1):
        exp = sorted(set((n_items - 1 - items[u * per:(u + 1) * per]).tolist()))
        assert c[p[u]:p[u + 1]].tolist() == exp


# ---------------------------------------------------------------- 2. the C ABI without a GPU
def _err(lib):
    m = lib.arx_last_error()
    return m.decode() if m else ""


def test_exclude_fill_argument_validation_without_gpu():
    from arx import _lib
    lib = _lib.lib
    P = 256                                   # stands in for a device pointer: only compared with NULL
    f = lib.arx_topk_exclude_fill
    assert f(None, 10, 4, 0, 10, P, 4, P, P, None) == EINVAL
    assert "arx_topk_exclude_fill" in _err(lib)
    assert f(P, 10, 4, 0, 10, None, 4, P, P, None) == EINVAL
    assert f(P, 10, 4, 0, 10, P, 4, None, P, None) == EINVAL
    assert f(P, 10, 4, 0, 10, P, 4, P, None, None) == EINVAL
    assert f(P, 10, 4, 0, 10, P, 0, P, P, None) == EINVAL            # key_rows 0
    assert f(P, 10, -1, 0, 10, P, 4, P, P, None) == EINVAL           # B < 0
    assert f(P, 10, 4, -5, 10, P, 4, P, P, None) == EINVAL           # col0 < 0
    assert f(P, 8, 4, 0, 10, P, 4, P, P, None) == EINVAL             # ld < ncols
    assert "ld < ncols" in _err(lib)
    # nothing to do is not an error (and launches nothing)
    assert f(P, 10, 0, 0, 10, P, 4, P, P, None) == 0
    assert f(P, 10, 4, 0, 0, P, 4, P, P, None) == 0


def test_mark_empty_argument_validation_without_gpu():
    from arx import _lib
    lib = _lib.lib
    P = 256
    f = lib.arx_topk_mark_empty
    assert f(None, 8, P, 8, 4, 8, None) == EINVAL
    assert "arx_topk_mark_empty" in _err(lib)
    assert f(P, 8, None, 8, 4, 8, None) == EINVAL
    assert f(P, 8, P, 8, 4, 0, None) == EINVAL                       # k = 0
    assert f(P, 4, P, 8, 4, 8, None) == EINVAL                       # ldv < k
    assert f(P, 8, P, 8, 0, 8, None) == 0


def test_filter_excl_argument_validation_without_gpu():
    from arx import _lib
    lib = _lib.lib
    P = 256
    f = lib.arx_gemm_nt_topk_filter_excl
    # (host only: the column split needs the CU count, which a GPU-less box does not have -- so only the checks
    # that come before it are exercised here)
    args = dict(A=P, lda=128, M=256, Bm=P, ldb=128, N=100000, K=128, bias=None, thr=P, ldthr=100, col_base=65536,
                cv=P, ci=P, ldc=4096, capp=32, ovf=P, lse=None, ldl=0, keys=P, key_rows=256, ptr=P, cols=P)

    def call(**kw):
        a = dict(args)
        a.update(kw)
        return f(*a.values(), None)
    for k in ("A", "Bm", "thr", "cv", "ci", "ovf"):
        assert call(**{k: None}) == EINVAL, k
        assert "arx_gemm_nt_topk_filter_excl" in _err(lib)
    for k in ("keys", "ptr", "cols"):
        assert call(**{k: None}) == EINVAL, k
        assert "row_keys" in _err(lib)
    assert call(key_rows=0) == EINVAL
    assert call(M=0) == EINVAL and call(N=0) == EINVAL and call(capp=0) == EINVAL
    assert call(col_base=-1) == EINVAL
    assert call(K=96) == EINVAL and "K must be" in _err(lib)
    assert call(A=P + 4) == EINVAL and "aligned" in _err(lib)
