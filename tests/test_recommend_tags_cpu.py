"""Recommend within item tags: the host half (no GPU).

 1. the two new C ABI entries refuse bad arguments with ARX_EINVAL and a message before any HIP call;
 2. item_tag_words, the per-column tag words built from an array or a {item: bit numbers} dict, and topk.tag_words,
    the per-row request words;
 3. the numpy oracle of tests/tags_oracle.py against a per-row brute-force loop, ties included.
"""
import numpy as np
import pytest

import tags_oracle as T

EINVAL = -1


def _err(lib):
    m = lib.arx_last_error()
    return m.decode() if m else ""


# ---------------------------------------------------------------- 1. the C ABI without a GPU
def test_tags_fill_argument_validation_without_gpu():
    from arx import _lib
    lib = _lib.lib
    P = 256                                   # stands in for a device pointer: only compared with NULL
    f = lib.arx_topk_tags_fill
    #        logits ld  M  col0 ncols tags any all want_rows stream
    assert f(None, 10, 4, 0, 10, P, P, P, 4, None) == EINVAL
    assert "arx_topk_tags_fill" in _err(lib)
    assert f(P, 10, 4, 0, 10, None, P, P, 4, None) == EINVAL
    assert f(P, 10, 4, 0, 10, P, None, P, 4, None) == EINVAL
    assert f(P, 10, 4, 0, 10, P, P, None, 4, None) == EINVAL
    assert f(P, 10, 4, 0, 10, P, P, P, 0, None) == EINVAL             # want_rows 0
    assert "want_rows" in _err(lib)
    assert f(P, 10, -1, 0, 10, P, P, P, 4, None) == EINVAL            # M < 0
    assert f(P, 10, 4, -5, 10, P, P, P, 4, None) == EINVAL            # col0 < 0
    assert f(P, 10, 4, 0, -1, P, P, P, 4, None) == EINVAL             # ncols < 0
    assert f(P, 8, 4, 0, 10, P, P, P, 4, None) == EINVAL              # ld < ncols
    assert "ld < ncols" in _err(lib)
    assert f(P, 2 ** 31, 4, 2 ** 31 - 5, 10, P, P, P, 4, None) == EINVAL     # col0 + ncols past 2^31
    assert "2^31" in _err(lib)
    # nothing to do is not an error (and launches nothing)
    assert f(P, 10, 0, 0, 10, P, P, P, 4, None) == 0
    assert f(P, 10, 4, 1500, 0, P, P, P, 4, None) == 0


def test_filter_tags_argument_validation_without_gpu():
    from arx import _lib
    lib = _lib.lib
    P = 256
    f = lib.arx_gemm_nt_topk_filter_tags
    # (host only: the column split needs the CU count, which a GPU-less box does not have -- so only the checks
    # that come before it are exercised here)
    args = dict(A=P, lda=128, M=256, Bm=P, ldb=128, N=100000, K=128, bias=None, thr=P, ldthr=100, col_base=65536,
                cv=P, ci=P, ldc=4096, capp=32, ovf=P, lse=None, ldl=0, keys=P, key_rows=256, ptr=P, cols=P,
                tags=P, any=P, all=P, want_rows=256)

    def call(**kw):
        a = dict(args)
        a.update(kw)
        return f(*a.values(), None)
    for k in ("A", "Bm", "thr", "cv", "ci", "ovf"):
        assert call(**{k: None}) == EINVAL, k
        assert "arx_gemm_nt_topk_filter_tags" in _err(lib)
    for k in ("tags", "any", "all"):
        assert call(**{k: None}) == EINVAL, k
        assert "col_tags" in _err(lib)
    assert call(want_rows=0) == EINVAL and "want_rows" in _err(lib)
    # the exclusion lists are optional, but only all together
    for k in ("keys", "ptr", "cols"):
        assert call(**{k: None}) == EINVAL, k
        assert "row_keys" in _err(lib)
    assert call(key_rows=0) == EINVAL
    assert call(M=0) == EINVAL and call(N=0) == EINVAL and call(capp=0) == EINVAL and call(ldc=0) == EINVAL
    assert call(lda=64) == EINVAL                                   # lda < K
    assert call(col_base=-1) == EINVAL
    assert call(col_base=2 ** 31 - 50) == EINVAL and "2^31" in _err(lib)
    assert call(K=96) == EINVAL and "K must be" in _err(lib)
    assert call(A=P + 4) == EINVAL and "aligned" in _err(lib)
    assert call(ldb=130) == EINVAL and "aligned" in _err(lib)


def test_tags_header_and_its_table_stay_in_step():
    """include/arx_tags.h against TAGS_PROTOTYPES of arx/_lib.py by TYPE, with the parser and the comparator of
    tests/test_abi_signatures_cpu.py (which does the same for arx.h and PROTOTYPES); the two names are exported by
    the library, arx.h includes the header, and neither table holds a name of the other."""
    import os
    import test_abi_signatures_cpu as A
    from arx import _lib
    decls = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_tags.h")).read())
    assert sorted(decls) == ["arx_gemm_nt_topk_filter_tags", "arx_topk_tags_fill"]
    # the table as the signature test reads it: the source up to `class ArxError`, without torch
    lines = open(os.path.join(A.ROOT, "a-recsys_amd", "arx", "_lib.py")).read().split("\n")
    end = next(i for i, l in enumerate(lines) if l.startswith("class ArxError"))
    ns = {"__file__": "_lib.py"}
    exec(compile("\n".join(l for l in lines[:end] if not l.startswith("import torch")), "_lib.py(tags)", "exec"), ns)
    protos = ns["TAGS_PROTOTYPES"]
    assert sorted(protos) == sorted(decls) == sorted(_lib.TAGS_PROTOTYPES)
    bad = [m for name in sorted(decls) for m in A.mismatches(name, decls[name], protos[name])]
    assert not bad, "\n".join(bad)
    # not vacuous: one i64 narrowed to i32 is reported
    res, args = protos["arx_topk_tags_fill"]
    k64 = next(k for k, a in enumerate(args) if a is A.C.c_int64)
    narrowed = list(args)
    narrowed[k64] = A.C.c_int32
    assert A.mismatches("arx_topk_tags_fill", decls["arx_topk_tags_fill"], (res, narrowed))
    for name in decls:
        assert hasattr(_lib.lib, name) and name not in _lib.PROTOTYPES
        assert getattr(_lib.lib, name).argtypes == list(protos[name][1])
    assert '#include "arx_tags.h"' in open(os.path.join(A.ROOT, "include", "arx.h")).read()


# ---------------------------------------------------------------- 2. host logic
def _item2logit(n_items):
    """item i -> logit n_items - 1 - i for even items, no logit (-1) for odd ones"""
    m = np.full(n_items + 2, -1, dtype=np.int32)
    ev = np.arange(0, n_items, 2)
    m[ev] = n_items - 1 - ev
    return m


def test_item_tag_words_array_and_dict_forms():
    from arx.attributes.embed_attribute import item_tag_words
    i2l = _item2logit(10)          # 0->9, 2->7, 4->5, 6->3, 8->1; odd items have no logit
    arr = np.array([1, 2, 2 ** 31, 8, 2 ** 32 - 1, 32, 0, 128, 5, 512], dtype=np.uint64)
    w = item_tag_words(arr, i2l, 10)
    assert w.dtype == np.int32 and w.shape == (10,)
    u = w.view(np.uint32)
    exp = np.zeros(10, dtype=np.uint32)
    exp[9], exp[7], exp[5], exp[3], exp[1] = 1, 2 ** 31, 2 ** 32 - 1, 0, 5
    np.testing.assert_array_equal(u, exp)              # columns 0, 2, 4, 6, 8 have no item: 0
    # the dict form: bit numbers; items without a logit and items past the map are skipped
    d = {0: [0], 2: [31], 4: range(32), 8: (0, 2), 3: [4], 99: [1], 6: []}
    np.testing.assert_array_equal(item_tag_words(d, i2l, 10).view(np.uint32), exp)
    # a shorter array: the items past it have no tags
    np.testing.assert_array_equal(item_tag_words(arr[:3], i2l, 10).view(np.uint32)[[9, 7, 5]], [1, 2 ** 31, 0])
    # signed input of the same values
    np.testing.assert_array_equal(item_tag_words(arr.astype(np.int64), i2l, 10), w)


def test_item_tag_words_range_errors():
    from arx.attributes.embed_attribute import item_tag_words
    i2l = _item2logit(10)
    for bad in (np.array([0, -1]), np.array([2 ** 32], dtype=np.int64), np.array([0.5, 1.0]),
                np.zeros((2, 2), dtype=np.int64), np.array([True, False])):
        with pytest.raises(ValueError):
            item_tag_words(bad, i2l, 10)
    for bad in ({0: [32]}, {0: [-1]}, {0: [1.0]}, {-1: [1]}, {0: [True]}):
        with pytest.raises(ValueError):
            item_tag_words(bad, i2l, 10)


def test_request_words_forms_and_errors():
    from arx.topk import recommend_key, tag_words
    a, l = tag_words(5, None, 4)
    assert a.dtype == np.int32 and a.tolist() == [5] * 4 and l.tolist() == [0] * 4
    a, l = tag_words(None, [1, 2 ** 31, 2 ** 32 - 1, 0], 4)
    assert a.tolist() == [0] * 4
    np.testing.assert_array_equal(l.view(np.uint32), np.array([1, 2 ** 31, 2 ** 32 - 1, 0], dtype=np.uint32))
    a, _ = tag_words(np.arange(4, dtype=np.uint32), 0, 4)
    assert a.tolist() == [0, 1, 2, 3]
    for bad in ((-1, None), (None, 2 ** 32), ([1, 2, 3], None), (None, [1] * 5), (1.5, None), ([0.0] * 4, None),
                (np.zeros((4, 1), dtype=np.int64), None), ([1, 2, 3, -4], 0), (True, None)):
        with pytest.raises(ValueError):
            tag_words(bad[0], bad[1], 4)
    assert [recommend_key(e, t) for e in (False, True) for t in (False, True)] == \
        ['recommend', 'recommend_tags', 'recommend_ex', 'recommend_ex_tags']


# ---------------------------------------------------------------- 3. the oracle against brute force
def test_oracle_equals_brute_force_with_ties():
    rng = np.random.default_rng(0)
    B, V, k = 6, 40, 12
    x = rng.integers(-3, 4, size=(B, V)).astype(np.float32)           # few distinct values: ties everywhere
    x[2, 5] = -np.inf                                                 # an item switched off by its bias
    tags = rng.integers(0, 16, V).astype(np.uint32)
    tags[7] = 2 ** 31 + 1
    want_any = np.array([0, 3, 0, 4, 2 ** 31, 8], dtype=np.uint32)
    want_all = np.array([0, 0, 5, 1, 1, 7], dtype=np.uint32)          # row 5: (8 any, 7 all) -> only tag 15
    ex = [rng.choice(V, 10, replace=False) for _ in range(B)]
    ex[0] = np.zeros(0, dtype=np.int64)
    for lists in (None, ex):
        ev, ei = T.topk(x, k, tags, want_any, want_all, lists)
        bv, bi = T.brute_topk(x, k, tags, want_any, want_all, lists)
        np.testing.assert_array_equal(ei, bi)
        np.testing.assert_array_equal(ev, bv)
    # row 0 of the unexcluded case has no constraint: the plain top-k
    ev, ei = T.topk(x, k, tags, want_any, want_all, None)
    pv, pi = T.topk(x, k)
    np.testing.assert_array_equal(ei[0], pi[0])
    # the eligibility rule itself, spelled out
    el = T.eligible(tags, want_any, want_all)
    assert el[0].all()
    assert el[4].tolist() == [bool(t & 2 ** 31) and bool(t & 1) for t in tags.tolist()] and el[4, 7]
    assert (ei[el.sum(1) < k] == -1).any()                            # a short row ends in -1
    for r in range(B):
        got = ei[r][ei[r] >= 0]
        assert el[r, got].all()
