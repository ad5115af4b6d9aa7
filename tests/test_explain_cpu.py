"""explain_items without a GPU: the ABI of include/arx_explain.h against EXPLAIN_PROTOTYPES by type, the argument
validation of arx_explain_slate before any HIP call, the Python checks of arx.explain.explain_items (before any feed,
the plan run patched out) and the float64 oracle of tests/explain_oracle.py against tests/slate_oracle.py."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import explain_oracle as EO      # noqa: E402
import slate_oracle as SO        # noqa: E402

EINVAL, EUNSUPPORTED = -1, -4
NAME = "arx_explain_slate"


def test_header_and_its_table_stay_in_step():
    """include/arx_explain.h against EXPLAIN_PROTOTYPES of arx/_lib.py by TYPE, with the parser and the comparator of
    tests/test_abi_signatures_cpu.py; the name is exported, bound and in no other table; arx.h includes the header
    and PROTOTYPES keeps its size."""
    import test_abi_signatures_cpu as A
    from arx import _lib
    decls = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_explain.h")).read())
    assert sorted(decls) == [NAME]
    lines = open(os.path.join(A.ROOT, "a-recsys_amd", "arx", "_lib.py")).read().split("\n")
    end = next(i for i, l in enumerate(lines) if l.startswith("class ArxError"))
    ns = {"__file__": "_lib.py"}
    exec(compile("\n".join(l for l in lines[:end] if not l.startswith("import torch")), "_lib.py(explain)", "exec"), ns)
    protos = ns["EXPLAIN_PROTOTYPES"]
    assert sorted(protos) == [NAME] == sorted(_lib.EXPLAIN_PROTOTYPES)
    bad = A.mismatches(NAME, decls[NAME], protos[NAME])
    assert not bad, "\n".join(bad)
    # not vacuous: the int T taken for an int64, and a host array of int64 taken for one of int, are reported
    res, args = protos[NAME]
    kc = max(k for k, a in enumerate(args) if a is A.C.c_int)
    wrong = list(args)
    wrong[kc] = A.C.c_int64
    assert A.mismatches(NAME, decls[NAME], (res, wrong))
    kp = next(k for k, a in enumerate(args) if A._is_pointer(a) and a._type_ is A.C.c_int64)
    wrong = list(args)
    wrong[kp] = A.C.POINTER(A.C.c_int)
    assert A.mismatches(NAME, decls[NAME], (res, wrong))
    others = [getattr(_lib, t) for t in dir(_lib) if t.endswith("PROTOTYPES") and t != "EXPLAIN_PROTOTYPES"]
    assert len(others) >= 12 and all(NAME not in t for t in others)
    assert hasattr(_lib.lib, NAME) and getattr(_lib.lib, NAME).argtypes == list(protos[NAME][1])
    assert '#include "arx_explain.h"' in open(os.path.join(A.ROOT, "include", "arx.h")).read()
    assert len(_lib.PROTOTYPES) == A.N_ENTRY_POINTS


def test_export_validates_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib

    def err():
        m = lib.arx_last_error()
        return m.decode() if m else ""
    P = 4096          # (pointers are only compared with NULL and checked for alignment before the first HIP call)
    vp = lambda xs: (C.c_void_p * len(xs))(*xs)

    def go(U=P, ldu=32, B=8, d=32, cand=P, ldc=None, Cc=5, V=100, F=2, kind=(0, 1), E=(P, P), lde=(32, 32),
           fbias=(P, None), cat_map=(None, None), vals=(None, P), starts=(None, P), lens=(None, P), T=3, feat=P, ldf=None,
           bias=P, ldb=None, tv=P, ti=P, tf=P, ldt=None, no_kind=False, no_E=False):
        n = max(F, 1)
        pad = lambda xs, fill: tuple(xs) + (fill,) * (n - len(xs))
        ka = None if no_kind else (C.c_int * n)(*pad(kind, 0)[:n])
        Ea = None if no_E else vp(pad(E, P)[:n])
        la = (C.c_int64 * n)(*pad(lde, lde[0])[:n])
        return lib.arx_explain_slate(U, ldu, B, d, cand, Cc if ldc is None else ldc, Cc, V, F, ka, Ea, la,
                                     vp(pad(fbias, None)[:n]), vp(pad(cat_map, None)[:n]), vp(pad(vals, None)[:n]),
                                     vp(pad(starts, None)[:n]), vp(pad(lens, None)[:n]), T, feat,
                                     Cc * F if ldf is None else ldf, bias, Cc if ldb is None else ldb, tv, ti, tf,
                                     Cc * T if ldt is None else ldt, None)
    invalid = [dict(F=0), dict(F=9), dict(F=-1),                                      # 1 <= F <= 8
               dict(T=17), dict(T=-1),                                                # 0 <= T <= 16
               dict(ldu=34), dict(ldu=28), dict(lde=(32, 34)), dict(lde=(28, 32)),    # not a multiple of 4; below d
               dict(U=None), dict(cand=None), dict(no_kind=True), dict(no_E=True), dict(E=(P, None)),
               dict(U=P + 4), dict(E=(P + 8, P)),                                     # not 16-byte aligned
               dict(tv=None), dict(ti=None), dict(tf=None), dict(tv=None, ti=None),   # tok_* partly NULL
               dict(T=0),                                                             # tok_* given, nothing to keep
               dict(kind=(0, 2)), dict(vals=(None, None)), dict(starts=(None, None)), dict(lens=(None, None)),
               dict(ldc=4), dict(ldf=9), dict(ldb=4), dict(ldt=14),                   # narrower than the outputs
               dict(B=-1), dict(Cc=-1), dict(V=-1), dict(V=1 << 31),
               dict(B=1 << 20, Cc=1 << 11), dict(B=1 << 31, Cc=1)]                    # B * C >= 2^31
    for bad in invalid:
        assert go(**bad) == EINVAL and NAME in err(), bad
    for bad in (dict(d=2, ldu=4, lde=(4, 4)), dict(d=260, ldu=260, lde=(260, 260)), dict(d=30), dict(d=0), dict(d=-4)):
        assert go(**bad) == EUNSUPPORTED and NAME in err() and "d=" in err(), bad
    assert "1 <= F <= 8" in (go(F=9), err())[1] and "0 <= T <= 16" in (go(T=17), err())[1]
    assert "2^31" in (go(B=1 << 20, Cc=1 << 11), err())[1] and "NULL together" in (go(ti=None), err())[1]
    # nothing to do: legal, launches nothing (there is no device here to launch on)
    assert go(B=0) == 0
    assert go(Cc=0) == 0
    assert go(B=0, d=256, ldu=260, lde=(256, 264), F=8, kind=(0,) * 8, T=16) == 0
    assert go(B=0, T=0, tv=None, ti=None, tf=None) == 0
    assert go(B=0, T=5, tv=None, ti=None, tf=None, feat=None, bias=None) == 0


# ---------------------------------------------------------------- the Python checks
def _model(V=50, B=4, pooled=False):
    """What explain_items reads of a model, with a plan whose run would fail: every refusal comes before any feed."""
    from arx import graph as G
    touched = []
    rt = types.SimpleNamespace(nodes=[], device='cpu')
    latent = types.SimpleNamespace(shape=(B, 8))
    pool = types.SimpleNamespace(shape=(V, 8))
    out = object.__new__(G.Node if pooled else G.Prediction)
    out.inputs = (latent, pool)
    model = types.SimpleNamespace(rt=rt, _plans={}, output=out, batch_size=B)
    return model, (lambda: touched.append('feed')), touched


def test_python_checks_come_before_any_feed(monkeypatch):
    from arx import explain, graph as G

    def boom(*a, **k):
        raise AssertionError("a refused call reached the plan")
    monkeypatch.setattr(G.Plan, "__init__", boom)
    monkeypatch.setattr(G.Plan, "run", boom)
    model, feed, touched = _model()
    items = np.zeros((4, 3), dtype=np.int64)
    for bad in (-1, 17, True, 2.5, None, '3'):
        with pytest.raises(ValueError, match="top"):
            explain.explain_items(model, feed, items, bad)
    for bad in (np.zeros(4, dtype=np.int64), np.zeros((3, 3), dtype=np.int64), np.zeros((4, 3)),
                np.full((4, 3), 50), np.full((4, 3), -2), np.zeros((4, 0), dtype=np.int64),
                np.zeros((4, 3), dtype=bool)):
        with pytest.raises(ValueError, match="explain_items"):
            explain.explain_items(model, feed, bad, 3)
    pooled, feed2, touched2 = _model(pooled=True)
    with pytest.raises(NotImplementedError, match="output_feat"):
        explain.explain_items(pooled, feed2, items, 3)
    assert not touched and not touched2 and not model._plans and not model.rt.nodes
    for ok in (0, 1, 16, np.int64(3)):
        assert explain.check_top(ok) == int(ok)
    assert explain.Explanation._fields == ('score', 'feature', 'bias', 'token_value', 'token_id', 'token_feature',
                                           'features')


def test_models_expose_explain_items():
    import inspect
    from arx.hmf.hmf_model import LatentProductModel
    from arx.word2vec.linear_seq import LinearSeq
    assert list(inspect.signature(LatentProductModel.explain_items).parameters) == ['self', 'user_input', 'items', 'top']
    assert list(inspect.signature(LinearSeq.explain_items).parameters) == ['self', 'user_input', 'item_input', 'items',
                                                                           'top']
    for fn in (LatentProductModel.explain_items, LinearSeq.explain_items):
        assert inspect.signature(fn).parameters['top'].default == 3
        assert 'SeqModel' in fn.__doc__ and 'sharded' in fn.__doc__


# ---------------------------------------------------------------- the oracle against itself
@pytest.mark.parametrize("name", ['id', 'mix', 'het', 'ccmm'])
def test_oracle_parts_sum_to_the_slate_score_exactly_on_dyadic_data(name):
    rng = np.random.default_rng(len(name))
    B, C, V, n_tok, d = 4, 9, 40, 30, 8
    feats = EO.layout(rng, name, V, n_tok, d, lambda: rng.choice([1, 2, 4, 8], size=V), dyadic=True)
    U = EO.users(rng, B, d, dyadic=True)
    cand = EO.slate(rng, B, C, V)
    p = EO.parts(U, feats, cand)
    P, b = EO.pooled(feats)
    want = SO.scores(U, P, b, cand)
    dead = np.isneginf(want)
    assert dead.any() and not dead.all()
    np.testing.assert_array_equal(np.where(dead, -np.inf, p['feat'].sum(-1)), want)
    np.testing.assert_array_equal(p['bias'][~dead], b[cand[~dead]])
    assert (p['feat'][dead] == 0).all() and (p['len'][dead] == 0).all()
    # every token contribution of a bag sums to its feature's part, and the order is (value desc, feature, position)
    val, ids, fts, order = EO.top_tokens(p, B, C, 5)
    for (r, j), (v, i, f, pos, _) in p['tok'].items():
        for k, ft in enumerate(feats):
            if ft['kind'] == 'mulhot':
                assert v[f == k].sum() == p['feat'][r, j, k]
        o = order[(r, j)]
        keys = list(zip(-v[o], f[o], pos[o]))
        assert keys == sorted(keys) and len(o) == len(v)
        n = min(5, len(o))
        assert (ids[r, j, :n] == i[o[:n]]).all() and (ids[r, j, n:] == -1).all() and np.isneginf(val[r, j, n:]).all()
    assert (ids[dead] == -1).all() and (fts[dead] == -1).all() and np.isneginf(val[dead]).all()


def test_oracle_keeps_a_nan_out_and_counts_a_repeat_twice():
    E = np.array([[1.0, 0.0], [2.0, 0.0], [np.nan, 0.0]], dtype=np.float32)
    feats = [dict(kind='mulhot', E=E, b=None, vals=np.array([1, 2, 0, 1], dtype=np.int32),
                  starts=np.array([0], dtype=np.int32), lens=np.array([4], dtype=np.int32))]
    p = EO.parts(np.array([[1.0, 0.0]], dtype=np.float32), feats, np.array([[0]]))
    val, ids, fts, _ = EO.top_tokens(p, 1, 1, 4)
    assert ids[0, 0].tolist() == [1, 1, 0, -1] and fts[0, 0].tolist() == [0, 0, 0, -1]
    assert val[0, 0].tolist() == [0.5, 0.5, 0.25, -np.inf]
