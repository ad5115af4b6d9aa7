"""The host half of the hardest-of-C negative draw (arx_neg_draw_hardest, include/arx_neg_hard.h) without a GPU: the
export's argument validation before any HIP call, the header against NEG_HARD_PROTOTYPES by type, and the refusals of
prepare_pair_negatives(hardest_of=) that need no launch."""
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

EINVAL, EUNSUPPORTED = -1, -4


def test_hardest_export_validates_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib

    def err():
        m = lib.arx_last_error()
        return m.decode() if m else ""
    P = 4096          # (pointers are only compared with NULL and checked for alignment before the first HIP call)

    def draw(users=P, B=8, n_users=4, ptr=P, cols=P, ex_cum=None, cum=None, V=100, C=8, U=P, ldu=32, n_urows=10,
             umap=None, n_umap=0, Pt=P, ldp=32, n_prows=100, d=32, out=P, cand=None, ldc=0, score=None, lds=0):
        return lib.arx_neg_draw_hardest(users, B, n_users, ptr, cols, ex_cum, cum, V, None, 0, None, 0, C, U, ldu,
                                        n_urows, umap, n_umap, Pt, ldp, n_prows, None, None, d, out, None, None, cand,
                                        ldc, score, lds, None)
    invalid = [dict(C=1), dict(C=0), dict(C=65), dict(C=-2),                           # C out of range
               dict(cum=P), dict(ex_cum=P),                                            # one weight table without the other
               dict(users=None), dict(ptr=None), dict(cols=None), dict(U=None), dict(Pt=None), dict(out=None),
               dict(ldu=28), dict(ldu=34), dict(ldp=28), dict(ldp=38),                 # below d; not a multiple of 4
               dict(U=P + 4), dict(Pt=P + 8),                                          # not 16-byte aligned
               dict(cand=P, ldc=7), dict(score=P, lds=7),                              # diagnostics narrower than C
               dict(B=-1), dict(n_users=-1), dict(n_umap=-1), dict(n_urows=-1), dict(n_prows=1 << 31),
               dict(V=0), dict(V=1 << 31)]
    for bad in invalid:
        assert draw(**bad) == EINVAL and "arx_neg_draw_hardest" in err(), bad
    for bad in (dict(d=30, ldu=32), dict(d=0), dict(d=2), dict(d=260, ldu=260, ldp=260), dict(d=-4)):
        assert draw(**bad) == EUNSUPPORTED and "arx_neg_draw_hardest" in err() and "d=" in err(), bad
    assert "2 <= C <= 64" in (draw(C=65), err())[1]
    # nothing to do: legal, launches nothing (there is no device here to launch on)
    assert draw(B=0) == 0
    assert draw(B=0, cum=P, ex_cum=P, cand=P, ldc=64, score=P, lds=68, C=64, d=256, ldu=256, ldp=260) == 0


def test_header_and_its_table_stay_in_step():
    """include/arx_neg_hard.h against NEG_HARD_PROTOTYPES of arx/_lib.py by TYPE, with the parser and the comparator of
    tests/test_abi_signatures_cpu.py; the name is exported and bound, arx.h includes the header, PROTOTYPES keeps its
    size."""
    import test_abi_signatures_cpu as A
    from arx import _lib
    decls = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_neg_hard.h")).read())
    names = ["arx_neg_draw_hardest"]
    assert sorted(decls) == names
    lines = open(os.path.join(A.ROOT, "a-recsys_amd", "arx", "_lib.py")).read().split("\n")
    end = next(i for i, l in enumerate(lines) if l.startswith("class ArxError"))
    ns = {"__file__": "_lib.py"}
    exec(compile("\n".join(l for l in lines[:end] if not l.startswith("import torch")), "_lib.py(hard)", "exec"), ns)
    protos = ns["NEG_HARD_PROTOTYPES"]
    assert sorted(protos) == names == sorted(_lib.NEG_HARD_PROTOTYPES)
    bad = [m for name in names for m in A.mismatches(name, decls[name], protos[name])]
    assert not bad, "\n".join(bad)
    # not vacuous: the int C taken for an int64 is reported
    res, args = protos[names[0]]
    kc = next(k for k, a in enumerate(args) if a is A.C.c_int)
    wrong = list(args)
    wrong[kc] = A.C.c_int64
    assert A.mismatches(names[0], decls[names[0]], (res, wrong))
    assert hasattr(_lib.lib, names[0]) and names[0] not in _lib.PROTOTYPES
    assert getattr(_lib.lib, names[0]).argtypes == list(protos[names[0]][1])
    assert '#include "arx_neg_hard.h"' in open(os.path.join(A.ROOT, "include", "arx.h")).read()
    assert len(_lib.PROTOTYPES) == A.N_ENTRY_POINTS


def _att(user_kinds, item_kinds):
    """What check_hardest_of reads of an EmbeddingAttribute: the kinds of the two feature lists."""
    from arx.attributes.embed_attribute import EmbeddingAttribute
    feats = lambda kinds: [types.SimpleNamespace(kind=k) for k in kinds]
    att = types.SimpleNamespace(user_feats=feats(user_kinds), item_feats=feats(item_kinds))
    att.check_hardest_of = types.MethodType(EmbeddingAttribute.check_hardest_of, att)
    return att


def test_hardest_of_refusals_need_no_device():
    att = _att(['cat'], ['cat'])
    for ok in (None, 2, 8, 64):
        att.check_hardest_of(ok)
    for bad in (1, 65, 2.5, 0, -3, True, '8', 8.0):
        with pytest.raises(ValueError, match='hardest_of'):
            att.check_hardest_of(bad)
    for users, items, side in ((['cat'], ['cat', 'mulhot'], 'item side'), (['cat'], ['mulhot'], 'item side'),
                               (['cat', 'cat'], ['cat'], 'user side'), (['mulhot'], ['cat'], 'user side'),
                               ([], ['cat'], 'user side')):
        with pytest.raises(NotImplementedError, match=side):
            _att(users, items).check_hardest_of(8)
        _att(users, items).check_hardest_of(None)                 # (without the argument nothing is refused)


def test_model_refuses_before_it_drops_its_plans():
    """LatentProductModel.prepare_pair_negatives raises before it touches the drawing plans or the attribute."""
    from arx.hmf.hmf_model import LatentProductModel

    def model(nonlinear, att, loss='bpr'):
        touched = []
        att.prepare_pair_negatives = lambda *a, **k: touched.append(k)
        return types.SimpleNamespace(loss_function=loss, nonlinear=nonlinear, att_emb=att,
                                     _plans={'train_draw': 1, 'eval_draw': 2}), touched
    prepare = LatentProductModel.prepare_pair_negatives
    for nl in ('relu', 'tanh'):
        mdl, touched = model(nl, _att(['cat'], ['cat']))
        with pytest.raises(NotImplementedError, match=nl):
            prepare(mdl, {}, hardest_of=8)
        assert mdl._plans == {'train_draw': 1, 'eval_draw': 2} and not touched
        prepare(mdl, {}, seed=2)                                  # the plain draw of an MLP model is as before
        assert not mdl._plans and touched[0]['hardest_of'] is None and touched[0]['seed'] == 2
    mdl, touched = model('linear', _att(['cat'], ['cat', 'mulhot']))
    with pytest.raises(NotImplementedError, match='item side'):
        prepare(mdl, {}, hardest_of=8)
    for bad in (1, 65, 2.5):
        with pytest.raises(ValueError, match='hardest_of'):
            prepare(mdl, {}, hardest_of=bad)
    assert mdl._plans == {'train_draw': 1, 'eval_draw': 2} and not touched
    mdl, touched = model('linear', _att(['cat'], ['cat']))
    prepare(mdl, {}, seed=5, hardest_of=16)
    assert not mdl._plans and touched[0]['hardest_of'] == 16
