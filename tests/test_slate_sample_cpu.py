"""score_items(sample_temperature=) without a GPU: the ABI of include/arx_slate_sample.h against SLATE_SAMPLE_PROTOTYPES
by type, argument validation of arx_slate_sample before any HIP call, the predicate on both sides of its edges, the
host rules of arx.slate.score_items (every refusal comes before any feed; the draw counter moves only on an accepted
sample_seed=None call) and the self-checks of the float64 oracle of tests/slate_sample_oracle.py."""
import itertools
import os
import types

import numpy as np
import pytest

import slate_sample_oracle as SS

NAMES = ["arx_slate_sample", "arx_slate_sample_supported"]
EINVAL, EUNSUPPORTED = -1, -4


# ---------------------------------------------------------------- 1. the ABI
def test_slate_sample_header_and_its_table_stay_in_step():
    import test_abi_signatures_cpu as A
    from arx import _lib
    decls = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_slate_sample.h")).read())
    assert sorted(decls) == NAMES
    lines = open(os.path.join(A.ROOT, "a-recsys_amd", "arx", "_lib.py")).read().split("\n")
    end = next(i for i, l in enumerate(lines) if l.startswith("class ArxError"))
    ns = {"__file__": "_lib.py"}
    exec(compile("\n".join(l for l in lines[:end] if not l.startswith("import torch")), "_lib.py(slate_sample)",
                 "exec"), ns)
    protos = ns["SLATE_SAMPLE_PROTOTYPES"]
    assert sorted(protos) == sorted(decls) == sorted(_lib.SLATE_SAMPLE_PROTOTYPES)
    bad = [m for name in sorted(decls) for m in A.mismatches(name, decls[name], protos[name])]
    assert not bad, "\n".join(bad)
    for name in NAMES:                                            # not vacuous: one i64 narrowed to i32 is reported
        res, args = protos[name]
        k64 = next(k for k, a in enumerate(args) if a is A.C.c_int64)
        narrowed = list(args)
        narrowed[k64] = A.C.c_int32
        assert any("parameter %d " % k64 in m for m in A.mismatches(name, decls[name], (res, narrowed)))
    for name in decls:
        assert hasattr(_lib.lib, name)
        assert all(name not in t for t in (_lib.PROTOTYPES, _lib.TAGS_PROTOTYPES, _lib.SLATE_PROTOTYPES,
                                           _lib.DIVERSE_PROTOTYPES, _lib.SAMPLE_PROTOTYPES))
        assert getattr(_lib.lib, name).argtypes == list(protos[name][1])
    assert "arx_slate_sample_supported" in _lib._NO_CHECK and "arx_slate_sample" not in _lib._NO_CHECK
    assert '#include "arx_slate_sample.h"' in open(os.path.join(A.ROOT, "include", "arx.h")).read()
    assert len(A.load_prototypes()) == A.N_ENTRY_POINTS == 146


# ---------------------------------------------------------------- 2. argument validation
def test_slate_sample_validates_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib

    def err():
        m = lib.arx_last_error()
        return m.decode() if m else ""
    A = 4096                                  # stands in for a device pointer: only compared with NULL

    def ss(cand=A, ldc=10, scores=A, lds=10, B=8, C=10, tau=A, tau_rows=8, seed=A, k=5, ids=A, ldi=5, values=A,
           ldv=5, pos=A, ldq=5, logp=A, ldl=5):
        return lib.arx_slate_sample(cand, ldc, scores, lds, B, C, tau, tau_rows, seed, k, ids, ldi, values, ldv, pos,
                                    ldq, logp, ldl, None)
    for kw in (dict(cand=None), dict(scores=None), dict(tau=None), dict(seed=None), dict(ids=None), dict(values=None),
               dict(pos=None), dict(k=0), dict(k=-1), dict(k=11, ldi=11, ldv=11, ldq=11, ldl=11), dict(ldc=9),
               dict(lds=9), dict(ldi=4), dict(ldv=4), dict(ldq=4), dict(ldl=4), dict(tau_rows=0), dict(tau_rows=-3),
               dict(B=-1), dict(C=-1), dict(C=0, k=1), dict(B=0, k=0), dict(B=0, tau_rows=0)):
        assert ss(**kw) == EINVAL and "arx_slate_sample" in err(), kw
    wide = dict(ldc=2000, lds=2000)
    for kw in (dict(C=1025, **wide), dict(C=1025, B=0, **wide), dict(C=2000, k=2000, ldi=2000, ldv=2000, ldq=2000,
                                                                      ldl=2000, **wide)):
        assert ss(**kw) == EUNSUPPORTED, kw
        assert "arx_slate_sample_supported" in err() and "1024" in err(), kw
    # nothing to do launches nothing; a NULL logp is accepted, and its leading dimension is then not looked at
    assert ss(B=0) == 0 and ss(B=0, logp=None) == 0 and ss(B=0, logp=None, ldl=0) == 0
    assert ss(B=0, C=1024, k=1024, ldi=1024, ldv=1024, ldq=1024, ldl=1024, ldc=1024, lds=1024) == 0
    assert ss(B=0, C=1, k=1, ldc=1, lds=1, ldi=1, ldv=1, ldq=1, ldl=1, tau_rows=1) == 0


def test_predicate_on_both_sides_of_its_edges():
    from arx import ops
    for C in (1, 2, 64, 1000, 1023, 1024):
        assert ops.slate_sample_supported(C) is True, C
    for C in (0, -1, 1025, 2048, 2 ** 31, 2 ** 40, -2 ** 40):
        assert ops.slate_sample_supported(C) is False, C


# ---------------------------------------------------------------- 3. host rules
class _Fed(object):
    """A placeholder that counts its feeds."""
    def __init__(self):
        self.fed = []
        self.value = None

    def feed(self, x):
        self.fed.append(np.array(x))


def _fake_model(mb=4, V=50, d=8):
    """What arx.slate.score_items looks at, without a device: a G.Prediction over (latent [mb, d], pool [V, d]) that is
    never run, and an att_emb with the real seed counter of EmbeddingAttribute over counting placeholders."""
    from arx import graph as G
    from arx.attributes.embed_attribute import EmbeddingAttribute as EA
    out = G.Prediction.__new__(G.Prediction)
    out.inputs = (types.SimpleNamespace(shape=(mb, d)), types.SimpleNamespace(shape=(V, d)))
    att = types.SimpleNamespace(batch_size=mb, sample_draws=0, _sample_tau=_Fed(), _sample_seed=_Fed())
    att.sample_args = lambda: (None, mb, None)
    att.next_sample_seed = types.MethodType(EA.next_sample_seed, att)
    att.feed_sample = types.MethodType(EA.feed_sample, att)
    feeds = []
    model = types.SimpleNamespace(output=out, batch_size=mb, att_emb=att, _plans={}, rt=None, feeds=feeds)
    return model, (lambda: feeds.append(1))


def test_every_refusal_comes_before_any_feed():
    from arx import slate
    model, feed = _fake_model()
    cand = np.arange(40, dtype=np.int32).reshape(4, 10)
    big = np.zeros((4, 1025), dtype=np.int32)
    for kw, what in ((dict(k=None, sample_temperature=0.5), "needs k"),
                     (dict(k=3, sample_temperature=0.5, diversify=0.5), "diversify"),
                     (dict(k=3, sample_temperature=0.5, max_per_group=2), "max_per_group"),
                     (dict(k=3, sample_seed=4), "sample_temperature"),
                     (dict(k=3, return_logprob=True), "sample_temperature"),
                     (dict(k=None, return_logprob=True), "sample_temperature"),
                     (dict(k=3, sample_temperature=-1.0), "sample_temperature"),
                     (dict(k=3, sample_temperature=float('nan')), "sample_temperature"),
                     (dict(k=3, sample_temperature=[0.5, 0.5]), "sample_temperature"),
                     (dict(k=3, sample_temperature=True), "sample_temperature"),
                     (dict(k=3, sample_temperature=0.5, sample_seed=-1), "sample_seed"),
                     (dict(k=3, sample_temperature=0.5, sample_seed=2 ** 63), "sample_seed"),
                     (dict(k=3, sample_temperature=0.5, sample_seed=1.5), "sample_seed")):
        with pytest.raises(ValueError, match=what):
            slate.score_items(model, feed, cand, **kw)
    with pytest.raises(ValueError, match="arx_slate_sample_supported"):
        slate.score_items(model, feed, big, k=3, sample_temperature=0.5)
    assert model.feeds == [] and model._plans == {} and model.att_emb.sample_draws == 0
    assert model.att_emb._sample_tau.fed == [] and model.att_emb._sample_seed.fed == []


def test_the_draw_counter_moves_only_on_an_accepted_unseeded_call():
    """The accepted calls replay a plan that is already there -- a stand-in whose run() does nothing: what is checked
    is what score_items feeds and when the counter moves."""
    import torch
    from arx import slate
    model, feed = _fake_model()
    C, k = 10, 3
    ids_in = _Fed()
    node = types.SimpleNamespace(inputs=(types.SimpleNamespace(inputs=(None, None, ids_in)),),
                                 top_ids=torch.zeros(4, k, dtype=torch.int32), top_values=torch.zeros(4, k),
                                 logp=torch.zeros(4, k))
    runs = []
    model._plans[('score_items', C, k, 'sample')] = types.SimpleNamespace(fetch=[node], run=lambda: runs.append(1))
    cand = np.arange(40, dtype=np.int32).reshape(4, 10)
    att = model.att_emb
    words = lambda: [int(x) for x in att._sample_seed.fed[-1].view(np.uint32)]
    out = slate.score_items(model, feed, cand, k, sample_temperature=0.5)
    assert len(out) == 2 and att.sample_draws == 1 and words() == [0, 0]
    out = slate.score_items(model, feed, cand, k, sample_temperature=[0.0, 0.5, 1.0, 2.0], return_logprob=True)
    assert len(out) == 3 and att.sample_draws == 2 and words() == [1, 0]
    np.testing.assert_array_equal(att._sample_tau.fed[-1], np.array([0.0, 0.5, 1.0, 2.0], dtype=np.float32))
    slate.score_items(model, feed, cand, k, sample_temperature=0.5, sample_seed=2 ** 40 + 7)     # a given seed: stays
    assert att.sample_draws == 2 and words() == [7, 2 ** 8]
    for kw in (dict(sample_temperature=-0.5), dict(sample_temperature=0.5, diversify=0.3),
               dict(sample_temperature=[1.0] * 3)):                                              # refused: stays
        with pytest.raises(ValueError):
            slate.score_items(model, feed, cand, k, **kw)
    assert att.sample_draws == 2 and len(runs) == 3 and len(ids_in.fed) == 3 and len(model.feeds) == 3
    slate.score_items(model, feed, cand, k, sample_temperature=0.5)
    assert att.sample_draws == 3 and words() == [2, 0]
    assert list(model._plans) == [('score_items', C, k, 'sample')] and all(len(q) == 4 for q in model._plans)


def test_the_new_keywords_exist():
    import inspect
    from arx import ops, slate
    from arx.hmf.hmf_model import LatentProductModel
    from arx.word2vec.linear_seq import LinearSeq
    for f in (LatentProductModel.score_items, LinearSeq.score_items, slate.score_items):
        p = inspect.signature(f).parameters
        assert p['sample_temperature'].default is None and p['sample_seed'].default is None
        assert p['return_logprob'].default is False
    assert callable(ops.slate_sample) and callable(ops.slate_sample_supported) and callable(slate.SlateSample)


# ---------------------------------------------------------------- 4. the oracle
def test_oracle_propensities_of_all_ordered_lists_sum_to_one():
    """C = 5, k = 3: exp(sum logp) over the 60 ordered lists is 1 within 1e-12."""
    cand = np.array([[7, 3, 11, 0, 5]])
    s = np.array([[0.3, -1.2, 2.0, 0.7, -0.4]], dtype=np.float32)
    for tau in (0.25, 1.0, 7.0):
        total = 0.0
        for perm in itertools.permutations(range(5), 3):
            total += np.exp(SS.logprob(cand, s, [tau], np.array([perm])).sum())
        assert abs(total - 1.0) < 1e-12, (tau, total)
    assert (SS.logprob(cand, s, [0.0], np.array([[2, 3, 0]])) == 0).all()
    assert (SS.logprob(cand, s, [1.0], np.array([[2, -1, -1]]))[0, 1:] == 0).all()


def test_oracle_a_duplicated_id_is_the_slate_with_the_later_copy_emptied():
    rng = np.random.default_rng(5)
    B, C, k = 6, 12, 12
    cand = np.stack([rng.permutation(40)[:C] for _ in range(B)])
    s = rng.standard_normal((B, C)).astype(np.float32)
    cand[:, 9] = cand[:, 2]; s[:, 9] = s[:, 2]                    # the same id, the same score bits
    cand[:, 5] = cand[:, 2]; s[:, 5] = s[:, 2]
    tau = np.array([0, 0.05, 1, 50, 1, 0.3], dtype=np.float32)
    g = SS.noise64(3, range(B), cand)
    emptied = cand.copy(); emptied[:, [5, 9]] = -1
    a = SS.select(cand, s, g, tau, k)
    b = SS.select(emptied, s, SS.noise64(3, range(B), emptied), tau, k)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert (a[2][:, :10] >= 0).all() and (a[2][:, 10:] == -1).all()
    assert not np.isin(a[2], [5, 9]).any()
    np.testing.assert_array_equal(SS.logprob(cand, s, tau, a[2]), SS.logprob(emptied, s, tau, b[2]))


LAW_IDS = [5, 17, 2, 40, 33, 8]
LAW_SCORES = [0, .5, 1, 1.5, -.5, .25]
LAW_TAU, LAW_ROWS, LAW_BOUND = 0.7, 4096, 58.30                   # the 0.999 quantile of chi^2 at 29 degrees


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_law_statistic_on_the_oracle_s_own_draws(seed):
    cand = np.tile(np.array(LAW_IDS, dtype=np.int32), (LAW_ROWS, 1))
    s = np.tile(np.array(LAW_SCORES, dtype=np.float32), (LAW_ROWS, 1))
    tau = np.full(LAW_ROWS, LAW_TAU, dtype=np.float32)
    ids, _, pos = SS.select(cand, s, SS.noise64(seed, range(LAW_ROWS), cand), tau, 2)
    lp = SS.logprob(cand, s, tau, pos)
    chi2, cells, small = SS.pair_chi2(ids, lp, LAW_IDS, SS.exact_pairs(LAW_IDS, LAW_SCORES, float(np.float32(LAW_TAU))))
    print("seed %d: chi2 = %.2f over %d cells, smallest expected %.2f" % (seed, chi2, cells, small))
    assert cells == 30 and 6.0 < small < 7.0
    assert chi2 < LAW_BOUND
