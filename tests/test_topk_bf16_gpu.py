"""recommend(scan_dtype='bf16') on the GPU: the bf16 filter scan with its exact f32 re-score (arx_topk_bf16.h).

What is compared with what:
  * exact-arithmetic inputs (multiples of 2^-3, biases multiples of 2^-6: every product and sum is exact in bf16 and in
    f32): ids AND values bit-identical to the f32 StreamTopK of the same node and to the float64 oracle;
  * continuous inputs: against the float64 oracle (tests/topk_bf16_oracle.py).  Values are held to the figure the
    re-scoring arithmetic is held to in tests/test_score_items_gpu.py -- |got - ref| <= 2 (d + 1) 2^-24 (sum |u p| + |b|),
    the textbook bound of a float32 dot in any order, which covers the first chunk's f32 GEMM as well -- and a
    first-chunk winner's value to rtol 1e-6 of the device's own f32 logit (tests/test_recommend_tags_gpu.py).  ids are
    compared on every row whose float64 gaps around the returned positions exceed the two values' bounds; the other
    rows (at most 2 %; the seeds below leave at most two of 130, counted on the CPU) are computed and left out;
  * the margin: columns the bf16 image alone would lose, and columns it alone would wrongly keep.
The smallest shapes of tests/test_recommend_tags_gpu.py: B = 130 (a full panel and a ragged one of 2 rows), V = 256 +
5 * 64 + 17 with chunk = 256 (five full tiles and a ragged one).
"""
import numpy as np
import pytest

import slate_oracle as SO
import tags_oracle as T
import topk_bf16_oracle as O
from test_recommend_exclude_gpu import _const, _csr, _hmf, _row_cols, _skipgram

pytestmark = pytest.mark.gpu

B0, V0, N0 = 130, 256 + 5 * 64 + 17, 256


class _Rig(object):
    """latent [B, d] and pool [V, d] + bias as graph nodes over GIVEN arrays"""

    def __init__(self, U, P, b):
        import torch
        from arx import graph as G
        self.rt = rt = G.Runtime()
        self.U, self.P, self.b = U, P, b
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)
        self.latent, self.pool = _const(rt, up(U)), _const(rt, up(P), up(b) if b is not None else None)

    def exclusions(self, lists):
        import torch
        ptr, cols = _csr(lists)
        dev = self.rt.device
        keys = np.arange(len(lists), dtype=np.int32)
        return (torch.from_numpy(keys).to(dev), len(keys), torch.from_numpy(ptr).to(dev), torch.from_numpy(cols).to(dev))

    def tags(self, tags, want_any, want_all):
        import torch
        up = lambda a: torch.from_numpy(T.i32(a)).to(self.rt.device)
        return (up(tags), up(want_any), up(want_all), len(want_any))

    def device_logits(self):
        """the f32 GEMM's logits, as the streaming node's chunks compute them"""
        import torch
        from arx import ops
        out = torch.empty((self.U.shape[0], self.P.shape[0]), dtype=torch.float32, device=self.rt.device)
        ops.gemm(self.latent.value, self.pool.value, out, self.rt.ws, transB=True, col_bias=self.pool.bias_value)
        return out.cpu().numpy()


def _filters(rng, B, V, exact64, with_ex, with_tags):
    """(row lists or None, (tags, any, all) or None, eligible bool [B, V])"""
    el = np.ones((B, V), dtype=bool)
    lists = tg = None
    if with_ex:
        top = np.argpartition(-exact64, 12, axis=1)[:, :12]                # adversarial: each row's own best columns
        lists = [np.unique(np.concatenate([top[r], rng.integers(0, V, 30)])) for r in range(B)]
        lists[1] = np.zeros(0, dtype=np.int64)
        for r, c in enumerate(lists):
            el[r, c] = False
    if with_tags:
        tags = T.random_tags(rng, V)
        want_any, want_all = T.random_words(rng, B)
        tg = (tags, want_any, want_all)
        el &= T.eligible(tags, want_any, want_all)
    return lists, tg, el


def _nodes(rig, k, lists, tg, **kw):
    from arx.hmf import hmf_model as hm
    ex = rig.exclusions(lists) if lists is not None else None
    ta = rig.tags(*tg) if tg is not None else None
    mk = lambda bf: hm.StreamTopK(rig.rt, rig.latent, rig.pool, k, chunk=N0, exclude=(lambda: ex) if ex else None,
                                  tags=(lambda: ta) if ta else None, scan_bf16=bf, **kw)
    return mk(False), mk(True)


# ---------------------------------------------------------------- exact-arithmetic inputs
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("k", [1, 10])
def test_exact_arithmetic_inputs_bit_identical_to_the_f32_scan(dev, d, k):
    """Plain, with exclusions, with tags, with both: ids and values of the bf16 node equal the f32 node's bit for bit
    (and the float64 oracle's).  Such data has ties in every row: the column-order tie rule through the new placement."""
    rng = np.random.default_rng(1000 * d + k)
    U, P, b = O.dyadic(rng, B0, V0, d)
    rig = _Rig(U, P, b)
    exact = O.exact_dot(U, P) + b.astype(np.float64)[None, :]
    assert max(len(np.unique(e)) for e in exact) < V0 - 20                   # scores on a 2^-6 grid: ties in every row
    for with_ex, with_tags in ((False, False), (True, False), (False, True), (True, True)):
        lists, tg, el = _filters(rng, B0, V0, exact, with_ex, with_tags)
        f32, bf = _nodes(rig, k, lists, tg)
        assert f32.fused and bf.fused and bf.scan_bf16 and not f32.scan_bf16
        f32.forward(False)
        bf.forward(False)
        what = 'ex=%s tags=%s' % (with_ex, with_tags)
        if not bf.overflowed():                                              # (a rare tag leaves thr = -inf: below)
            assert bf._bf16 is not None and tuple(bf._bf16[0].shape) == (V0 - N0, d)
        else:
            assert with_tags
            from arx.topk import run_complete
            run_complete(bf, lambda: bf.forward(False))
            run_complete(f32, lambda: f32.forward(False))
        ev, ei = O.topk_rows(np.where(el, exact, -np.inf), k)
        gi, gv = bf.indices.cpu().numpy(), bf.value.cpu().numpy()
        np.testing.assert_array_equal(gi, f32.indices.cpu().numpy(), err_msg=what)
        np.testing.assert_array_equal(gv.view(np.int32), f32.value.cpu().numpy().view(np.int32), err_msg=what)
        np.testing.assert_array_equal(gi, ei, err_msg=what)
        np.testing.assert_array_equal(gv, ev.astype(np.float32), err_msg=what)
        assert (gi >= N0).any()                                              # (winners from the bf16-scanned tail)


# ---------------------------------------------------------------- continuous inputs
def _continuous(d, k):
    """seeded normal data in the scales of the other top-k tests; the seed of (d, k) keeps the oracle's own near-ties
    under the 2 % cap (_gap_rows needs no device: the counts beside SEEDS were taken on the CPU, the test asserts them)"""
    rng = np.random.default_rng(SEEDS[(d, k)])
    U = rng.standard_normal((B0, d)).astype(np.float32)
    P = (rng.standard_normal((V0, d)) * 0.5).astype(np.float32)
    b = (rng.standard_normal(V0) * 0.5).astype(np.float32)
    return rng, U, P, b


# rows left out per (plain, filtered) case, counted on the CPU: (32, 10): 1, 0; (64, 10): 1, 0; (128, 10): 2, 2 (the value
# bound grows with d: at d = 128 it is 1.2e-3 against top-10 gaps of ~0.1); none at k = 1
SEEDS = {(32, 1): 321, (32, 10): 3210, (64, 1): 641, (64, 10): 1, (128, 1): 1281, (128, 10): 13}


def _value_bound(U, P, b, d):
    """[B, V]: 2 (d + 1) 2^-24 (sum |u p| + |b|), the figure of test_score_items_gpu.py"""
    a = np.abs(U.astype(np.float64)) @ np.abs(P.astype(np.float64)).T
    if b is not None:
        a = a + np.abs(b.astype(np.float64))[None, :]
    return SO.bound(d) * a


def _gap_rows(scores, lim, k):
    """bool [B]: rows whose float64 gaps around the first k positions (the k-th against the (k+1)-th included) all
    exceed the two neighbours' value bounds -- where the ids of an f32 computation must equal the oracle's."""
    ok = np.ones(scores.shape[0], dtype=bool)
    col = np.arange(scores.shape[1])
    for r in range(scores.shape[0]):
        o = np.lexsort((col, -scores[r]))[:k + 1]
        s, l = scores[r, o], lim[r, o]
        live = np.isfinite(s[:-1]) & np.isfinite(s[1:])
        ok[r] = bool(np.all((s[:-1][live] - s[1:][live]) > (l[:-1] + l[1:])[live]))
    return ok


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("k", [1, 10])
def test_continuous_inputs_against_the_float64_oracle(dev, d, k):
    rng, U, P, b = _continuous(d, k)
    rig = _Rig(U, P, b)
    exact = O.exact_dot(U, P) + b.astype(np.float64)[None, :]
    lim = _value_bound(U, P, b, d)
    dev_logits = rig.device_logits()
    for with_ex, with_tags in ((False, False), (True, True)):
        lists, tg, el = _filters(rng, B0, V0, exact, with_ex, with_tags)
        sc = np.where(el, exact, -np.inf)
        ok = _gap_rows(sc, lim, k)
        print("d=%d k=%d ex=%s: %d of %d rows left out (near-ties of the oracle)" % (d, k, with_ex, (~ok).sum(), B0))
        assert (~ok).sum() <= 0.02 * B0
        _, bf = _nodes(rig, k, lists, tg)
        bf.forward(False)
        assert bf.fused and not bf.overflowed() and bf._bf16 is not None
        ev, ei = O.topk_rows(sc, k)
        gi, gv = bf.indices.cpu().numpy().astype(np.int64), bf.value.cpu().numpy()
        np.testing.assert_array_equal(gi[ok], ei[ok])
        assert np.array_equal(gi < 0, np.isneginf(gv))
        for r in range(B0):                                                  # every row: the values of ITS ids
            live = gi[r] >= 0
            c = gi[r][live]
            assert el[r, c].all() and len(set(c.tolist())) == len(c)
            assert (np.abs(gv[r][live].astype(np.float64) - exact[r, c]) <= lim[r, c]).all()
            first = c < N0
            np.testing.assert_allclose(gv[r][live][first], dev_logits[r, c[first]], rtol=1e-6)
        assert (gi >= N0).any()


# ---------------------------------------------------------------- the margin does its work
def test_margin_keeps_the_winners_the_bf16_image_would_lose(dev):
    """d = 32, user rows of ones.  Exactly k first-chunk columns of entries 1 + 2^-10 (score 32 + 2^-5) set the
    threshold; tail columns of entries 1 + 2^-9 score 32 + 2^-4 -- winners -- but their bf16 image is 1.0 and their
    approximate score 32, BELOW the threshold: only the margin lets them through.  All of them must be returned."""
    d, k = 32, 10
    U = np.ones((B0, d), dtype=np.float32)
    P = np.zeros((V0, d), dtype=np.float32)
    first = np.array([3, 17, 40, 41, 99, 128, 130, 200, 254, 255])
    tail = np.array([N0, N0 + 63, N0 + 64, N0 + 200, N0 + 319, V0 - 1])     # every tile, the ragged one's last column
    P[first] = 1 + 2.0 ** -10
    P[tail] = 1 + 2.0 ** -9
    assert (O.bf16_round(P[tail]) == 1.0).all()
    rig = _Rig(U, P, None)
    f32, bf = _nodes(rig, k, None, None)
    f32.forward(False)
    bf.forward(False)
    assert not bf.overflowed()
    exp_i = np.concatenate([tail, first[:k - len(tail)]])
    exp_v = np.concatenate([np.full(len(tail), 32 + 2.0 ** -4), np.full(k - len(tail), 32 + 2.0 ** -5)])
    gi, gv = bf.indices.cpu().numpy(), bf.value.cpu().numpy()
    np.testing.assert_array_equal(gi, np.broadcast_to(exp_i, (B0, k)))
    np.testing.assert_array_equal(gv, np.broadcast_to(exp_v.astype(np.float32), (B0, k)))
    np.testing.assert_array_equal(gi, f32.indices.cpu().numpy())
    np.testing.assert_array_equal(gv, f32.value.cpu().numpy())


def test_columns_whose_image_rounds_up_past_the_threshold_are_not_returned(dev):
    """The mirror: first-chunk columns of entries 1 + 2^-8 + 2^-9 (score 32.1875) set the threshold; tail columns of
    entries 1 + 2^-8 + 2^-16 score 32.1255 -- losers -- but their image is 1 + 2^-7, approximate score 32.25, ABOVE it.
    They pass the filter; the exact re-score must keep them out."""
    d, k = 32, 10
    U = np.ones((B0, d), dtype=np.float32)
    P = np.zeros((V0, d), dtype=np.float32)
    first = np.array([3, 17, 40, 41, 99, 128, 130, 200, 254, 255])
    tail = np.array([N0, N0 + 63, N0 + 64, N0 + 200, N0 + 319, V0 - 1])
    P[first] = 1 + 2.0 ** -8 + 2.0 ** -9
    P[tail] = 1 + 2.0 ** -8 + 2.0 ** -16
    assert (O.bf16_round(P[tail]) == np.float32(1 + 2.0 ** -7)).all()
    rig = _Rig(U, P, None)
    f32, bf = _nodes(rig, k, None, None)
    f32.forward(False)
    bf.forward(False)
    assert not bf.overflowed()
    gi, gv = bf.indices.cpu().numpy(), bf.value.cpu().numpy()
    np.testing.assert_array_equal(gi, np.broadcast_to(first, (B0, k)))
    np.testing.assert_array_equal(gv, np.full((B0, k), 32.1875, dtype=np.float32))
    np.testing.assert_array_equal(gi, f32.indices.cpu().numpy())
    # they DID pass the filter (the test is about the re-score): their slots hold the exact score now, not 32.25
    _, cand_v, cand_i, _, _ = bf._cand_bufs(N0, V0)
    cv, ci = cand_v.cpu().numpy(), cand_i.cpu().numpy()
    occ = ~np.isneginf(cv)
    assert sorted(set(ci[occ].tolist())) == sorted(tail.tolist())
    np.testing.assert_array_equal(cv[occ], np.float32(32 * (1 + 2.0 ** -8 + 2.0 ** -16)))


# ---------------------------------------------------------------- the kernels through the ABI
@pytest.mark.parametrize("K", [8, 32, 64, 128, 200])
def test_rows_bf16_norm_bit_exact_against_numpy(dev, K):
    """The image against numpy's round-to-nearest-even, ties to even and a NaN included, out of a strided view and
    with a ragged last row block; the norms >= the float64 norm and within 2^-18 of it."""
    import torch
    from arx import ops
    rng = np.random.default_rng(K)
    N, ld = 37, K + 8
    X = (rng.standard_normal((N, ld)) * np.exp(rng.standard_normal((N, 1)) * 3)).astype(np.float32)
    X[1, :K] = 1 + 2.0 ** -8                    # ties: to the even significand (down)
    X[2, :K] = -(1 + 3 * 2.0 ** -8)             # ties: to the even significand (up in magnitude)
    X[3, :K] = 1 + 2.0 ** -8 + 2.0 ** -20
    X[4, :K] = 0.0
    X[5, :K] = np.float32(2.0 ** -40)
    dx = torch.from_numpy(X).to(dev)
    view = dx[:, :K]
    img = torch.full((N + 1, K), 7.0, dtype=torch.bfloat16, device=dev)
    nrm = torch.full((N + 1,), -1.0, dtype=torch.float32, device=dev)
    ops.rows_bf16_norm(view, img[:N], nrm[:N])
    got = img.view(torch.int16).cpu().numpy().view(np.uint16)
    np.testing.assert_array_equal(got[:N], O.bf16_bits(X[:, :K]))
    assert (got[N] == 0x40e0).all() and float(nrm[N].item()) == -1.0                           # nothing past row N
    ref = O.norms(X[:, :K])
    n = nrm[:N].cpu().numpy().astype(np.float64)
    assert (n >= ref).all() and (n <= ref * (1 + 2.0 ** -18)).all() and n[4] == 0.0
    Y = X[:, :K].copy()
    Y[6, K // 2] = np.nan
    ops.rows_bf16_norm(torch.from_numpy(Y).to(dev), img[:N], nrm[:N])
    got = img.view(torch.int16).cpu().numpy().view(np.uint16)
    np.testing.assert_array_equal(got[:N], O.bf16_bits(Y))
    assert got[6, K // 2] == 0x7fc0 and np.isnan(nrm[6].item())


@pytest.mark.parametrize("d", [32, 64, 128])
def test_filter_candidate_lists_equal_the_oracles_survivors_in_column_order(dev, d):
    """arx_gemm_nt_topk_filter_bf16 alone: per row, the occupied slots of its segments read part after part are the
    oracle's survivor set in ascending column order, exclusions and tags applied; every stored value is the
    approximate v~.  Columns whose widened logit lies within the rounding of the two sides' arithmetic of the
    threshold may fall either way: the data leaves few, and they are checked to be the only difference."""
    import torch
    from arx import ops
    from arx.topk import bf16_margin_coeff, bf16_margin_coeff_f32
    rng = np.random.default_rng(50 + d)
    U = rng.standard_normal((B0, d)).astype(np.float32)
    P = (rng.standard_normal((V0, d)) * np.exp(rng.standard_normal((V0, 1)) * 0.5)).astype(np.float32)
    b = (rng.standard_normal(V0) * 0.5).astype(np.float32)
    rig = _Rig(U, P, b)
    exact = O.exact_dot(U, P) + b.astype(np.float64)[None, :]
    lists, tg, _ = _filters(rng, B0, V0, exact, True, True)
    tags, want_any, want_all = tg
    thr = np.sort(exact[:, :N0], axis=1)[:, -10].astype(np.float32)
    thr[7] = -np.inf                                                         # a row without a threshold:
    lists[7] = np.arange(N0 + 40, V0)                                        # (few columns, or its segments overflow)
    want_any[7] = want_all[7] = 0
    el = T.eligible(tags, want_any, want_all)
    for r, c in enumerate(lists):
        el[r, c] = False
    tl = V0 - N0
    dev_ = rig.rt.device
    img = torch.empty((tl, d), dtype=torch.bfloat16, device=dev_)
    coln = torch.empty(tl, dtype=torch.float32, device=dev_)
    ops.rows_bf16_norm(rig.pool.value[N0:], img, coln)
    parts, capp = ops.gemm_nt_topk_parts(B0, tl), 64
    cand_v = torch.full((B0, parts * capp), float('-inf'), dtype=torch.float32, device=dev_)
    cand_i = torch.full((B0, parts * capp), -5, dtype=torch.int32, device=dev_)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev_)
    ta = rig.tags(tags, want_any, want_all)
    ops.gemm_nt_topk_filter_bf16(rig.latent.value, img, coln, rig.pool.bias_value[N0:], torch.from_numpy(thr).to(dev_),
                                 N0, cand_v, cand_i, capp, ovf, bf16_margin_coeff_f32(d),
                                 tags=(ta[0][N0:],) + tuple(ta[1:]), ex=rig.exclusions(lists))
    assert int(ovf.item()) == 0
    cv, ci = cand_v.cpu().numpy(), cand_i.cpu().numpy()
    w, v = O.widened(U, P[N0:], b[N0:], bf16_margin_coeff(d))
    # what the two sides' arithmetic may disagree by: the order of the f32 adds, the norms rounded up, two steps of thr
    t = thr.astype(np.float64)[:, None]
    slack = 4 * _value_bound(U, P[N0:], b[N0:], d) + 2.0 ** -16 * (w - v) + np.where(np.isfinite(t), 2.0 ** -21 * np.abs(t), 0)
    sure = (w > t + slack) & el[:, N0:]
    maybe = (w > t - slack) & el[:, N0:]
    assert (maybe & ~sure).sum() <= 3 and sure.sum() > B0
    for r in range(B0):
        occ = ~np.isneginf(cv[r])
        cols = ci[r][occ]
        assert (ci[r][~occ] == -5).all()                                     # nothing written beside the survivors
        assert (np.diff(cols) > 0).all(), r                                  # ascending over the parts
        got = np.zeros(tl, dtype=bool)
        got[cols - N0] = True
        assert (got >= sure[r]).all() and (got <= maybe[r]).all(), r
        lim = _value_bound(U[r:r + 1], P[cols], b[cols], d)[0]
        assert (np.abs(cv[r][occ].astype(np.float64) - v[r, cols - N0]) <= lim).all()
        for p in range(parts):                                               # a part's slots fill from the front
            o = occ[p * capp:(p + 1) * capp]
            assert not (o[1:] & ~o[:-1]).any()
    assert (~np.isneginf(cv[7])).sum() == el[7, N0:].sum() > 0               # thr = -inf: every eligible column


def test_overflow_flag_then_the_chunked_path_gives_the_oracle(dev):
    """Candidate segments forced short and a tail that beats the first chunk: the bf16 run raises the overflow flag,
    run_complete re-runs chunked (f32) and the result is the f32 node's chunked one bit for bit, the oracle's ids."""
    from arx.topk import run_complete
    d, k = 64, 10
    rng = np.random.default_rng(77)
    U, P, b = O.dyadic(rng, B0, V0, d)
    b[N0:] += 8.0                                                            # most tail columns beat every threshold
    rig = _Rig(U, P, b)
    f32, bf = _nodes(rig, k, None, None)
    for n in (f32, bf):
        n.slack, n.min_capp = 0.0, 8
    bf.forward(False)
    assert bf.overflowed()
    run_complete(bf, lambda: bf.forward(False))
    assert bf.fused and int(bf.overflow.item()) != 0                         # (overflowed, re-ran chunked, restored)
    with f32.chunked():
        f32.forward(False)
    exact = O.exact_dot(U, P) + b.astype(np.float64)[None, :]
    ev, ei = O.topk_rows(exact, k)
    np.testing.assert_array_equal(bf.indices.cpu().numpy(), ei)
    np.testing.assert_array_equal(bf.indices.cpu().numpy(), f32.indices.cpu().numpy())
    np.testing.assert_array_equal(bf.value.cpu().numpy(), f32.value.cpu().numpy())


def test_cand_rescore_equals_slate_scores_bit_for_bit_and_skips_empties(dev):
    import torch
    from arx import ops
    rng = np.random.default_rng(5)
    for d in (32, 64, 128, 20):
        Bn, V, C = 9, 700, 75
        U = rng.standard_normal((Bn, d)).astype(np.float32)
        P = rng.standard_normal((V, d)).astype(np.float32)
        b = rng.standard_normal(V).astype(np.float32)
        cand = rng.integers(0, V, size=(Bn, C)).astype(np.int32)
        empty = rng.random((Bn, C)) < 0.4
        empty[3] = True
        val = np.where(empty, -np.inf, rng.standard_normal((Bn, C))).astype(np.float32)
        cand[empty] = 2 ** 31 - 1                                            # stale indices of empty slots: never read
        up = lambda a: torch.from_numpy(a).to(dev)
        dU, dP, db, dc = up(U), up(P), up(b), up(cand)
        want = torch.empty((Bn, C), dtype=torch.float32, device=dev)
        ops.slate_scores(dU, dP, db, up(np.where(empty, 0, cand).astype(np.int32)), want)
        wide_v = torch.full((Bn, C + 5), 3.0, dtype=torch.float32, device=dev)
        wide_v[:, :C] = up(val)
        wide_i = torch.zeros((Bn, C + 5), dtype=torch.int32, device=dev)
        wide_i[:, :C] = dc
        ops.cand_rescore(dU, dP, db, wide_v[:, :C], wide_i[:, :C])
        got = wide_v.cpu().numpy()
        exp = np.where(empty, -np.inf, want.cpu().numpy()).astype(np.float32)
        np.testing.assert_array_equal(got[:, :C].view(np.int32), exp.view(np.int32), err_msg=str(d))
        assert (got[:, C:] == 3.0).all()


# ---------------------------------------------------------------- end to end
def _oracle_ids(node, rows, k):
    """float64 top-k of the node's OWN latent and pool (as they stand after its last run) without each row's
    columns `rows`, the rows where an f32 computation must agree, and the scores"""
    U, P = node.inputs[0].value.cpu().numpy(), node.inputs[1].value.cpu().numpy()
    bias = node.inputs[1].bias_value
    b = bias.cpu().numpy() if bias is not None else None
    sc = O.exact_dot(U, P)
    if b is not None:
        sc = sc + b.astype(np.float64)[None, :]
    for r, c in enumerate(rows or []):
        sc[r, np.asarray(c, dtype=np.int64)] = -np.inf
    ok = _gap_rows(sc, _value_bound(U, P, b, U.shape[1]), k)
    return O.topk_rows(sc, k)[1], ok


def _hmf_het(seed, B=32, top_n=30, d=32):
    from arx.hmf.hmf_model import LatentProductModel
    from arx.utils.synthetic import SyntheticHMF
    syn = SyntheticHMF(seed=seed, n_users=200, n_items=5000, logit_size=4800, item_mulhot=True, mulhot_vocab=300,
                       avg_len=4, max_len=9)
    params = syn.glorot_params(d, seed=seed + 1, scale=0.5)
    i2l, l2i = syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind
    model = LatentProductModel(syn.n_users, syn.n_items, d, 1, B, 0.5, 1.0, syn.u_attr, syn.i_attr, i2l, l2i,
                               loss_function='ce', params=params, top_N_items=top_n)
    return syn, model


@pytest.mark.parametrize("het", [False, True])
@pytest.mark.parametrize("exclude_seen", [False, True])
def test_hmf_bf16_streamed_equals_materialised(dev, monkeypatch, het, exclude_seen):
    """LatentProductModel.step(recommend, scan_dtype='bf16') of a streaming model (a first chunk of 1536) against the
    materialised f32 twin: eager, captured, replayed; after a training step of both (the image is rebuilt from the new
    table -- for HET items the latents are recomputed per call anyway); beside the f32 plan of the same filters."""
    from arx.hmf import hmf_model as hm
    make = _hmf_het if het else _hmf
    syn, mat = make(4)
    monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '0')
    _, st = make(4)
    assert isinstance(st.topk, hm.StreamTopK) and isinstance(mat.topk, hm.TopK)
    st.topk.chunk = 1536
    st.topk._buf = st.topk._buf[:, :1536].contiguous()
    rng = np.random.default_rng(6)
    B, k = mat.batch_size, mat.topk.k
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    sets = {int(u): rng.integers(0, syn.n_items, 60).tolist() for u in users}
    rows = _row_cols(syn, sets, users) if exclude_seen else None
    if exclude_seen:
        for m in (mat, st):
            m.prepare_recommend_exclusions(sets)
    key = 'recommend_ex_bf16' if exclude_seen else 'recommend_bf16'
    kw = dict(recommend=True, exclude_seen=exclude_seen)
    seen = []
    for phase in range(2):
        for n in range(3):                                                   # eager, captured, replayed
            exp = mat.step(None, list(users), None, **kw)
            got = st.step(None, list(users), None, scan_dtype='bf16', **kw)
            node = st._bf16_nodes[key]
            assert isinstance(node, hm.StreamTopK) and node.fused and node.scan_bf16 and node.chunk == 1536
            assert int(node.overflow.item()) == 0 and node._bf16 is not None
            ei, ok = _oracle_ids(node, rows, k)                              # (a model's items may score alike:
            assert ok.sum() >= B // 2                                        # such a row is held to the twin alone)
            np.testing.assert_array_equal(got[ok], ei[ok], err_msg='phase %d call %d' % (phase, n))
            np.testing.assert_array_equal(got, exp, err_msg='phase %d call %d' % (phase, n))
        seen.append(got)
        # the f32 plan of the same filters beside it: its own node, the same answer, both plans kept
        f32 = st.step(None, list(users), None, **kw)
        np.testing.assert_array_equal(f32, exp)
        assert key in st._plans and key[:-5] in st._plans and st._recommend_node(key[:-5]) is not node
        assert not st._recommend_node(key[:-5]).scan_bf16
        if phase == 0:                                                       # a training step in between
            tu, ti = syn.sample_batch(B, rng)
            for _ in range(3):
                for m in (mat, st):
                    m.step(None, list(tu), list(ti))
    assert (seen[0] != seen[1]).any()                                        # the answer followed the new table
    # the chunked route of the same plan key: f32, still the answer
    node.fused = False
    st._plans.pop(key, None)
    np.testing.assert_array_equal(st.step(None, list(users), None, scan_dtype='bf16', **kw), exp)


@pytest.mark.parametrize("exclude_seen", [False, True])
def test_linear_seq_bf16(dev, monkeypatch, exclude_seen):
    from arx.hmf import hmf_model as hm
    syn, mat = _skipgram()
    monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '0')
    _, st = _skipgram()
    assert isinstance(st.topk, hm.StreamTopK) and isinstance(mat.topk, hm.TopK)
    st.topk.chunk = 128
    st.topk._buf = st.topk._buf[:, :128].contiguous()
    B, k = mat.batch_size, mat.topk.k
    rng = np.random.default_rng(9)
    users = rng.choice(syn.n_users, B, replace=False).astype(np.int32)
    ctx = syn.sample_batch(B, rng)[1][None, :]
    sets = {int(u): rng.integers(0, syn.n_items, 50).tolist() for u in users}
    rows = _row_cols(syn, sets, users) if exclude_seen else None
    if exclude_seen:
        for m in (mat, st):
            m.prepare_recommend_exclusions(sets)
    key = 'recommend_ex_bf16' if exclude_seen else 'recommend_bf16'
    rec = lambda m, **kw: m.step(None, list(users), ctx.tolist(), recommend=True, exclude_seen=exclude_seen, **kw)
    for n in range(3):
        exp, got = rec(mat), rec(st, scan_dtype='bf16')
        node = st._bf16_nodes[key]
        assert node.fused and node.scan_bf16 and int(node.overflow.item()) == 0 and node._bf16 is not None
        ei, ok = _oracle_ids(node, rows, k)
        assert ok.sum() >= B // 2
        np.testing.assert_array_equal(got[ok], ei[ok], err_msg='call %d' % n)
        np.testing.assert_array_equal(got, exp, err_msg='call %d' % n)
    np.testing.assert_array_equal(rec(st), exp)
    assert key in st._plans and key[:-5] in st._plans
    # a dense recommend has no scan: the option is accepted and changes nothing
    np.testing.assert_array_equal(rec(mat, scan_dtype='bf16'), exp)
    assert not getattr(mat, '_bf16_nodes', None)
    with pytest.raises(NotImplementedError, match="sample_temperature"):
        rec(st, scan_dtype='bf16', sample_temperature=0.5)
