"""The order of the bag sum (bag_sum in gather.hip), bit for bit, behind every entry point that forms a bag mean:
ops.gather_mulhot_mean, ops.gather_id_plus_bag, ops.lookup_multi (four sites in one launch) and the serving kernel
ops.het_rows_range at world 1.

The host model is a float32 numpy restatement of the kernels' arithmetic: per block of LPR tokens (LPR = lanes per
row), cnt = min(LPR, len - j0) and full = cnt & ~3; token t < full is added to accumulator t % 4, the tokens
full <= t < cnt to accumulator 0 one after the other behind the full groups; the accumulators carry over the blocks;
the row is scale * (((a0 + a1) + (a2 + a3)) / len + id row).  How many token rows a lane has in flight is not part
of it.  The bias output sums its tokens across lanes and is held to the float64 oracle at the tolerance of
tests/test_kernels_gpu.py, and has to be equal between the entry points."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-4                      # tests/test_kernels_gpu.py
ATOL = 1e-5
N_TOK = 300
ROWS_IN_FLIGHT = 8               # kBagNF
EMPTY_BIAS = np.float32(-1e30)   # kEmptySlotBias
SCALE = 0.3                      # not a power of two: the last multiply rounds


def _lpr(d):
    n, p = (d + 3) // 4, 1
    while p < n:
        p *= 2
    return p


def _bag_lengths(d, case):
    if case == "ones":
        return np.ones(40, dtype=np.int32)
    if case == "nf":
        return np.full(40, ROWS_IN_FLIGHT, dtype=np.int32)
    top = min(2 * _lpr(d) + 9, 73)                  # every length, twice: all residues mod 4 and mod 8, LPR, LPR +- 1,
    return np.repeat(np.arange(1, top + 1), 2).astype(np.int32)     # 2 LPR +- 1 and a third block


def _model_sum(T, toks, lpr):
    acc = np.zeros((4, T.shape[1]), dtype=np.float32)
    for j0 in range(0, len(toks), lpr):
        cnt = min(lpr, len(toks) - j0)
        full = cnt & ~3
        for t in range(full):
            acc[t % 4] += T[toks[j0 + t]]
        for t in range(full, cnt):
            acc[0] += T[toks[j0 + t]]
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


@functools.lru_cache(maxsize=None)
def _case(d, case):
    """Inputs, the float32 model rows and the float64 oracle of one (d, case); computed once, read only."""
    rng = np.random.default_rng(1000 * d + len(case))
    lens = _bag_lengths(d, case)
    rng.shuffle(lens)
    n = len(lens)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    vals = rng.integers(0, N_TOK, size=int(lens.sum())).astype(np.int32)
    T = rng.standard_normal((N_TOK, d)).astype(np.float32)
    bT = rng.standard_normal(N_TOK).astype(np.float32)
    I = rng.standard_normal((n, d)).astype(np.float32)
    bI = rng.standard_normal(n).astype(np.float32)
    cmap = rng.permutation(n).astype(np.int32)
    lpr, sc = _lpr(d), np.float32(SCALE)
    mean = np.empty((n, d), dtype=np.float32)
    mean64, bias64 = np.empty((n, d)), np.empty(n)
    for e in range(n):
        toks = vals[starts[e]:starts[e] + lens[e]]
        mean[e] = _model_sum(T, toks, lpr) / np.float32(lens[e])
        mean64[e] = T[toks].astype(np.float64).sum(0) / lens[e]
        bias64[e] = bT[toks].astype(np.float64).sum() / lens[e]
    zero = np.zeros((1, d), dtype=np.float32)
    out = dict(n=n, lens=lens, starts=starts, vals=vals, T=T, bT=bT, I=I, bI=bI, cmap=cmap,
               bag=sc * (mean + zero), het=sc * (mean + I[cmap]), onehot=sc * I[cmap],
               bag64=SCALE * mean64, bag_b64=SCALE * bias64, het_b64=SCALE * (bias64 + bI[cmap].astype(np.float64)),
               onehot_b=sc * bI[cmap])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _bits_equal(got, want_np, what):
    import torch
    want = torch.from_numpy(np.array(want_np)).to(got.device)
    assert torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32)), what


@pytest.mark.parametrize("case", ["sweep", "ones", "nf"])
@pytest.mark.parametrize("d", [128, 64, 32, 20, 16, 4])
def test_bag_sum_order(dev, d, case):
    import torch
    from arx import ops
    c = _case(d, case)
    n = c["n"]
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)          # (a copy: the shared case is read-only)
    T, bT, I, bI, cmap = t(c["T"]), t(c["bT"]), t(c["I"]), t(c["bI"]), t(c["cmap"])
    vals, starts, lens = t(c["vals"]), t(c["starts"]), t(c["lens"])
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    new = lambda rows, *w: torch.full((rows,) + w, -7.5, dtype=torch.float32, device=dev)

    # K1: the bag mean alone
    k1, k1_b = new(n, d), new(n)
    ops.gather_mulhot_mean(T, bT, vals, starts, lens, ids, k1, scale=SCALE, bias_out=k1_b)
    _bits_equal(k1, c["bag"], "gather_mulhot_mean")
    np.testing.assert_allclose(k1_b.cpu().numpy(), c["bag_b64"], rtol=RTOL, atol=ATOL)

    # K1 with the id row
    ib, ib_b = new(n, d), new(n)
    ops.gather_id_plus_bag(I, bI, cmap, T, bT, vals, starts, lens, ids, ib, scale=SCALE, bias_out=ib_b)
    _bits_equal(ib, c["het"], "gather_id_plus_bag")
    np.testing.assert_allclose(ib_b.cpu().numpy(), c["het_b64"], rtol=RTOL, atol=ATOL)

    # the step's lookup launch: a one-hot site, a bag-only site, an id + bag site, an empty site
    rng = np.random.default_rng(d)
    i_one = rng.integers(0, n, size=5).astype(np.int32)
    i_bag = rng.integers(0, n, size=37).astype(np.int32)
    i_het = np.concatenate([np.arange(n), rng.integers(0, n, size=301 - n)]).astype(np.int32)
    hole = 17                                        # an EMPTY slot: a zero row, bias kEmptySlotBias
    i_het[hole] = -1
    o_one, b_one = new(5, d), new(5)
    o_bag, b_bag = new(37, d), new(37)
    o_het, b_het = new(301, d), new(301)
    o_none, b_none = new(1, d)[:0], new(1)[:0]
    none = torch.empty((0,), dtype=torch.int32, device=dev)
    ops.lookup_multi(ops.LookupSet([
        (I, bI, cmap, None, None, None, None, None, t(i_one), o_one, SCALE, b_one),
        (None, None, None, T, bT, vals, starts, lens, t(i_bag), o_bag, SCALE, b_bag),
        (I, bI, cmap, T, bT, vals, starts, lens, t(i_het), o_het, SCALE, b_het),
        (I, bI, cmap, T, bT, vals, starts, lens, none, o_none, SCALE, b_none)]))
    _bits_equal(o_one, c["onehot"][i_one], "lookup_multi, one-hot site")
    _bits_equal(b_one, c["onehot_b"][i_one], "lookup_multi, one-hot site, bias")
    _bits_equal(o_bag, c["bag"][i_bag], "lookup_multi, bag-only site")
    want = c["het"][np.maximum(i_het, 0)].copy()
    want[hole] = 0.0
    _bits_equal(o_het, want, "lookup_multi, id + bag site")
    live = i_het >= 0
    assert b_het[hole].item() == EMPTY_BIAS
    # the bias: equal between the entry points, and held to the float64 oracle above
    assert torch.equal(b_bag, k1_b[t(i_bag).long()])
    assert torch.equal(b_het[t(live)], ib_b[t(i_het[live]).long()])

    # the serving rows of the sharded HET view, world 1: item c is entity c, its id row is row c of the shard
    hv, hv_b = new(n, d), new(n)
    ops.het_rows_range(t(c["I"][c["cmap"]]), t(c["bI"][c["cmap"]]), T, bT, vals, starts, lens, n, 1, 0, 0, n, hv,
                       bias_out=hv_b, scale=SCALE)
    _bits_equal(hv, c["het"], "het_rows_range")
    assert torch.equal(hv_b, ib_b)

    # accumulate: a fused multiply-add may differ from the model, the oracle's tolerance holds
    acc = torch.full((n, d), 1.0, dtype=torch.float32, device=dev)
    ops.gather_mulhot_mean(T, None, vals, starts, lens, ids, acc, scale=SCALE, accumulate=True)
    np.testing.assert_allclose(acc.cpu().numpy(), 1.0 + c["bag64"], rtol=RTOL, atol=ATOL)
