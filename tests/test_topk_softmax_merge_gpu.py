"""arx_topk_softmax_merge_shards (ops.topk_softmax_merge_shards) against a numpy float64 merge: the W-way merge of
per-shard top-k lists of GLOBAL logit ids by (value desc, id asc) -- tf.nn.top_k's rule -- with the winners' softmax
values exp(v - lse) and the row's lse = logsumexp over the shards' parts.  Inputs carry trailing empties, empties in
the middle of a list, a shard whose whole list is empty (lse part -inf), a row in which every shard is empty (ids -1,
values 0, lse -inf, no NaN), equal values on different shards (the lower id first), -inf values at list ends, and ids
that are no c * W + s.  io is exact (values are selected, not computed); lse_out: RTOL 1e-4 / ATOL 1e-5 (what
tests/test_gemm_nt_fused_gpu.py grants arx_row_logsumexp); po: rtol 1e-4, atol 1e-9 (what test_seq_step_recommend
holds softmax values to)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LSE_RTOL, LSE_ATOL = 1e-4, 1e-5
P_RTOL, P_ATOL = 1e-4, 1e-9


def _inputs(W, B, k, seed):
    rng = np.random.default_rng(seed)
    # values from a coarse grid: equal values on different shards are common; a few -inf
    v = (rng.integers(-40, 41, size=(W, B, k)) / 8.0).astype(np.float32)
    v[rng.random((W, B, k)) < 0.02] = -np.inf
    # ids: distinct within a row, in no relation to (column, shard)
    ids = np.empty((W, B, k), dtype=np.int32)
    for r in range(B):
        ids[:, r, :] = (rng.permutation(3 * W * k)[:W * k] + 1000).reshape(W, k)
    o = np.lexsort((ids, -v), axis=-1)                       # every list: value desc, id asc
    v, ids = np.take_along_axis(v, o, -1), np.take_along_axis(ids, o, -1)
    tail = rng.integers(0, k + 1, size=(W, B))               # trailing empties (k: the whole list)
    ids[np.arange(k)[None, None, :] >= (k - tail)[:, :, None]] = -1
    ids[rng.random((W, B, k)) < 0.1] = -1                    # empties in the middle
    with np.errstate(over='ignore', divide='ignore'):
        part = np.log(np.exp(v.astype(np.float64)).sum(-1)) + rng.random((W, B))
    part = part.astype(np.float32)
    s0 = W // 2
    ids[s0, 0, :] = -1                                       # row 0: shard s0 holds nothing
    part[s0, 0] = -np.inf
    if B > 1:
        ids[:, B - 1, :] = -1                                # the last row: every shard is empty
        part[:, B - 1] = -np.inf
    if W > 1 and B > 2:                                      # row 1: one value everywhere -- pure id order across shards
        v[:, 1, :] = 0.5
        for s in range(W):
            m = ids[s, 1, :] >= 0
            ids[s, 1, m] = np.sort(ids[s, 1, m])
    return v, ids, part


def _expected(v, ids, part, k):
    W, B, _ = v.shape
    io = np.full((B, k), -1, dtype=np.int32)
    po = np.zeros((B, k), dtype=np.float64)
    lse = np.full(B, -np.inf, dtype=np.float64)
    for r in range(B):
        p = part[:, r].astype(np.float64)
        mx = p.max()
        if np.isfinite(mx):
            lse[r] = mx + np.log(np.exp(p - mx).sum())
        vv, ii = v[:, r, :].reshape(-1).astype(np.float64), ids[:, r, :].reshape(-1)
        keep = ii >= 0
        vv, ii = vv[keep], ii[keep]
        o = np.lexsort((ii, -vv))[:k]
        vv, ii = vv[o], ii[o]
        ok = ~np.isneginf(vv)
        io[r, :len(o)] = np.where(ok, ii, -1)
        po[r, :len(o)] = np.where(ok, np.exp(np.where(ok, vv, 0.0) - lse[r]), 0.0)
    return io, po, lse


@pytest.mark.parametrize("W", [1, 2, 3, 64])
@pytest.mark.parametrize("k", [1, 7, 100, 1024])
def test_topk_softmax_merge_shards_matches_numpy(dev, W, k):
    import torch
    from arx import ops
    for B in (1, 5, 67):                                      # 67: no multiple of the four rows of a block
        v, ids, part = _inputs(W, B, k, seed=1000 * W + k + B)
        io_e, po_e, lse_e = _expected(v, ids, part, k)
        po = torch.full((B, k), float('nan'), dtype=torch.float32, device=dev)
        io = torch.full((B, k), -7, dtype=torch.int32, device=dev)
        lse = torch.full((B,), float('nan'), dtype=torch.float32, device=dev)
        ops.topk_softmax_merge_shards(torch.from_numpy(v).to(dev), torch.from_numpy(ids).to(dev),
                                      torch.from_numpy(part).to(dev), po, io, lse)
        io_g, po_g, lse_g = io.cpu().numpy(), po.cpu().numpy(), lse.cpu().numpy()
        assert not np.isnan(po_g).any() and not np.isnan(lse_g).any(), (W, B, k)
        np.testing.assert_array_equal(io_g, io_e, err_msg='ids W %d B %d k %d' % (W, B, k))
        fin = np.isfinite(lse_e)
        np.testing.assert_array_equal(np.isneginf(lse_g), ~fin)
        np.testing.assert_allclose(lse_g[fin], lse_e[fin], rtol=LSE_RTOL, atol=LSE_ATOL)
        np.testing.assert_allclose(po_g, po_e, rtol=P_RTOL, atol=P_ATOL, err_msg='values W %d B %d k %d' % (W, B, k))
        assert (po_g[io_g < 0] == 0).all()
        if B > 1:                                             # the all-empty row
            assert (io_g[B - 1] == -1).all() and (po_g[B - 1] == 0).all() and np.isneginf(lse_g[B - 1])
        # lse_out is optional: same winners without it
        io2 = torch.empty_like(io)
        po2 = torch.empty_like(po)
        ops.topk_softmax_merge_shards(torch.from_numpy(v).to(dev), torch.from_numpy(ids).to(dev),
                                      torch.from_numpy(part).to(dev), po2, io2)
        np.testing.assert_array_equal(io2.cpu().numpy(), io_g)
        np.testing.assert_array_equal(po2.cpu().numpy(), po_g)


def test_topk_softmax_merge_shards_wrapper_checks(dev):
    import torch
    from arx import ops
    W, B, k = 2, 3, 4
    f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)
    i = lambda *sh: torch.zeros(sh, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ops.topk_softmax_merge_shards(f(W, B, k), i(W, B, k), f(W, B + 1), f(B, k), i(B, k))
    with pytest.raises(ValueError):
        ops.topk_softmax_merge_shards(f(W, B, k), i(W, B, k), f(W, B), f(B, k + 1), i(B, k))
    with pytest.raises(ValueError):
        ops.topk_softmax_merge_shards(f(W, B, 2 * k)[:, :, ::2], i(W, B, k), f(W, B), f(B, k), i(B, k))
    with pytest.raises(ValueError):
        ops.topk_softmax_merge_shards(f(W, B, k), f(W, B, k), f(W, B), f(B, k), i(B, k))
    ops.topk_softmax_merge_shards(f(W, 0, k), i(W, 0, k), f(W, 0), f(0, k), i(0, k))      # zero rows: a no-op
