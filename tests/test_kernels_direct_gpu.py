"""Direct parity tests for the kernels that the whole-model tests alone used to reach (test_kernels_gpu.py holds
the others): every kernel is called through its arx.ops wrapper on seeded fp32 inputs and compared with an fp64
numpy restatement of the same operation (the oracle where it states the op), at the shapes where such kernels
go wrong: past a 256-thread stride, a second chunk, a 32-bit mask word, an LDS limit, a tile edge.

Tolerances are test_kernels_gpu.py's (RTOL 1e-4, ATOL 1e-5); integer outputs, copies, fills, transposes, gathers,
dropout masks and arg-max positions are bit-exact; long sums with cancellation (GEMM results, dots, norms) use the
scale-relative GEMM bound of test_gemm_nt_scorer_shape, |err| <= 2e-6 * sum|a||b| + 1e-5."""
import numpy as np
import pytest

from oracle import ref_graph as rg

pytestmark = pytest.mark.gpu

RTOL = 1e-4
ATOL = 1e-5


def _t(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _mask(rng, B, W, p=0.05):
    return (rng.random((B, W)) > p)


def _oracle():
    e = rg.RefEmbeddingAttribute.__new__(rg.RefEmbeddingAttribute)
    e.dt = np.dtype(np.float64)
    return e


def _grid(rng, shape, lim=4.0):
    """fp32 values on the grid of multiples of 2^-8 in [-lim, lim]: x - t + 1 is exact in fp32, so the hinge
    of the rs kinds has the same active set in fp32 and fp64."""
    n = int(lim * 256)
    return (rng.integers(-n, n + 1, size=shape) / 256.0).astype(np.float32)


def _wide(dev, rows, cols, fill, off=4, pad=8):
    """A [rows, cols] view (leading dimension cols + pad) into a canary-filled wider tensor."""
    import torch
    base = torch.full((rows, cols + pad), float(fill), dtype=torch.float32, device=dev)
    return base, base[:, off:off + cols]


def _canary_ok(base, cols, fill, off=4):
    b = base.cpu().numpy()
    return bool(np.all(b[:, :off] == fill) and np.all(b[:, off + cols:] == fill))


def _scale_bound(err, scale):
    assert np.all(err <= 2e-6 * scale + 1e-5), float((err / (scale + 1e-9)).max())


# ---------------------------------------------------------------------------------------------------------
# 1. rs-family loss
# ---------------------------------------------------------------------------------------------------------
RS_EXP_P = {'log': 1.005, 'exp': 1.3, 'poly': 1.2, 'poly2': 0.7, 'linear': 1.005, 'square': 1.005}


def _pow2_gscale(dl):
    """A power of two near 1 / max|dl| (never 1.0): the non-target gradients of the steepest row are O(1)."""
    m = float(np.max(np.abs(dl)))
    k = int(np.clip(-np.ceil(np.log2(m)) if m > 0 else 0, -60, 60))
    return float(2.0 ** (k if k != 0 else -1))


def _rs_reference(logits, tgt, kind, func, keep, row_w):
    """fp64 oracle -> ((loss, dlogits, per-row gradient factor g_r = gscale * row_w * dl), gscale); asserts that no
    kept column sits within 1e-6 of the hinge."""
    e = _oracle()
    x = logits.astype(np.float64)
    B = x.shape[0]
    if kind in ('rs', 'rs-sig'):
        pre = np.abs(x - x[np.arange(B), tgt].reshape(B, 1) + 1)
        assert not np.any(keep & (pre > 0) & (pre < 1e-6))
    bl, cache = e.compute_loss(x, tgt, kind, keep, loss_func=func, exp_p=RS_EXP_P[func])
    gscale = _pow2_gscale(cache['dl'])
    w = np.ones(B) if row_w is None else row_w.astype(np.float64)
    dl, _ = e.compute_loss_bwd(cache, gscale * w)
    return (bl, dl, np.abs(gscale * w * cache['dl'])), gscale


def _check_rs(got, ref, tgt):
    """loss at RTOL / ATOL.  Gradient d[r, c] = g_r * err'(r, c), the target column -(row sum): RTOL plus an
    absolute term of 5e-7 * g_r (never above ATOL: gscale keeps g_r <= 1).  The absolute term is what fp32 owes:
    err' <= 1 is formed from O(1) intermediates, and err (1 - err) or sg (1 - sg) loses about 2^-24 ABSOLUTELY,
    not relatively, where a sigmoid saturates; 5e-7 is eight such roundings."""
    (got_l, got_d), (bl, dl, grow) = got, ref
    if got_l is not None:
        np.testing.assert_allclose(got_l, bl, rtol=RTOL, atol=ATOL)
    if got_d is not None:
        atol = np.minimum(ATOL, 5e-7 * grow).reshape(-1, 1) + 1e-30
        err = np.abs(got_d.astype(np.float64) - dl)
        tol = RTOL * np.abs(dl) + atol
        assert np.all(err <= tol), (float((err / tol).max()), np.argwhere(err > tol)[:4].tolist())


def _run_rs(dev, logits, tgt, kind, func, gscale, mask=None, mask_rows=0, pos=None, row_w=None, strided=False,
            want_loss=True, want_grad=True):
    from arx import ops
    import torch
    B, V = logits.shape
    if strided:
        lbase, L = _wide(dev, B, V, 0.0)
        L.copy_(_t(dev, logits))
        dbase, D = _wide(dev, B, V, 7.0)
    else:
        L = _t(dev, logits)
        D = torch.full((B, V), 7.0, dtype=torch.float32, device=dev)
    out_l = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
    ops.loss_rs(L, _t(dev, tgt), kind, func, RS_EXP_P[func], out_l if want_loss else None,
                D if want_grad else None, gscale, mask=None if mask is None else _t(dev, mask.astype(np.uint8)),
                pos=pos, row_w=None if row_w is None else _t(dev, row_w), mask_rows=mask_rows)
    torch.cuda.synchronize()
    if strided:
        assert _canary_ok(dbase, V, 7.0)
    return (out_l.cpu().numpy() if want_loss else None), (D.cpu().numpy() if want_grad else None)


@pytest.mark.parametrize("kind", ['rs', 'rs-sig', 'rs-sig2', 'bbpr'])
@pytest.mark.parametrize("func", ['log', 'exp', 'poly', 'poly2', 'linear', 'square'])
def test_loss_rs_every_kind_and_transform(dev, kind, func):
    """All kinds x loss_funcs at (33, 257): one column past the 256-thread stride, nine mask words.  Logits in
    [-1, 1] and 70 % of the columns masked keep s below ~200, so 'exp' (1.3^-s) stays a normal fp32 number."""
    rng = np.random.default_rng(len(kind) * 10 + len(func))
    B, V = 33, 257
    logits = _grid(rng, (B, V), 1.0)
    tgt = rng.integers(0, V, size=B).astype(np.int32)
    keep = _mask(rng, B, V, p=0.7)
    row_w = (rng.integers(1, 9, size=B) / 8.0).astype(np.float32)
    ref, gs = _rs_reference(logits, tgt, kind, func, keep, row_w)
    _check_rs(_run_rs(dev, logits, tgt, kind, func, gs, mask=keep, row_w=row_w), ref, tgt)


def _pos_csr(rng, n_users, n_items, lens):
    ptr = np.zeros(n_users + 1, dtype=np.int32)
    items = []
    for u in range(n_users):
        n = min(int(lens[u % len(lens)]), n_items)
        items.extend(rng.choice(n_items, size=n, replace=False).tolist())
        ptr[u + 1] = len(items)
    return ptr, np.asarray(items if items else [0], dtype=np.int32)


def _csr_keep(users, ptr, items, item2slot, rows, V):
    """The keep-mask the positives CSR stands for: [rows, V] bool, False at every positive that has a column."""
    keep = np.ones((rows, V), dtype=bool)
    for r in range(rows):
        u = users[r]
        for it in items[ptr[u]:ptr[u + 1]]:
            if item2slot[it] >= 0:
                keep[r, item2slot[it]] = False
    return keep


RS_SUBSET = [('rs', 'log'), ('rs-sig', 'linear'), ('rs-sig2', 'poly'), ('bbpr', 'log')]


@pytest.mark.parametrize("kind,func", RS_SUBSET)
@pytest.mark.parametrize("B,V", [(64, 3100), (7, 50), (33, 257), (5, 9001), (3, 1), (2, 31), (2, 33)])
def test_loss_rs_shapes_and_mask_forms(dev, B, V, kind, func):
    """Shape sweep x the four mask forms: mask array (k_loss_rs<false>), mask array with mask_rows = B // 2,
    no mask, and the positives CSR (k_loss_rs<true>: LDS bit mask) against the mask the same CSR stands for --
    users without positives, positives without a column, a positive listed twice."""
    from arx import ops
    import torch
    rng = np.random.default_rng(B * 131 + V)
    logits = _grid(rng, (B, V))
    tgt = rng.integers(0, V, size=B).astype(np.int32)
    row_w = (rng.integers(1, 9, size=B) / 8.0).astype(np.float32)
    # mask array, one row per batch row; logits / dlogits as column slices of wider tensors
    keep = _mask(rng, B, V, p=0.3)
    ref, gs = _rs_reference(logits, tgt, kind, func, keep, row_w)
    _check_rs(_run_rs(dev, logits, tgt, kind, func, gs, mask=keep, row_w=row_w, strided=True), ref, tgt)
    # loss only / gradient only
    got_l, none_d = _run_rs(dev, logits, tgt, kind, func, gs, mask=keep, row_w=row_w, want_grad=False)
    assert none_d is None
    _check_rs((got_l, None), ref, tgt)
    none_l, got_d = _run_rs(dev, logits, tgt, kind, func, gs, mask=keep, row_w=row_w, want_loss=False)
    assert none_l is None
    _check_rs((None, got_d), ref, tgt)
    # mask_rows = B // 2: row r uses mask row r % mask_rows
    mr = B // 2
    keep2 = _mask(rng, mr, V, p=0.3)
    full2 = keep2[np.arange(B) % mr]
    ref, gs = _rs_reference(logits, tgt, kind, func, full2, None)
    _check_rs(_run_rs(dev, logits, tgt, kind, func, gs, mask=keep2, mask_rows=mr), ref, tgt)
    # no mask
    ref, gs = _rs_reference(logits, tgt, kind, func, np.ones((B, V), dtype=bool), None)
    _check_rs(_run_rs(dev, logits, tgt, kind, func, gs), ref, tgt)
    # positives CSR
    n_users, n_items = B + 3, V + 40
    ptr, items = _pos_csr(rng, n_users, n_items, [0, 3, 17, 1, 70])
    for u in range(n_users):                                   # a positive listed twice
        if ptr[u + 1] - ptr[u] >= 3:
            items[ptr[u] + 2] = items[ptr[u]]
    item2slot = np.full(n_items, -1, dtype=np.int32)
    item2slot[rng.permutation(n_items)[:V]] = np.arange(V, dtype=np.int32)    # 40 items have no column
    users = rng.integers(0, n_users, size=B).astype(np.int32)
    users[0] = 0                                               # a user with no positives
    keep3 = _csr_keep(users, ptr, items, item2slot, B, V)
    dmask = torch.ones((B, V), dtype=torch.uint8, device=dev)
    csr = (_t(dev, users), _t(dev, ptr), _t(dev, items), _t(dev, item2slot))
    ops.pos_mask_scatter(*csr, dmask, 0)
    np.testing.assert_array_equal(dmask.cpu().numpy().astype(bool), keep3)
    ref, gs = _rs_reference(logits, tgt, kind, func, keep3, row_w)
    _check_rs(_run_rs(dev, logits, tgt, kind, func, gs, pos=csr, row_w=row_w, strided=True), ref, tgt)
    _check_rs(_run_rs(dev, logits, tgt, kind, func, gs, mask=keep3, row_w=row_w), ref, tgt)


@pytest.mark.parametrize("kind,func", [('rs', 'log'), ('rs-sig2', 'poly')])
def test_loss_rs_csr_mask_bits_above_48k(dev, kind, func):
    """V = 400 000: 50 000 bytes of mask bits, the dynamic-LDS opt-in branch; positives at both ends of the mask."""
    rng = np.random.default_rng(4)
    B, V = 2, 400000
    logits = _grid(rng, (B, V))
    tgt = np.array([17, V - 1], dtype=np.int32)
    n_items = V + 10
    item2slot = np.full(n_items, -1, dtype=np.int32)
    item2slot[:V] = rng.permutation(V).astype(np.int32)
    inv = np.argsort(item2slot[:V])                            # column -> item
    planted = inv[[0, 31, 32, 393215, 393216, V - 2, V - 1]]
    lists = [np.concatenate([planted, rng.choice(n_items, size=500, replace=False)]),
             rng.choice(n_items, size=3000, replace=False)]
    ptr = np.array([0, len(lists[0]), len(lists[0]) + len(lists[1])], dtype=np.int32)
    items = np.concatenate(lists).astype(np.int32)
    users = np.array([0, 1], dtype=np.int32)
    keep = _csr_keep(users, ptr, items, item2slot, B, V)
    assert not keep[0, V - 1] and not keep[0, 393216] and keep.sum() < B * V - 3000
    ref, gs = _rs_reference(logits, tgt, kind, func, keep, None)
    csr = tuple(_t(dev, a) for a in (users, ptr, items, item2slot))
    _check_rs(_run_rs(dev, logits, tgt, kind, func, gs, pos=csr), ref, tgt)


def test_loss_rs_csr_refuses_more_than_2_20_columns(dev):
    from arx import ops
    from arx._lib import ArxError
    import torch
    V = (1 << 20) + 1
    assert V == ops.POS_MASK_MAX_COLS + 1
    L = torch.zeros((1, V), dtype=torch.float32, device=dev)
    z = torch.zeros(4, dtype=torch.int32, device=dev)
    out = torch.zeros(1, dtype=torch.float32, device=dev)
    with pytest.raises(ArxError, match=r"\(-4\).*exceed the LDS mask"):           # ARX_EUNSUPPORTED
        ops.loss_rs(L, z[:1], 'rs', 'log', 1.005, out, None, 1.0, pos=(z[:1], z[:2], z[:1], z))
    ops.loss_rs(L, z[:1], 'rs', 'log', 1.005, out, None, 1.0)                    # the mask-array form takes it
    np.testing.assert_allclose(out.item(), np.log1p(float(V)), rtol=RTOL)


# ---------------------------------------------------------------------------------------------------------
# 2. ce, log-sum-exp, warp_eval, the bad-target contract
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("V", [4095, 4096, 4097, 9001])
def test_loss_ce_both_kernels(dev, V, scale):
    """k_loss_ce_regs (V <= 4096) and k_loss_ce on both sides of the switch; row weights, strided dlogits, and
    logits scaled by 30 (exp overflows without the max subtraction)."""
    from arx import ops
    import torch
    rng = np.random.default_rng(V)
    B = 9
    logits = (rng.standard_normal((B, V)) * scale).astype(np.float32)
    tgt = rng.integers(0, V, size=B).astype(np.int32)
    tgt[0], tgt[1] = V - 1, 0
    row_w = rng.random(B).astype(np.float32)
    e = _oracle()
    bl, cache = e.compute_loss(logits.astype(np.float64), tgt, 'ce')
    dl, _ = e.compute_loss_bwd(cache, 0.5 * row_w.astype(np.float64))
    out_l = torch.empty(B, dtype=torch.float32, device=dev)
    dbase, D = _wide(dev, B, V, 7.0)
    ops.loss_ce(_t(dev, logits), _t(dev, tgt), out_l, D, 0.5, row_w=_t(dev, row_w))
    got_l, got_d = out_l.cpu().numpy(), D.cpu().numpy()
    assert np.all(np.isfinite(got_l)) and np.all(np.isfinite(got_d))
    np.testing.assert_allclose(got_l, bl, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got_d, dl, rtol=RTOL, atol=1e-7)
    assert _canary_ok(dbase, V, 7.0)


def _lse64(x):
    x = x.astype(np.float64)
    m = x.max(1, keepdims=True)
    return (np.log(np.exp(x - m).sum(1, keepdims=True)) + m)[:, 0]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("V", [1, 63, 256, 257, 4097, 100003])
def test_row_logsumexp(dev, B, V):
    from arx import ops
    import torch
    rng = np.random.default_rng(B * 7 + V)
    x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    x[0, :] = 1.25                                             # a constant row: lse = 1.25 + log V
    if B > 1:
        x[1, :] = -80.0                                        # one +80 among -80s
        x[1, V // 2] = 80.0
    base, X = _wide(dev, B, V, 50.0, off=3, pad=5)             # strided input; the canaries would dominate the sum
    X.copy_(_t(dev, x))
    out = torch.empty(B, dtype=torch.float32, device=dev)
    ops.row_logsumexp(X, out)
    np.testing.assert_allclose(out.cpu().numpy(), _lse64(x), rtol=RTOL, atol=ATOL)
    out2 = torch.empty(B, dtype=torch.float32, device=dev)
    ops.row_logsumexp(_t(dev, x), out2)
    np.testing.assert_array_equal(out2.cpu().numpy(), out.cpu().numpy())


def _bad_target_case(rng, B, V):
    logits = _grid(rng, (B, V))
    tgt = rng.integers(0, V, size=B).astype(np.int32)
    bad = np.zeros(B, dtype=bool)
    bad[[1, 4]] = True
    tbad = tgt.copy()
    tbad[1], tbad[4] = -1, V
    return logits, tgt, tbad, bad


def _assert_bad_rows(l_bad, d_bad, l_ok, d_ok, bad, dbase, V):
    """bad rows: NaN loss, all-zero gradient row; good rows: bit-identical to the run without bad rows (rows are
    independent workgroups / waves); the canary columns around dlogits untouched."""
    assert np.all(np.isnan(l_bad[bad]))
    assert np.all(d_bad[bad] == 0)
    np.testing.assert_array_equal(l_bad[~bad], l_ok[~bad])
    np.testing.assert_array_equal(d_bad[~bad], d_ok[~bad])
    assert _canary_ok(dbase, V, 7.0)


@pytest.mark.parametrize("name,V", [('warp', 3100), ('warp', 1000), ('warp_pos', 3100), ('warp_pos', 1000),
                                    ('ce', 3100), ('ce', 4097), ('rs', 3100), ('rs_pos', 257), ('rs-sig2', 50)])
def test_bad_target_rows_are_nan_and_write_nothing(dev, name, V):
    """The documented contract of a target without a logit column (tcol < 0 or tcol >= V): the row's loss is NaN,
    its gradient row zero, nothing is read or written through the bad index.  V = 1000 takes the wave-per-row
    margin kernel, V = 3100 the workgroup-per-row one."""
    from arx import ops
    import torch
    rng = np.random.default_rng(V + len(name))
    B = 6
    logits, tgt, tbad, bad = _bad_target_case(rng, B, V)
    keep = _mask(rng, B, V, p=0.3)
    n_items = V + 5
    ptr, items = _pos_csr(rng, B, n_items, [0, 5, 30])
    item2slot = np.full(n_items, -1, dtype=np.int32)
    item2slot[:V] = rng.permutation(V).astype(np.int32)
    csr = tuple(_t(dev, a) for a in (np.arange(B, dtype=np.int32), ptr, items, item2slot))

    def run(t):
        out_l = torch.full((B,), 3.0, dtype=torch.float32, device=dev)
        dbase, D = _wide(dev, B, V, 7.0)
        L, T, M = _t(dev, logits), _t(dev, t), _t(dev, keep.astype(np.uint8))
        if name == 'warp':
            ops.loss_warp(L, T, M, out_l, D, 0.25)
        elif name == 'warp_pos':
            ops.loss_warp_pos(L, T, *csr, out_l, D, 0.25)
        elif name == 'ce':
            ops.loss_ce(L, T, out_l, D, 0.25)
        elif name == 'rs_pos':
            ops.loss_rs(L, T, 'rs', 'log', 1.005, out_l, D, 0.25, pos=csr)
        else:
            ops.loss_rs(L, T, name, 'log', 1.005, out_l, D, 0.25, mask=M)
        torch.cuda.synchronize()
        return out_l.cpu().numpy(), D.cpu().numpy(), dbase

    l_ok, d_ok, _ = run(tgt)
    assert np.all(np.isfinite(l_ok))
    l_bad, d_bad, dbase = run(tbad)
    _assert_bad_rows(l_bad, d_bad, l_ok, d_ok, bad, dbase, V)


@pytest.mark.parametrize("B,V", [(64, 3100), (6, 257), (5, 9001)])
def test_warp_eval_parity_and_bad_targets(dev, B, V):
    """k_warp_eval against the oracle (mask array, mask_rows, no mask), and its bad-target convention: margin_rank
    NaN and true_rank -1 for a target without a logit column, every other row unchanged."""
    from arx import ops
    import torch
    rng = np.random.default_rng(B + V)
    logits, tgt, tbad, bad = _bad_target_case(rng, B, V)
    e = _oracle()
    mr = B // 2
    keep2 = _mask(rng, mr, V, p=0.3)
    forms = [(_mask(rng, B, V, p=0.3), 0), (keep2, mr), (None, 0)]
    for keep, mrows in forms:
        full = np.ones((B, V), dtype=bool) if keep is None else keep[np.arange(B) % keep.shape[0]]
        ref_m, ref_t = e.warp_eval(logits.astype(np.float64), tgt, full)
        M = None if keep is None else _t(dev, keep.astype(np.uint8))
        outs = []
        for t in (tgt, tbad):
            o_m = torch.full((B,), 3.0, dtype=torch.float32, device=dev)
            o_t = torch.full((B,), 3, dtype=torch.int32, device=dev)
            ops.loss_warp_eval(_t(dev, logits), _t(dev, t), M, o_m, o_t, mask_rows=mrows)
            outs.append((o_m.cpu().numpy(), o_t.cpu().numpy()))
        np.testing.assert_allclose(outs[0][0], ref_m, rtol=RTOL, atol=ATOL)
        np.testing.assert_array_equal(outs[0][1], ref_t)
        assert np.all(np.isnan(outs[1][0][bad])) and np.all(outs[1][1][bad] == -1)
        np.testing.assert_array_equal(outs[1][0][~bad], outs[0][0][~bad])
        np.testing.assert_array_equal(outs[1][1][~bad], outs[0][1][~bad])


# ---------------------------------------------------------------------------------------------------------
# 3. streaming eval chain
# ---------------------------------------------------------------------------------------------------------
def _eval_chain(dev, Ld, tscore, mode, chunks, views=True, unmask=None):
    """eval_chunk_accum over the column chunks of the device logits Ld, optional eval_warp_unmask, eval_finish."""
    from arx import ops
    import torch
    B = Ld.shape[0]
    acc0 = torch.full((B,), 9.0, dtype=torch.float32, device=dev)
    acc1 = torch.full((B,), 9.0, dtype=torch.float32, device=dev)
    c0 = 0
    for k, n in enumerate(chunks):
        ch = Ld[:, c0:c0 + n]
        ops.eval_chunk_accum(ch if views else ch.contiguous(), tscore, mode, k == 0, acc0, acc1)
        c0 += n
    assert c0 == Ld.shape[1]
    if unmask is not None:
        U, P, pb, csr, mrows = unmask
        ops.eval_warp_unmask(U, P, pb, tscore, *csr, acc0, mask_rows=mrows)
    out = torch.empty(B, dtype=torch.float32, device=dev)
    ops.eval_finish(mode, acc0, acc1, tscore, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


EVAL_CHUNKINGS = [[1000], [96] * 10 + [40], [1, 999], [999, 1]]


@pytest.mark.parametrize("B,d", [(1, 4), (3, 32), (4, 64), (5, 128), (257, 256), (5, 256), (257, 32)])
def test_eval_chain_ce_and_warp(dev, B, d):
    """L = U P^T + pbias cut into ragged chunks: 'ce' (online log-sum-exp) and 'warp' with the positives taken
    out again by k_eval_unmask -- users with 0 / 1 / 64 / 65 / 200 positives (second batch of 64), a positive
    named twice within a batch and across batches, positives without a column, the target among the positives,
    mask_rows = B // 2.  Every chunking agrees with the single chunk and with fp64; the same formula in fp32
    numpy meets RTOL too, which shows the bound has margin for this data."""
    from arx import ops
    import torch
    rng = np.random.default_rng(B * 1000 + d)
    V = 1000
    U = (rng.standard_normal((B, d)) / d ** 0.25).astype(np.float32)
    P = (rng.standard_normal((V, d)) / d ** 0.25).astype(np.float32)
    pb = (rng.standard_normal(V) * 0.1).astype(np.float32)
    Ud, Pd, pbd = _t(dev, U), _t(dev, P), _t(dev, pb)
    Ld = torch.empty((B, V), dtype=torch.float32, device=dev)
    ops.gemm(Ud, Pd, Ld, ops.Workspace(dev), transB=True, col_bias=pbd)
    # positives
    n_users, n_items = 5, V + 100
    item2col = np.full(n_items, -1, dtype=np.int32)
    item2col[:V] = rng.permutation(V).astype(np.int32)          # items >= V have no column
    ptr, items = _pos_csr(rng, n_users, n_items, [0, 1, 64, 65, 200])
    u2, u3, u4 = int(ptr[2]), int(ptr[3]), int(ptr[4])
    items[u2 + 10] = items[u2 + 3]                              # twice within one batch of 64
    items[u3 + 64] = items[u3 + 3]                              # twice across batches
    items[u4 + 10] = items[u4 + 3]
    items[u4 + 64:u4 + 84] = items[u4:u4 + 20]                  # twenty more across batches
    items[u4 + 150] = items[u4 + 100]
    mrows = B // 2 if B >= 2 else 0
    nm = mrows if mrows else B
    users = (np.arange(nm) % n_users).astype(np.int32)
    users = users[rng.permutation(nm)] if nm > 5 else np.array([4, 2, 3, 0, 1], dtype=np.int32)[:nm]
    row_user = users[np.arange(B) % nm]
    tcol = rng.integers(0, V, size=B).astype(np.int32)
    for r in range(0, B, 2):                                    # the target among the positives
        lst = items[ptr[row_user[r]]:ptr[row_user[r] + 1]]
        cols = item2col[lst]
        if np.any(cols >= 0):
            tcol[r] = cols[cols >= 0][0]
    keep = _csr_keep(row_user, ptr, items, item2col, B, V)
    tscore = Ld[torch.arange(B, device=dev), _t(dev, tcol.astype(np.int64))].contiguous()
    csr = tuple(_t(dev, a) for a in (users, ptr, items, item2col))
    # references
    rows = np.arange(B)

    def ref(dt):
        L = U.astype(dt) @ P.astype(dt).T + pb.astype(dt)
        t = L[rows, tcol].reshape(B, 1)
        m = L.max(1, keepdims=True)
        ce = (np.log(np.exp(L - m).sum(1, keepdims=True)) + m - t)[:, 0]
        warp = np.log1p(np.where(keep, np.maximum(L - t + 1, 0), 0).sum(1, dtype=dt))
        return ce, warp

    ce64, warp64 = ref(np.float64)
    ce32, warp32 = ref(np.float32)
    np.testing.assert_allclose(ce32, ce64, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(warp32, warp64, rtol=RTOL, atol=ATOL)
    for mode, want in ((0, ce64), (1, warp64)):
        un = (Ud, Pd, pbd, csr, mrows) if mode == 1 else None
        single = _eval_chain(dev, Ld, tscore, mode, EVAL_CHUNKINGS[0], unmask=un)
        np.testing.assert_allclose(single, want, rtol=RTOL, atol=ATOL)
        for chunks in EVAL_CHUNKINGS[1:]:
            for views in (True, False):
                got = _eval_chain(dev, Ld, tscore, mode, chunks, views=views, unmask=un)
                np.testing.assert_allclose(got, single, rtol=RTOL, atol=ATOL)
                np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("order", ['low_last', 'low_first', 'ninf_last', 'ninf_first', 'ninf_only'])
def test_eval_chunk_ce_rescaling_and_all_neg_inf_chunk(dev, order):
    """The online log-sum-exp across chunks 200 apart (l0 * exp(m0 - mm) underflows to 0, the other side keeps its
    weight), and a chunk whose every logit is -inf: it adds nothing (k_eval_chunk guards m == -inf like the sharded
    twins); all chunks -inf gives lse = -inf."""
    import torch
    rng = np.random.default_rng(len(order))
    B, n = 5, 300
    a = rng.standard_normal((B, n)).astype(np.float32)
    if order.startswith('low'):
        b = (rng.standard_normal((B, 77)) - 200.0).astype(np.float32)
    else:
        b = np.full((B, 77), -np.inf, dtype=np.float32)
    parts = {'low_last': [a, b], 'low_first': [b, a], 'ninf_last': [a, b], 'ninf_first': [b, a, b],
             'ninf_only': [b, b]}[order]
    L = np.concatenate(parts, axis=1)
    t = rng.standard_normal(B).astype(np.float32)
    got = _eval_chain(dev, _t(dev, L), _t(dev, t), 0, [p.shape[1] for p in parts])
    if order == 'ninf_only':
        assert np.all(np.isneginf(got))
    else:
        with np.errstate(divide='ignore'):
            want = _lse64(L) - t
        assert np.all(np.isfinite(got))
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------
# 4. pooling
# ---------------------------------------------------------------------------------------------------------
def _bags(rng, W, max_bag, min_len):
    lens = rng.integers(min_len, max_bag + 1, size=W)
    if W > 2 and min_len == 0:
        lens[[0, W // 2, W - 1]] = 0                            # empty bags at both ends and inside
    offs = np.zeros(W + 1, dtype=np.int32)
    offs[1:] = np.cumsum(lens)
    return offs


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("B,W,max_bag", [(5, 7, 3), (33, 300, 8), (4, 257, 1), (2, 1000, 40), (1, 1, 64)])
def test_segment_pool_fwd_bwd(dev, B, W, max_bag, mode):
    """tf.segment_max (mode 2) and score_max + log(1 + segment_sum exp) (mode 3) over bags, forward and backward,
    every tensor a column slice of a wider one.  Empty bags: mode 3 gives M + log(1); mode 2 is defined by the
    kernel as -inf forward and no gradient (there is no token to receive one).  Mode 2 scores lie on the integer
    grid [-2, 2], so bags hold exact ties: the gradient is shared equally, g / cnt, to 1 ulp.  The 37 pad columns
    past offs[W] of dscores come back 0."""
    from arx import ops
    import torch
    rng = np.random.default_rng(B * 100 + W + mode)
    offs = _bags(rng, W, max_bag, 0 if W > 2 else 1)
    T = int(offs[-1])
    cap = T + 37
    if mode == 2:
        scores = rng.integers(-2, 3, size=(B, cap)).astype(np.float32)
    else:
        scores = rng.standard_normal((B, cap)).astype(np.float32)
    dout = rng.standard_normal((B, W)).astype(np.float32)
    sbase, S = _wide(dev, B, cap, 0.0)
    S.copy_(_t(dev, scores))
    obase, O = _wide(dev, B, W, 7.0)
    gbase, G = _wide(dev, B, W, 0.0)
    G.copy_(_t(dev, dout))
    dbase, D = _wide(dev, B, cap, 7.0)
    gmax = None
    x = scores.astype(np.float64)
    if mode == 3:
        gmax = torch.zeros(1, dtype=torch.float32, device=dev)
        gidx = torch.zeros(2, dtype=torch.int32, device=dev)
        ops.max_argmax(S[:, :T], 0, True, gmax, gidx)
        M = float(scores[:, :T].max())
        assert float(gmax.item()) == M
    resid = torch.full((B,), 7.0, dtype=torch.float32, device=dev) if mode == 3 else None
    ops.segment_pool_fwd(S, _t(dev, offs), W, mode, O, gmax=gmax)
    ops.segment_pool_bwd(S, _t(dev, offs), W, mode, O, G, D, gmax=gmax, resid_rows=resid)
    torch.cuda.synchronize()
    out, dsc = O.cpu().numpy(), D.cpu().numpy()
    ref_out = np.empty((B, W))
    ref_d = np.zeros((B, cap))
    ref_res = np.zeros(B)
    for j in range(W):
        q0, q1 = int(offs[j]), int(offs[j + 1])
        seg = x[:, q0:q1]
        if mode == 2:
            ref_out[:, j] = seg.max(1) if q1 > q0 else -np.inf
            if q1 > q0:
                hit = seg == seg.max(1, keepdims=True)
                ref_d[:, q0:q1] = hit * (dout[:, j].astype(np.float64) / hit.sum(1)).reshape(B, 1)
        else:
            ex = np.exp(seg - M)
            s = ex.sum(1)
            ref_out[:, j] = M + np.log1p(s)
            ref_d[:, q0:q1] = ex * (dout[:, j] / (1 + s)).reshape(B, 1)
            ref_res += dout[:, j] / (1 + s)
    if mode == 2:
        np.testing.assert_array_equal(out, ref_out.astype(np.float32))
        np.testing.assert_allclose(dsc, ref_d, rtol=1.2e-7, atol=0)          # one correctly rounded division
        if max_bag >= 3 and W >= 7:
            assert (np.count_nonzero(ref_d[:, :T], axis=1) > np.count_nonzero(np.diff(offs))).any()   # ties exist
    else:
        np.testing.assert_allclose(out, ref_out, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(dsc, ref_d, rtol=RTOL, atol=1e-7)
        np.testing.assert_allclose(resid.cpu().numpy(), ref_res, rtol=RTOL, atol=ATOL)
    assert np.all(dsc[:, T:] == 0)
    assert _canary_ok(obase, W, 7.0) and _canary_ok(dbase, cap, 7.0)


def _argmax_rule(x, col_base=0):
    """larger value, then smaller global column, then smaller row"""
    m = x.max()
    rc = np.argwhere(x == m)
    k = np.lexsort((rc[:, 0], rc[:, 1]))[0]
    return float(m), int(rc[k, 0]), int(rc[k, 1]) + col_base


@pytest.mark.parametrize("rows,cols", [(4, 1000), (64, 3100), (1, 1), (300, 70000)])
def test_max_argmax_tie_order_and_chunks(dev, rows, cols):
    """(value, row, col) of the maximum with the documented tie order.  The maximum is planted many times; one pair
    is planted so that ONE thread of the grid-strided loop meets the loser first and the winner later (stride =
    blocks x 256 elements, at most 256 blocks), which is where the per-thread comparison decides.  Fed as column
    chunks (col_base, first=False) the result is the same: an equal value in a later chunk does not displace."""
    from arx import ops
    import torch
    rng = np.random.default_rng(rows + cols)
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    n = rows * cols
    if n > 1:
        top = 100.0
        stride = min(256, -(-n // 2048)) * 256
        cw = min(5, cols - 1)
        iw = (rows - 1) * cols + cw                            # the winner: last row, a small column
        for k in range(1, 64):
            io = iw - stride * k
            if io >= 0 and io % cols > cw:
                x[io // cols, io % cols] = top                 # met first by the same thread, loses on the column
                break
        x[rows - 1, cw] = top
        for _ in range(40):                                    # more copies, none in a smaller column
            x[rng.integers(0, rows), rng.integers(cw + 1, cols) if cols > cw + 1 else cw] = top
        if rows > 1 and cols > cw + 1:
            x[0, cw + 1] = top                                 # smaller row, larger column: still loses
        assert (x == top).sum() >= 3
    want = _argmax_rule(x)
    base, X = _wide(dev, rows, cols, 1000.0, off=3, pad=5)     # strided; the canaries exceed every value
    X.copy_(_t(dev, x))
    best = torch.zeros(1, dtype=torch.float32, device=dev)
    bidx = torch.zeros(2, dtype=torch.int32, device=dev)
    ops.max_argmax(X, 0, True, best, bidx)
    assert (float(best.item()), int(bidx[0].item()), int(bidx[1].item())) == want
    ops.max_argmax(_t(dev, x), 0, True, best, bidx)
    assert (float(best.item()), int(bidx[0].item()), int(bidx[1].item())) == want
    if cols >= 4:
        cuts = sorted(set([0, 1, cols // 3, cols // 3 + cols // 2, cols]))
        for k in range(len(cuts) - 1):
            ops.max_argmax(X[:, cuts[k]:cuts[k + 1]], cuts[k], k == 0, best, bidx)
            part = _argmax_rule(x[:, :cuts[k + 1]])
            assert (float(best.item()), int(bidx[0].item()), int(bidx[1].item())) == part, k
        assert part == want


@pytest.mark.parametrize("d", [4, 128, 1024])
def test_gmax_residual_bwd(dev, d):
    from arx import ops
    import torch
    rng = np.random.default_rng(d)
    B = 9
    U = rng.standard_normal((B, d)).astype(np.float32)
    Ev = rng.standard_normal(d).astype(np.float32)
    dU0 = rng.standard_normal((B, d)).astype(np.float32)
    g, r = np.float32(-0.75), 6
    resid = _t(dev, np.array([g], dtype=np.float32))
    idx = _t(dev, np.array([r, 41], dtype=np.int32))
    for with_extra in (True, False):
        row_grad = torch.full((d + 3,), 7.0, dtype=torch.float32, device=dev)
        bias_grad = torch.full((2,), 7.0, dtype=torch.float32, device=dev) if with_extra else None
        ubase, dU = _wide(dev, B, d, 7.0)
        dU.copy_(_t(dev, dU0))
        ops.gmax_residual_bwd(resid, idx, _t(dev, U), _t(dev, Ev), row_grad, bias_grad, dU if with_extra else None)
        rgot = row_grad.cpu().numpy()
        np.testing.assert_allclose(rgot[:d], g * U[r].astype(np.float64), rtol=1e-6, atol=0)
        assert np.all(rgot[d:] == 7.0)
        want = dU0.astype(np.float64).copy()
        if with_extra:
            want[r] += g * Ev.astype(np.float64)
            np.testing.assert_array_equal(bias_grad.cpu().numpy(), np.array([g, 7.0], dtype=np.float32))
        got = dU.cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)
        np.testing.assert_array_equal(np.delete(got, r, 0), np.delete(dU0, r, 0))     # accumulated onto row r only
        assert _canary_ok(ubase, d, 7.0)


@pytest.mark.parametrize("per_step", [False, True])
@pytest.mark.parametrize("d", [0, 20, 96, 128, 256, 300])
def test_gmax_norm_corr(dev, d, per_step):
    """corr[t] = 2 <M, R> + |R|^2: M the merged gradient row of table row vrows[t] (key lists naming it 0, 1 and
    many times), R the rank-one rows landing on it.  Summed form: the first step naming v carries every R of v,
    the others write 0; per-step form: every step on its own X_t.  d = 0 stands for the bias-only form; the thread
    group layout changes with d (20 and 96 do not divide 256, 256 is one full block, 300 has a second block)."""
    from arx import ops
    import torch
    rng = np.random.default_rng(d + 7 * per_step)
    L, rows, nsrc, n = 6, 50, 40, 500
    v_many, v_one, v_none = 7, 3, 11
    vrows = np.array([v_many, v_one, v_many, v_none, v_many, v_one], dtype=np.int32)
    keys = rng.integers(0, rows, size=n).astype(np.int32)
    keys[(keys == v_one) | (keys == v_none)] = 20
    keys[rng.choice(n, size=60, replace=False)] = v_many
    keys[123] = v_one
    src = rng.integers(0, nsrc, size=n).astype(np.int32)
    coef = rng.standard_normal(n).astype(np.float32)
    wd = max(d, 1)
    X = rng.standard_normal((L, nsrc, wd)).astype(np.float32)
    Xb = rng.standard_normal((L, nsrc)).astype(np.float32)
    RG = rng.standard_normal((L, wd)).astype(np.float32)
    RGb = rng.standard_normal(L).astype(np.float32)
    want = np.zeros(L)
    scale = np.zeros(L)
    for t in range(L):
        v = vrows[t]
        if not per_step and v in vrows[:t]:
            continue
        hit = keys == v
        for Xs, Rs, on in ((X, RG, d > 0), (Xb[:, :, None], RGb[:, None], True)):
            if not on:
                continue
            Xt = Xs[t if per_step else 0].astype(np.float64)
            terms = coef[hit].astype(np.float64)[:, None] * Xt[src[hit]]
            Mrow = terms.sum(0)
            R = Rs[t].astype(np.float64) if per_step else Rs[vrows == v].astype(np.float64).sum(0)
            want[t] += 2 * Mrow @ R + R @ R
            scale[t] += 2 * np.abs(terms).sum(0) @ np.abs(Rs[vrows == v].astype(np.float64)).sum(0) + \
                np.square(np.abs(Rs[vrows == v].astype(np.float64)).sum(0)).sum()
    Xd = _t(dev, X if per_step else X[0]) if d > 0 else None
    Xbd = _t(dev, Xb if per_step else Xb[0])
    corr = torch.full((L,), 7.0, dtype=torch.float32, device=dev)
    ops.gmax_norm_corr(_t(dev, keys), _t(dev, src), _t(dev, coef), n, Xd, wd, per_step, nsrc * wd, Xbd, per_step,
                       nsrc, _t(dev, vrows), _t(dev, RG) if d > 0 else None, _t(dev, RGb), corr)
    got = corr.cpu().numpy()
    if not per_step:
        assert np.all(got[[2, 4, 5]] == 0)
    _scale_bound(np.abs(got - want), scale)
    assert np.all(np.abs(want[[0, 1, 3]]) > 1e-3)


# ---------------------------------------------------------------------------------------------------------
# 5. per-step TN GEMM
# ---------------------------------------------------------------------------------------------------------
STEPS_TN_CASES = [
    # steps, Kb, M, N      path (arx_gemm_f32_steps_tn)                      reduce kernel of C_sum
    (1, 64, 64, 64),     # steps == 1: launch_gemm<64,64,16> fallback        k_splitk_reduce (1 < 8 steps)
    (3, 16, 64, 64),     # Kb % 32 == 16: fallback                            k_splitk_reduce
    (5, 48, 128, 64),    # Kb % 32 == 16: fallback                            k_splitk_reduce
    (7, 64, 128, 128),   # LDS-DMA, bm 128                                    k_splitk_reduce (7 < 8)
    (8, 64, 256, 64),    # LDS-DMA, bm 128                                    k_splitk_reduce_lanes (>= 8)
    (50, 64, 128, 128),  # LDS-DMA, bm 128 (the LSTM shape)                   k_splitk_reduce_lanes
    (4, 32, 192, 64),    # LDS-DMA, bm 64 (M % 128 != 0)                      k_splitk_reduce
    (9, 32, 100, 36),    # LDS-DMA takes it (M % 4, N % 4, N > 32): bm 64, ragged M and N tiles; lanes reduce
    (9, 32, 100, 30),    # N <= 32: gemm_dma_supported refuses -> fallback, ragged tiles; N % 4 != 0: k_splitk_reduce
]


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("steps,Kb,M,N", STEPS_TN_CASES)
def test_gemm_steps_tn(dev, steps, Kb, M, N, strided):
    """C_steps[t] = A_t^T B_t, rowsum_steps[t] = column sums of A_t, C_sum = beta C_sum + sum_t, rowsum_sum."""
    from arx import ops
    import torch
    rng = np.random.default_rng(steps * 1000 + Kb + M + N)
    K = steps * Kb
    A = rng.standard_normal((K, M)).astype(np.float32)
    Bm = rng.standard_normal((K, N)).astype(np.float32)
    C0 = rng.standard_normal((M, N)).astype(np.float32)
    if strided:                                                # 16-byte aligned slices: the path stays the same
        _, Ad = _wide(dev, K, M, 50.0)
        _, Bd = _wide(dev, K, N, 50.0)
        Ad.copy_(_t(dev, A))
        Bd.copy_(_t(dev, Bm))
    else:
        Ad, Bd = _t(dev, A), _t(dev, Bm)
    A3 = A.astype(np.float64).reshape(steps, Kb, M)
    B3 = Bm.astype(np.float64).reshape(steps, Kb, N)
    ref = np.einsum('tkm,tkn->tmn', A3, B3)
    sc = np.einsum('tkm,tkn->tmn', np.abs(A3), np.abs(B3))
    ref_rs, sc_rs = A3.sum(1), np.abs(A3).sum(1)
    for beta, with_sum, with_rs in ((0.0, True, True), (0.5, True, False), (0.0, False, True), (0.0, False, False)):
        Cs = torch.full((steps, M, N), 7.0, dtype=torch.float32, device=dev)
        rs = torch.full((steps, M), 7.0, dtype=torch.float32, device=dev) if with_rs else None
        cbase, Csum = _wide(dev, M, N, 7.0)
        Csum.copy_(_t(dev, C0))
        rsum = torch.full((M,), 7.0, dtype=torch.float32, device=dev) if with_rs and with_sum else None
        ops.gemm_steps_tn(Ad, Bd, Cs, rs, steps, Kb, C_sum=Csum if with_sum else None, beta=beta, rowsum_sum=rsum)
        torch.cuda.synchronize()
        _scale_bound(np.abs(Cs.cpu().numpy() - ref), sc)
        if with_rs:
            _scale_bound(np.abs(rs.cpu().numpy() - ref_rs), sc_rs)
        if with_sum:
            _scale_bound(np.abs(Csum.cpu().numpy() - (beta * C0 + ref.sum(0))), sc.sum(0) + beta * np.abs(C0))
            assert _canary_ok(cbase, N, 7.0)
        else:
            np.testing.assert_array_equal(Csum.cpu().numpy(), C0)
        if rsum is not None:
            _scale_bound(np.abs(rsum.cpu().numpy() - ref_rs.sum(0)), sc_rs.sum(0))


# ---------------------------------------------------------------------------------------------------------
# 6. small kernels
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 1000003])
def test_act_fwd_bwd_in_place(dev, n):
    """relu / tanh forward and backward, in place as the MLP calls them (y is x, dx is dy)."""
    from arx import ops
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 2).astype(np.float32)
    x[::7] = 0.0
    x[n // 2] = 30.0
    x[n // 3] = -30.0
    dy = rng.standard_normal(n).astype(np.float32)
    x64 = x.astype(np.float64)
    for kind, f in ((0, np.maximum(x64, 0)), (1, np.tanh(x64))):
        buf = _t(dev, np.concatenate([x, [7.0]]).astype(np.float32))
        ops.act_fwd(buf[:n], kind, buf[:n])
        y = buf.cpu().numpy()
        assert y[n] == 7.0
        if kind == 0:
            np.testing.assert_array_equal(y[:n], f.astype(np.float32))
        else:
            np.testing.assert_allclose(y[:n], f, rtol=RTOL, atol=ATOL)
            assert np.all(np.abs(y[:n]) <= 1.0)
        g = _t(dev, np.concatenate([dy, [7.0]]).astype(np.float32))
        ops.act_bwd(buf[:n], g[:n], kind, g[:n])
        dx = g.cpu().numpy()
        assert dx[n] == 7.0
        yy = y[:n].astype(np.float64)
        want = dy * ((yy > 0) if kind == 0 else (1 - yy * yy))
        np.testing.assert_allclose(dx[:n], want, rtol=1e-6, atol=1e-6)


def test_dropout_step_counter_and_bwd(dev):
    from arx import ops
    import torch
    rng = np.random.default_rng(0)
    n = 1 << 20
    x = (rng.standard_normal(n) + 3.0).astype(np.float32)
    dy = rng.standard_normal(n).astype(np.float32)
    xd, dyd = _t(dev, x), _t(dev, dy)
    step = torch.zeros(1, dtype=torch.int64, device=dev)

    def draw(p, seed):
        y = torch.empty(n, dtype=torch.float32, device=dev)
        km = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        ops.dropout_fwd_step(xd, p, seed, step, y, km)
        return y.cpu().numpy(), km.cpu().numpy()

    for p in (0.5, 0.9):
        y0, k0 = draw(p, 11)
        y1, k1 = draw(p, 11)
        np.testing.assert_array_equal(k0, k1)                  # same (seed, step): the same mask
        np.testing.assert_array_equal(y0, y1)
        assert set(np.unique(k0).tolist()) <= {0, 1}
        kept = k0.astype(bool)
        np.testing.assert_allclose(y0[kept], x[kept].astype(np.float64) / p, rtol=1e-6)
        assert np.all(y0[~kept] == 0)
        # n independent Bernoulli(p) draws: the kept share is within 5 standard deviations sqrt(p (1 - p) / n) of p
        assert abs(kept.mean() - p) <= 5 * np.sqrt(p * (1 - p) / n)
        dx = torch.empty(n, dtype=torch.float32, device=dev)
        ops.dropout_bwd(dyd, _t(dev, k0), p, dx)
        np.testing.assert_allclose(dx.cpu().numpy(), dy.astype(np.float64) * k0 / p, rtol=1e-6)
        _, k_seed = draw(p, 12)
        ops.counter_add(step)
        _, k_step = draw(p, 11)
        assert int(step.item()) >= 1
        for other in (k_seed, k_step):                         # independent masks agree on p^2 + (1-p)^2 of the draws
            agree = (other == k0).mean()
            q = p * p + (1 - p) * (1 - p)
            assert abs(agree - q) <= 5 * np.sqrt(q * (1 - q) / n)
    step.zero_()
    ops.counter_add(step, 5)
    ops.counter_add(step)
    assert int(step.item()) == 6
    y, k = draw(1.0, 3)
    assert np.all(k == 1)
    np.testing.assert_array_equal(y, x)


DENSE_SIZES = [1, 255, 4096, 100003]


@pytest.mark.parametrize("count", [1, 8, 9, 17])
def test_adagrad_dense_multi(dev, count):
    """1, 8, 9 and 17 tensors (a second and third launch of 8) of mixed sizes against rg.adagrad_apply per tensor,
    with the device-side gradient scale, every third tensor without an accumulator (plain SGD)."""
    from arx import ops
    import torch
    rng = np.random.default_rng(count)
    lr, gs = 0.5, 0.25
    params, want = [], []
    for k in range(count):
        n = DENSE_SIZES[(k + count) % 4]
        w = rng.standard_normal(n).astype(np.float32)
        acc = (0.1 + rng.random(n)).astype(np.float32) if k % 3 != 2 else None
        g = rng.standard_normal(n).astype(np.float32)
        params.append((_t(dev, w), _t(dev, acc) if acc is not None else None, _t(dev, g)))
        w64, g64 = w.astype(np.float64), g.astype(np.float64) * gs
        if acc is None:
            want.append((w64 - lr * g64, None))
        else:
            a64 = acc.astype(np.float64)
            rg.adagrad_apply(w64, a64, g64, lr)
            want.append((w64, a64))
    ops.adagrad_dense_multi(params, torch.tensor([lr], dtype=torch.float32, device=dev),
                            gscale_dev=torch.tensor([gs], dtype=torch.float32, device=dev))
    for (w, acc, _), (w64, a64) in zip(params, want):
        np.testing.assert_allclose(w.cpu().numpy(), w64, rtol=RTOL, atol=ATOL)
        if a64 is not None:
            np.testing.assert_allclose(acc.cpu().numpy(), a64, rtol=RTOL)


@pytest.mark.parametrize("count", [1, 8, 9])
def test_sq_norm_accum_multi(dev, count):
    """out += sum_i w_i x_i^2 over 1, 8 and 9 tensors (second launch), some [rows, d] with a per-row scale, onto a
    non-zero out: equals the chain of single-tensor calls at 1e-6 and the fp64 sum at RTOL."""
    from arx import ops
    import torch
    rng = np.random.default_rng(count)
    items, total = [], 3.5
    for k in range(count):
        if k % 3 == 1:
            rows, d = [(37, 20), (500, 128), (1, 4)][(k // 3) % 3]
            x = rng.standard_normal((rows, d)).astype(np.float32)
            rs = rng.random(rows).astype(np.float32)
            total += float((rs.astype(np.float64)[:, None] * x.astype(np.float64) ** 2).sum())
            items.append((_t(dev, x), d, _t(dev, rs), None))
        else:
            n = DENSE_SIZES[(k + count) % 4]
            x = rng.standard_normal(n).astype(np.float32)
            total += float((x.astype(np.float64) ** 2).sum())
            items.append((_t(dev, x), 1, None, None))
    out = torch.tensor([3.5], dtype=torch.float32, device=dev)
    ops.sq_norm_accum_multi(items, out)
    one = torch.tensor([3.5], dtype=torch.float32, device=dev)
    for x, d, rs, n in items:
        ops.sq_norm_accum(x, one, d=d, row_scale=rs, n=n)
    np.testing.assert_allclose(out.item(), total, rtol=RTOL)
    np.testing.assert_allclose(out.item(), one.item(), rtol=1e-6)


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 4095, 4096, 4097, 8191, 8192, 8193, 100003])
def test_dot_scaled(dev, n):
    """One workgroup, three unrolled loops (8 x 1024, 4 x 1024, 1024) with hand-written bounds: every n around
    them; the n= override shorter than the tensors (the tail holds values that would show)."""
    from arx import ops
    import torch
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n + 5).astype(np.float32)
    y = rng.standard_normal(n + 5).astype(np.float32)
    x[n:], y[n:] = 1000.0, 1000.0
    out = torch.full((2,), 7.0, dtype=torch.float32, device=dev)
    ops.dot_scaled(_t(dev, x), _t(dev, y), 0.5, out, n=n)
    got = out.cpu().numpy()
    assert got[1] == 7.0
    x64, y64 = x[:n].astype(np.float64), y[:n].astype(np.float64)
    _scale_bound(np.abs(got[0] - 0.5 * (x64 @ y64)), 0.5 * (np.abs(x64) @ np.abs(y64)))
    if n:
        ops.dot_scaled(_t(dev, x[:n]), _t(dev, y[:n]), 0.5, out)
        assert out.cpu().numpy()[0] == got[0]


def test_inv_len_scale_axpby_fill(dev):
    from arx import ops
    import torch
    rng = np.random.default_rng(2)
    lens = rng.integers(1, 50, size=700).astype(np.int32)
    ids = rng.integers(0, 700, size=300).astype(np.int32)
    out = torch.empty(300, dtype=torch.float32, device=dev)
    ops.inv_len_scale(_t(dev, lens), _t(dev, ids), 0.25, out)
    np.testing.assert_allclose(out.cpu().numpy(), 0.25 / lens[ids].astype(np.float64), rtol=1e-6)
    out = torch.full((701,), 7.0, dtype=torch.float32, device=dev)
    ops.inv_len_scale(_t(dev, lens), None, 2.0, out[:700])
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[:700], 2.0 / lens.astype(np.float64), rtol=1e-6)
    assert got[700] == 7.0
    for n in (1, 257, 100003):
        x = rng.standard_normal(n).astype(np.float32)
        y = rng.standard_normal(n + 1).astype(np.float32)
        yd = _t(dev, y)
        ops.axpby(0.5, _t(dev, x), -2.0, yd, n=n)
        got = yd.cpu().numpy()
        np.testing.assert_allclose(got[:n], 0.5 * x.astype(np.float64) - 2.0 * y[:n], rtol=1e-6, atol=1e-6)
        assert got[n] == y[n]
        yn = torch.full((n,), float('nan'), dtype=torch.float32, device=dev)
        ops.axpby(3.0, _t(dev, x), 0.0, yn)                    # b == 0 overwrites: NaN * 0 is not formed
        np.testing.assert_array_equal(yn.cpu().numpy(), np.float32(3.0) * x)
    for n in (0, 1, 255, 1001):
        for fill, dt, v in ((ops.fill_f32, torch.float32, -1.5), (ops.fill_i32, torch.int32, -7),
                            (ops.fill_u8, torch.uint8, 201)):
            t = torch.ones(n + 3, dtype=dt, device=dev)
            fill(t[1:1 + n], v)
            got = t.cpu().numpy()
            assert np.all(got[1:1 + n] == v) and got[0] == 1 and np.all(got[1 + n:] == 1)


@pytest.mark.parametrize("rows,cols", [(1, 1), (31, 33), (32, 32), (100, 257)])
def test_transpose(dev, rows, cols):
    from arx import ops
    rng = np.random.default_rng(rows + cols)
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    _, S = _wide(dev, rows, cols, 50.0, off=3, pad=5)
    S.copy_(_t(dev, x))
    dbase, D = _wide(dev, cols, rows, 7.0, off=3, pad=5)
    ops.transpose(S, D)
    np.testing.assert_array_equal(D.cpu().numpy(), x.T)
    assert _canary_ok(dbase, rows, 7.0, off=3)


def test_take_rows_site_onehot_add_col_bias(dev):
    from arx import ops
    from arx._lib import call
    import torch
    rng = np.random.default_rng(6)
    B, C, k = 37, 300, 11
    table = rng.integers(-5, 10 ** 6, size=(B, C)).astype(np.int32)
    pos = rng.integers(0, C, size=(B, k)).astype(np.int32)
    tb = _t(dev, np.pad(table, ((0, 0), (0, 7))))[:, :C]
    pb = _t(dev, np.pad(pos, ((0, 0), (2, 3))))[:, 2:2 + k]
    out = torch.full((B, k + 4), -9, dtype=torch.int32, device=dev)
    ops.take_rows_i32(tb, pb, out[:, 1:1 + k])
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:, 1:1 + k], np.take_along_axis(table, pos, 1))
    assert np.all(got[:, 0] == -9) and np.all(got[:, 1 + k:] == -9)
    # sparse_site_onehot: keys through cat_map (or the id itself), an empty slot (id < 0) -> KEY_NONE
    n = 1000
    cmap = rng.integers(0, 77, size=500).astype(np.int32)
    ids = rng.integers(0, 500, size=n).astype(np.int32)
    ids[::13] = -1
    for cm in (cmap, None):
        want = np.where(ids < 0, ops.KEY_NONE, (cmap[np.maximum(ids, 0)] if cm is not None else ids))
        keys = torch.full((n + 1,), -3, dtype=torch.int32, device=dev)
        src = torch.full((n + 1,), -3, dtype=torch.int32, device=dev)
        coef = torch.full((n + 1,), 7.0, dtype=torch.float32, device=dev)
        ops.sparse_site_onehot(_t(dev, cm) if cm is not None else None, _t(dev, ids), 40, 0.125, keys[:n], src[:n],
                               coef[:n])
        np.testing.assert_array_equal(keys.cpu().numpy(), np.append(want, -3))
        np.testing.assert_array_equal(src.cpu().numpy(), np.append(40 + np.arange(n), -3))
        np.testing.assert_array_equal(coef.cpu().numpy(), np.append(np.full(n, 0.125, np.float32), 7.0))
        keys.fill_(-3)
        ops.sparse_site_onehot(_t(dev, cm) if cm is not None else None, _t(dev, ids), 40, 0.125, keys[:n], None, None)
        np.testing.assert_array_equal(keys.cpu().numpy(), np.append(want, -3))
    # arx_add_col_bias has no ops wrapper (and no caller): the C entry point itself, ld > cols
    rows, cols = 33, 130
    y = rng.standard_normal((rows, cols)).astype(np.float32)
    b = rng.standard_normal(cols).astype(np.float32)
    ybase, Y = _wide(dev, rows, cols, 7.0, off=3, pad=5)
    Y.copy_(_t(dev, y))
    bd = _t(dev, b)
    call("arx_add_col_bias", Y.data_ptr(), int(Y.stride(0)), rows, cols, bd.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(Y.cpu().numpy(), y + b)
    assert _canary_ok(ybase, cols, 7.0, off=3)


def test_copy_2d_gather_rows_wide_take_shard_route(dev):
    """Four more plumbing kernels that only model / distributed tests reached: bit-exact."""
    from arx import ops
    import torch
    rng = np.random.default_rng(8)
    rows, cols = 37, 132
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    _, S = _wide(dev, rows, cols, 50.0)
    S.copy_(_t(dev, x))
    dbase, D = _wide(dev, rows, cols, 7.0)
    ops.copy_2d(S, D)
    np.testing.assert_array_equal(D.cpu().numpy(), x)
    assert _canary_ok(dbase, cols, 7.0)
    # gather_rows_wide: any width (a second 1024-column block, a ragged tail, the scalar path), zeros for row
    # indices out of range
    for width, off in ((1030, 4), (5, 3), (1024, 4)):
        src = rng.standard_normal((50, width)).astype(np.float32)
        idx = rng.integers(0, 50, size=70).astype(np.int32)
        idx[[3, 9]] = [-1, 50]
        _, Sv = _wide(dev, 50, width, 50.0, off=off)
        Sv.copy_(_t(dev, src))
        gbase, G = _wide(dev, 70, width, 7.0, off=off)
        ops.gather_rows_wide(Sv, _t(dev, idx), G)
        want = np.where(((idx >= 0) & (idx < 50))[:, None], src[np.clip(idx, 0, 49)], 0).astype(np.float32)
        np.testing.assert_array_equal(G.cpu().numpy(), want)
        assert _canary_ok(gbase, width, 7.0, off=off)
    table = rng.integers(-9, 10 ** 6, size=900).astype(np.int32)
    idx = rng.integers(-1, 900, size=1000).astype(np.int32)
    out = torch.full((1001,), -3, dtype=torch.int32, device=dev)
    ops.take_i32(_t(dev, table), _t(dev, idx), out[:1000], fill=-77)
    np.testing.assert_array_equal(out.cpu().numpy(), np.append(np.where(idx >= 0, table[np.maximum(idx, 0)], -77), -3))
    ids = rng.integers(-1, 5000, size=1300).astype(np.int32)
    for world, rank in ((1, 0), (3, 2), (8, 0)):
        r_out = torch.full((1301,), -3, dtype=torch.int32, device=dev)
        k_out = torch.full((1301,), -3, dtype=torch.int32, device=dev)
        ops.shard_route(_t(dev, ids), world, rank, 777, r_out[:1300], k_out[:1300])
        own = (ids >= 0) & (ids % world == rank)
        np.testing.assert_array_equal(r_out.cpu().numpy(), np.append(np.where(own, ids // world, 777), -3))
        np.testing.assert_array_equal(k_out.cpu().numpy(), np.append(np.where(own, ids // world, ops.KEY_NONE), -3))
