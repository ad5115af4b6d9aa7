"""Pure-numpy restatements of what the fused scorer-GEMM epilogues (csrc/gemm_nt.hip) and TopKScan compute, given the
materialised logits: the column-range split, a row's candidate segments (with and without exclusion lists and a
segment capacity), tf.nn.top_k's order, the chunk + merge composition and a log-sum-exp that knows -inf.
test_gemm_nt_fused_gpu.py compares the kernels with these; test_gemm_nt_oracle_cpu.py compares these with brute force,
so the oracle is itself checked where no GPU is present."""
import numpy as np

TILE = 64            # columns per pool tile (kNtBN)
PANEL = 128          # rows per workgroup (kNtBM)
IDX_FILL = -7        # what the tests pre-fill cand_i with


def split_ranges(N, parts):
    """include/arx.h next to arx_gemm_nt_topk_parts: range p covers [p * tpb * 64, min(N, (p + 1) * tpb * 64)),
    tpb = ceil(ceil(N / 64) / parts)."""
    tiles = -(-N // TILE)
    tpb = -(-tiles // parts)
    assert -(-tiles // tpb) == parts, (N, parts, tpb)
    return tpb, [(p * tpb * TILE, min(N, (p + 1) * tpb * TILE)) for p in range(parts)]


def parts_for(cu_count, M, N):
    """The number of ranges arx_gemm_nt_topk_parts reports on a device with cu_count compute units (two workgroups
    per unit, at least one tile each, then the fewest ranges with the same tiles per range)."""
    panels = -(-M // PANEL)
    tiles = -(-N // TILE)
    ns = max(1, min(-(-2 * cu_count // panels), tiles))
    tpb = -(-tiles // ns)
    return -(-tiles // tpb)


def excl_mask(M, N, col_base, ex):
    """[M, N] bool, True where row r's list names the absolute column col_base + c.  ex = (row_keys, key_rows, ex_ptr,
    ex_cols) as numpy arrays, key = row_keys[r % key_rows], key < 0: nothing; None: nothing at all."""
    out = np.zeros((M, N), dtype=bool)
    if ex is None:
        return out
    keys, key_rows, ptr, cols = ex
    for r in range(M):
        key = int(keys[r % key_rows])
        if key < 0:
            continue
        c = np.asarray(cols[ptr[key]:ptr[key + 1]], dtype=np.int64) - col_base
        c = c[(c >= 0) & (c < N)]
        out[r, c] = True
    return out


def expected_segments(L, thr, ranges, capp, ldcand, col_base=0, excluded=None):
    """-> (cand_v [M, ldcand] float32, cand_i [M, ldcand] int32, overflow): per row and range p the columns c of the
    range in ascending order with L[r, c] > thr[r] (strictly; nothing beats NaN) that are not excluded -- an excluded
    column takes no position -- cut at capp, at cand[r, p * capp ..); everything else keeps the pre-fill (-inf,
    IDX_FILL).  overflow: some segment was longer than capp."""
    M = L.shape[0]
    cv = np.full((M, ldcand), -np.inf, dtype=np.float32)
    ci = np.full((M, ldcand), IDX_FILL, dtype=np.int32)
    over = False
    with np.errstate(invalid='ignore'):
        surv = L > np.asarray(thr, dtype=L.dtype).reshape(M, 1)
    if excluded is not None:
        surv &= ~excluded
    for p, (lo, hi) in enumerate(ranges):
        s = surv[:, lo:hi]
        pos = np.cumsum(s, axis=1) - 1
        rr, cc = np.nonzero(s)
        pp = pos[rr, cc]
        over = over or bool((pp >= capp).any())
        keep = pp < capp
        rr, cc, pp = rr[keep], cc[keep], pp[keep]
        cv[rr, p * capp + pp] = L[rr, lo + cc]
        ci[rr, p * capp + pp] = col_base + lo + cc
    return cv, ci, over


def topk_tf(L, k, excluded=None):
    """tf.nn.top_k's order -- value descending, lower column first on ties -- over the columns that are not excluded;
    a row with fewer than k eligible columns (or whose further winners are -inf) ends in (-inf, -1)."""
    M, N = L.shape
    x = L.astype(np.float64)
    if excluded is not None:
        x = np.where(excluded, -np.inf, x)
    kk = min(k, N)
    order = np.argsort(-x, axis=1, kind='stable')[:, :kk]
    v = np.take_along_axis(x, order, axis=1)
    vals = np.full((M, k), -np.inf, dtype=np.float32)
    idx = np.full((M, k), -1, dtype=np.int32)
    vals[:, :kk] = v.astype(np.float32)
    idx[:, :kk] = np.where(np.isneginf(v), -1, order)
    return vals, idx


def merge_topk(va, ia, vb, ib, k):
    """arx_topk_merge: two lists sorted by (value descending, index ascending), every index of A below every index of
    B -> the k best of both, A winning ties."""
    v = np.concatenate([va, vb], axis=1).astype(np.float64)
    i = np.concatenate([ia, ib], axis=1)
    order = np.argsort(-v, axis=1, kind='stable')[:, :k]
    return np.take_along_axis(v, order, axis=1).astype(np.float32), np.take_along_axis(i, order, axis=1)


def topk_chunked(L, k, chunk):
    """The chunked path's composition: top-k of every chunk (indices offset by the chunk's first column) merged into
    a running result.  Equal to topk_tf(L, k) (without the -1 marks: no exclusion here)."""
    M, N = L.shape
    rv, ri = None, None
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        kc = min(k, c1 - c0)
        v, i = topk_tf(L[:, c0:c1], kc)
        i = np.where(i >= 0, i + c0, i)
        rv, ri = (v, i) if rv is None else merge_topk(rv, ri, v, i, k)
    return rv, ri


def lse64(x, axis=1):
    """float64 log-sum-exp; a slice of nothing but -inf gives -inf, -inf entries add nothing."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=axis, keepdims=True)
    m0 = np.where(np.isneginf(m), 0.0, m)
    with np.errstate(divide='ignore'):
        return np.squeeze(m0 + np.log(np.exp(x - m0).sum(axis=axis, keepdims=True)), axis=axis)
