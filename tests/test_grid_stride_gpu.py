"""Second and third trips of the grid-stride loops of csrc/pair.hip, window.hip, slate.hip and similar.hip.

Those kernels launch a grid capped at a multiple of the CU count and stride over the rest of their rows.  Every shape
here is 2 * trip + remainder, with `trip` taken from tests/grid_trips.py for the CU count of the device the test runs
on, and every test asserts through that module that its shape really lies past two trips.  Each call past the cap
("the big call") gets three checks:

  1. the fp64 numpy restatement the project already has for that kernel (imported, not copied), at the tolerance of
     the kernel's existing direct test; integer outputs bit for bit
  2. launch-shape invariance, bit for bit: the same kernel on row slices of at most trip // 2 rows (one trip each) --
     the first rows, a slice straddling the end of the first trip, the last ragged rows -- gives the rows of the big
     call (the draws are keyed by the row number: a shorter call must give the head of the longer one; a slate row is
     compared with a call of that row alone)
  3. canaries: outputs are column slices of wider canary-filled buffers with one spare row behind the last; the
     padding and the spare row keep their value, and the outputs themselves start from a sentinel, so a row the loop
     skipped shows.

The data and the references are built once per shape and left unchanged."""
import numpy as np
import pytest

import grid_trips as GT
import similar_oracle as S
import slate_oracle as SO
from numpy_backend_similar import NumpySimilarBackend      # (the window and the unit-row doubles: one class chain)
from test_bpr_cpu import rank_select
from test_bpr_gpu import KINDS, _csr, _pair_case, _pair_ref
from test_hmf_gpu import ATOL, RTOL
from test_kernels_direct_gpu import _canary_ok, _t, _wide
from test_neg_draw_weighted_cpu import draw_key
from test_neg_draw_weighted_gpu import _tables_of

pytestmark = pytest.mark.gpu

CANARY = 55.0           # padding columns, spare rows, rows of dR no slot names
SENT = 9.0              # what an output row holds before its kernel writes it
_CASES = {}


def _cu():
    from arx import ops
    return int(ops.device_info()["cu_count"])


def _once(key, build):
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d entries differ, first at %s" % (what, len(bad), bad[0].tolist()))


def _in2d(dev, a, pad=4):
    """a [rows, d] as the left columns of a [rows, d + pad] tensor: an input with leading dimension d + pad."""
    import torch
    rows, d = a.shape
    base = torch.full((rows, d + pad), CANARY, dtype=torch.float32, device=dev)
    base[:, :d] = _t(dev, a)
    return base[:, :d]


def _out2d(dev, rows, cols, fill, pad=4):
    """(base, view): a [rows, cols] output view holding `fill` (a sentinel, or an array to accumulate into), leading
    dimension cols + pad, inside a CANARY-filled tensor with one spare row behind the last."""
    base, view = _wide(dev, rows + 1, cols, CANARY, off=0, pad=pad)
    view = view[:rows]
    if isinstance(fill, np.ndarray):
        view.copy_(_t(dev, fill))
    else:
        view.fill_(fill)
    return base, view


def _out2d_ok(base, rows, cols):
    return _canary_ok(base, cols, CANARY, off=0) and bool((base[rows] == CANARY).all().item())


def _out1d(dev, n, fill, dtype=None):
    """(base, view) of n entries holding `fill` with one spare entry behind them."""
    import torch
    base = torch.full((n + 1,), fill, dtype=dtype or torch.float32, device=dev)
    return base, base[:n]


def _np(t):
    return np.ascontiguousarray(t.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------
# pair.hip: k_pair_loss, k_pair_loss_slots, k_pair_auc, k_pair_auc_counts
# ---------------------------------------------------------------------------------------------------------
PAIR_SEED = 5
PAIR_D = [132, 64]      # 64 lanes per row (31 idle), one row per wave / 16 lanes, four rows per wave
KINK = 1e-4             # (test_bpr_gpu.py: no row near the hinge's kink, fp32 takes the same branch)


def _pair_shape(cu, d):
    T = GT.pair_rows(cu, d)
    B = 2 * T + 3
    void = np.zeros(B, dtype=bool)
    void[[T // 2, T + T // 2, 2 * T + 1]] = True                              # one void row in each of the three trips
    return T, B, void


def _pair_big(cu, kind, d):
    """Operands (test_bpr_gpu._pair_case) and the fp64 reference of the plain form; 'bpr-hinge': the first seed from
    PAIR_SEED on that leaves no row within KINK of the kink."""
    def build():
        T, B, void = _pair_shape(cu, d)
        gscale = 1.0 / B
        for seed in range(PAIR_SEED, PAIR_SEED + 16):
            ops_ = _pair_case(B, d, seed)
            U, P, pb, N, nb, rw, dU0 = ops_
            ref = _pair_ref(kind, U, P, pb, N, nb, void, rw, gscale, dU0)
            if kind == 'bpr' or np.abs(1.0 + ref['x']).min() > KINK:
                break
        return dict(T=T, B=B, void=void, gscale=gscale, ops=ops_, ref=ref, seed=seed)
    return _once(('pair', cu, kind, d), build)


def _pair_slots_big(cu, kind, d):
    """The same rows as packed rows of ONE block named by slot: R[pos_slot[r]] = (P[r] | pbias[r]), R[neg_slot[r]] =
    (N[r] | nbias[r]); the slots are a random permutation (one writer per row of dR), 7 rows are named by nobody, the
    void rows have neg_slot = -1 and one more row a slot >= n_slots (its negative is not read, its score is 0)."""
    def build():
        c = _pair_big(cu, kind, d)
        T, B = c['T'], c['B']
        U, P, pb, N, nb, rw, dU0 = c['ops']
        rng = np.random.default_rng(1000 + d)
        n_slots = 2 * B + 7
        perm = rng.permutation(n_slots).astype(np.int32)
        pos_slot, neg_slot = perm[:B].copy(), perm[B:2 * B].copy()
        R = rng.standard_normal((n_slots, d + 4)).astype(np.float32)
        R[pos_slot, :d], R[pos_slot, d] = P, pb
        R[neg_slot, :d], R[neg_slot, d] = N, nb
        neg_slot[c['void']] = -1
        neg_slot[T + 5] = n_slots + 5
        live = (neg_slot >= 0) & (neg_slot < n_slots)
        assert (~live).sum() == 4 and len(np.unique(np.concatenate([pos_slot, neg_slot[live]]))) == B + live.sum()
        ref = _pair_ref(kind, U, P, pb, N * live[:, None], nb * live, ~live, rw, c['gscale'], dU0)
        want_dR = np.full((n_slots, d + 1), CANARY)
        want_dR[pos_slot, :d], want_dR[pos_slot, d] = ref['dP'], ref['dpb']
        want_dR[neg_slot[live], :d], want_dR[neg_slot[live], d] = ref['dN'][live], ref['dnb'][live]
        named = np.zeros(n_slots, dtype=bool)
        named[pos_slot] = True
        named[neg_slot[live]] = True
        return dict(c, R=R, pos_slot=pos_slot, neg_slot=neg_slot, live=live, n_slots=n_slots, ref=ref,
                    want_dR=want_dR, named=named)
    return _once(('pair_slots', cu, kind, d), build)


def _pair_inputs(dev, c):
    U, P, pb, N, nb, rw, _ = c['ops']
    return dict(U=_in2d(dev, U), P=_in2d(dev, P), N=_in2d(dev, N), pb=_t(dev, pb), nb=_t(dev, nb), rw=_t(dev, rw),
                ids=_t(dev, np.where(c['void'], -1, 7).astype(np.int32)))


def _pair_call(dev, c, kind, t, lo, hi):
    """arx_pair_loss_fwdbwd on rows [lo, hi): row weights, acc_dU = 1, leading dimensions d + 4 -> numpy outputs."""
    from arx import ops
    n, d = hi - lo, c['ops'][0].shape[1]
    one = {k: _out1d(dev, n, SENT) for k in ('ps', 'ns', 'loss', 'dpb', 'dnb')}
    two = {'dU': _out2d(dev, n, d, c['ops'][6][lo:hi]), 'dP': _out2d(dev, n, d, SENT), 'dN': _out2d(dev, n, d, SENT)}
    ops.pair_loss(t['U'][lo:hi], t['P'][lo:hi], t['pb'][lo:hi], t['N'][lo:hi], t['nb'][lo:hi], kind, c['gscale'],
                  one['ps'][1], one['ns'][1], one['loss'][1], neg_ids=t['ids'][lo:hi], row_w=t['rw'][lo:hi],
                  dU=two['dU'][1], acc_dU=True, dP=two['dP'][1], dpbias=one['dpb'][1], dN=two['dN'][1],
                  dnbias=one['dnb'][1])
    for k, (base, _) in one.items():
        assert float(base[n].item()) == SENT, k + ': the spare entry'
    for k, (base, _) in two.items():
        assert _out2d_ok(base, n, d), k + ': padding or spare row'
    out = {k: _np(v[1]) for k, v in list(one.items()) + list(two.items())}
    out['dev'] = (one['ps'][1], one['ns'][1])
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", PAIR_D)
def test_pair_loss_past_the_grid_cap(dev, kind, d):
    import torch
    from arx import ops
    cu = _cu()
    c = _pair_big(cu, kind, d)
    T, B, void, ref = c['T'], c['B'], c['void'], c['ref']
    gpw = 64 // GT.lanes_per_row(d)
    assert GT.past(B, T) and T == GT.pair_rows(cu, d) and gpw == {132: 1, 64: 4}[d] and B % 4 != 0
    assert GT.past(B, GT.PAIR_AUC_ROWS) and B % GT.PAIR_AUC_ROWS != 0
    assert sorted(np.nonzero(void)[0] // T) == [0, 1, 2]
    if kind == 'bpr-hinge':
        assert np.abs(1.0 + ref['x']).min() > KINK, c['seed']
    t = _pair_inputs(dev, c)
    big = _pair_call(dev, c, kind, t, 0, B)
    for k in ('ps', 'ns', 'loss', 'dpb', 'dnb', 'dU', 'dP', 'dN'):
        np.testing.assert_allclose(big[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=k)
    dU0 = c['ops'][6]
    for k in ('loss', 'dP', 'dN', 'dpb', 'dnb'):
        assert not np.any(big[k][void]), k                                    # void rows: exact zeros
    np.testing.assert_array_equal(big['dU'][void], dU0[void])
    # the auc over the device's own scores: k_pair_auc strides 256 rows per round
    auc = ops.pair_auc(big['dev'][0], big['dev'][1], t['ids'], torch.zeros(1, dtype=torch.float32, device=dev))
    x32 = big['ns'] - big['ps']
    assert abs(float(auc.item()) - (0.5 - 0.5 * np.sign(x32[~void]).mean())) < 1e-6
    for lo, hi in GT.slices(B, T):
        part = _pair_call(dev, c, kind, t, lo, hi)
        for k in ('ps', 'ns', 'loss', 'dpb', 'dnb', 'dU', 'dP', 'dN'):
            _same_bits(part[k], big[k][lo:hi], "%s of rows [%d, %d)" % (k, lo, hi))


def _slots_call(dev, c, kind, t, lo, hi):
    """arx_pair_loss_slots on rows [lo, hi) against the whole block R -> numpy outputs (dR: all n_slots rows)."""
    import torch
    from arx import ops
    n, d, n_slots = hi - lo, c['ops'][0].shape[1], c['n_slots']
    one = {k: _out1d(dev, n, SENT) for k in ('ps', 'ns', 'loss')}
    dU = _out2d(dev, n, d, c['ops'][6][lo:hi])
    dR = _out2d(dev, n_slots, d + 4, CANARY)                                  # lddr = d + 8
    cnt = torch.full((3,), -7, dtype=torch.int32, device=dev)
    ops.pair_loss_slots(t['U'][lo:hi], t['R'], t['pos'][lo:hi], t['neg'][lo:hi], kind, c['gscale'], one['ps'][1],
                        one['ns'][1], one['loss'][1], row_w=t['rw'][lo:hi], dU=dU[1], acc_dU=True, dR=dR[1],
                        auc_counts=cnt[:2])
    for k, (base, _) in one.items():
        assert float(base[n].item()) == SENT, k + ': the spare entry'
    assert _out2d_ok(dU[0], n, d), 'dU: padding or spare row'
    assert _out2d_ok(dR[0], n_slots, d + 4), 'dR: padding or spare row'
    out = {k: _np(v[1]) for k, v in one.items()}
    out.update(dU=_np(dU[1]), dR=_np(dR[1]), cnt=cnt.cpu().numpy())
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", PAIR_D)
def test_pair_loss_slots_past_the_grid_cap(dev, kind, d):
    cu = _cu()
    c = _pair_slots_big(cu, kind, d)
    T, B, live, ref, n_slots = c['T'], c['B'], c['live'], c['ref'], c['n_slots']
    assert GT.past(B, T) and T == GT.pair_rows(cu, d) and B % 4 != 0
    assert GT.past(B, GT.PAIR_AUC_COUNTS_ROWS) and B % GT.PAIR_AUC_COUNTS_ROWS != 0
    assert sorted(np.nonzero(c['neg_slot'] == -1)[0] // T) == [0, 1, 2] and (c['neg_slot'] >= n_slots).sum() == 1
    if kind == 'bpr-hinge':                                                   # (a void row takes no branch: c = 0)
        assert np.abs(1.0 + ref['x'][live]).min() > KINK, c['seed']
    U, rw = c['ops'][0], c['ops'][5]
    t = dict(U=_in2d(dev, U), R=_in2d(dev, c['R']), pos=_t(dev, c['pos_slot']), neg=_t(dev, c['neg_slot']),
             rw=_t(dev, rw))
    assert t['R'].shape[1] == d + 4 and t['R'].stride(0) == d + 8
    big = _slots_call(dev, c, kind, t, 0, B)
    for k in ('ps', 'ns', 'loss', 'dU'):
        np.testing.assert_allclose(big[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=k)
    dR = big['dR']
    np.testing.assert_allclose(dR[:, :d + 1], c['want_dR'], rtol=RTOL, atol=ATOL, err_msg='dR')
    assert (dR[~c['named']] == CANARY).all() and (~c['named']).sum() == 7 + 4     # rows no slot names
    assert (dR[:, d + 1:] == CANARY).all()                                    # behind the bias column
    dU0 = c['ops'][6]
    assert not np.any(big['loss'][~live]) and not np.any(big['ns'][~live])
    assert not np.any(dR[c['pos_slot'][~live], :d + 1])                       # a void row's positive: exact zeros
    np.testing.assert_array_equal(big['dU'][~live], dU0[~live])
    # the two integers of the auc from the device's own scores: k_pair_auc_counts, 4096 rows per round, ragged last
    x32 = big['ns'] - big['ps']
    assert big['cnt'].tolist() == [int(np.sign(x32[live]).sum()), int(live.sum()), -7]
    for lo, hi in GT.slices(B, T):
        part = _slots_call(dev, c, kind, t, lo, hi)
        for k in ('ps', 'ns', 'loss', 'dU'):
            _same_bits(part[k], big[k][lo:hi], "%s of rows [%d, %d)" % (k, lo, hi))
        mine = np.concatenate([c['pos_slot'][lo:hi], c['neg_slot'][lo:hi][live[lo:hi]]])
        _same_bits(part['dR'][mine], dR[mine], "dR of rows [%d, %d)" % (lo, hi))
        rest = np.ones(n_slots, dtype=bool)
        rest[mine] = False
        assert (part['dR'][rest] == CANARY).all()


# ---------------------------------------------------------------------------------------------------------
# pair.hip: k_neg_draw_uniform, k_neg_draw_weighted
# ---------------------------------------------------------------------------------------------------------
DRAW_V, DRAW_USERS = 1000, 300
DRAW_FULL = 7           # the user whose list covers all of V: void rows
DRAW_SEED, DRAW_STEP, DRAW_COUNTER = 5, 3, 2


def _draw_big(cu):
    def build():
        V, n_users = DRAW_V, DRAW_USERS
        rng = np.random.default_rng(21)
        trip = GT.neg_draw_rows(cu)
        B = 2 * trip + 77
        lists = [np.sort(rng.choice(V, int(k), replace=False)) for k in rng.integers(0, 41, size=n_users)]
        lists[3] = np.zeros(0, dtype=np.int64)
        lists[DRAW_FULL] = np.arange(V)
        lists[11] = np.arange(40)                                             # a leading run
        lists[12] = np.arange(V - 40, V)                                      # a trailing run
        assert all((np.diff(l) > 0).all() for l in lists)                    # sorted and unique
        users = rng.integers(0, n_users, size=B).astype(np.int32)
        users[rng.random(B) < 0.01] = -1                                      # out of range: no list
        users[rng.random(B) < 0.01] = n_users
        edges = np.array([0, trip - 1, trip, 2 * trip - 1, 2 * trip, B - 1])  # first and last row of every trip
        users[edges] = [20, 21, 11, 12, 22, 23]
        users[edges + np.array([1, -1, 1, -1, 1, -1])] = DRAW_FULL            # a void row beside each
        q = rng.integers(1, 1 << 20, size=V).astype(np.int64)
        q[rng.random(V) < 0.2] = 0
        cum, ex_cum = _tables_of(q, lists)
        col2item = (rng.permutation(V) * 2 + 1).astype(np.int32)              # not the identity
        sample = np.unique(np.concatenate([edges, np.arange(0, B, max(1, B // 64))]))
        return dict(trip=trip, B=B, lists=lists, users=users, edges=edges, q=q, cum=cum, ex_cum=ex_cum,
                    col2item=col2item, sample=sample)
    return _once(('draw', cu), build)


def _groups(users, n_users):
    """(list index or -1 for a user out of range, rows) per distinct user id, every row once."""
    order = np.argsort(users, kind='stable')
    su = users[order]
    cuts = np.nonzero(np.diff(su))[0] + 1
    for rows in np.split(order, cuts):
        u = int(users[rows[0]])
        yield (u if 0 <= u < n_users else -1), rows


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("with_map", [False, True], ids=["columns", "col2item"])
def test_neg_draw_past_the_grid_cap(dev, weighted, with_map):
    """Every row of a draw of 2 * trip + 77 rows against the statement of its kernel, as
    test_neg_draw_is_the_rank_select_of_its_rank / test_weighted_draw_is_the_column_of_its_mass_point do, vectorised
    per distinct user; the RNG key of the first and last row of every trip (and 64 more) in Python integers."""
    import torch
    from arx import ops
    cu = _cu()
    c = _draw_big(cu)
    trip, B, V, lists, users = c['trip'], c['B'], DRAW_V, c['lists'], c['users']
    assert GT.past(B, trip) and trip == GT.neg_draw_rows(cu) and B % GT.BLOCK != 0
    ptr, cols = _csr(lists, dev)
    c2i_np = c['col2item'] if with_map else np.arange(V, dtype=np.int32)
    c2i = _t(dev, c['col2item']) if with_map else None
    users_d = _t(dev, users)
    cum, ex_cum = _t(dev, c['cum']), _t(dev, c['ex_cum'])
    step_dev = torch.tensor([DRAW_STEP], dtype=torch.int64, device=dev)

    def draw(n):
        items, look = _out1d(dev, n, -7, torch.int32), _out1d(dev, n, -7, torch.int32)
        if weighted:
            aux = _out1d(dev, n, -7, torch.int64)
            ops.neg_draw_weighted(users_d[:n], ptr, cols, ex_cum, cum, V, c2i, DRAW_SEED, step_dev, DRAW_COUNTER,
                                  items[1], lookup_items=look[1], out_mass=aux[1])
        else:
            aux = _out1d(dev, n, -7, torch.int32)
            ops.neg_draw_uniform(users_d[:n], ptr, cols, V, c2i, DRAW_SEED, step_dev, DRAW_COUNTER, items[1],
                                 lookup_items=look[1], out_rank=aux[1])
        for base, _ in (items, look, aux):
            assert int(base[n].item()) == -7                                  # the spare entry
        return items[1].cpu().numpy(), look[1].cpu().numpy(), aux[1].cpu().numpy()
    items, look, aux = draw(B)
    seen_void = 0
    for k, rows in _groups(users, DRAW_USERS):
        lst = lists[k] if k >= 0 else lists[3]
        if weighted:
            masked = c['q'].copy()
            masked[lst] = 0
            running = np.cumsum(masked)
            total = int(running[-1])
        else:
            total = V - len(lst)                                              # eligible columns
        if total == 0:
            assert k == DRAW_FULL
            assert (items[rows] == -1).all() and (aux[rows] == -1).all() and (look[rows] == c2i_np[0]).all()
            seen_void += len(rows)
            continue
        t = aux[rows].astype(np.int64)
        assert (t >= 0).all() and (t < total).all(), k
        if weighted:
            col = np.searchsorted(running, t, side='right')                   # the masked cumulative sum
            assert (c['q'][col] > 0).all()
        else:
            col = t + np.searchsorted(lst - np.arange(len(lst)), t, side='right')
        assert not np.isin(col, lst).any(), k
        np.testing.assert_array_equal(items[rows], c2i_np[col], err_msg="user %d" % k)
        np.testing.assert_array_equal(look[rows], items[rows])
    assert seen_void >= 6 and (users[c['edges']] != DRAW_FULL).all()
    for r in c['sample']:                                                     # the key of row r, whatever its trip
        k = int(users[r]) if 0 <= users[r] < DRAW_USERS else 3
        if k == DRAW_FULL:
            continue
        key = draw_key(DRAW_SEED, DRAW_STEP + DRAW_COUNTER, int(r))
        if weighted:
            assert int(aux[r]) == (key * (int(c['cum'][-1]) - int(c['q'][lists[k]].sum()))) >> 64, r
        else:
            assert int(aux[r]) == ((key >> 32) * (V - len(lists[k]))) >> 32, r
            assert items[r] == c2i_np[rank_select(lists[k], aux[r])], r
    # the draw is keyed by the row number: a call of one trip gives the head of the big call
    head = draw(trip // 2)
    for got, want in zip(head, (items, look, aux)):
        np.testing.assert_array_equal(got, want[:trip // 2])


# ---------------------------------------------------------------------------------------------------------
# window.hip: k_gather_window (arx_gather_window_fwd, arx_window_slots_fwd), k_window_slots_bwd, k_site_window
# ---------------------------------------------------------------------------------------------------------
WINDOW = [(132, 5), (36, 2)]    # (d, n): the unrolled four and the tail, one row per wave / below the unroll, four rows


def _window_big(cu, d, n):
    def build():
        T = GT.window_rows(cu, d)
        mb = 2 * T + 3
        assert n * mb < 2 ** 31
        rng = np.random.default_rng(100 * n + d)
        Vf, N = 211, 150
        E = rng.standard_normal((Vf, d)).astype(np.float32)
        cmap = rng.permutation(Vf)[:N].astype(np.int32)
        ids = rng.integers(0, N, size=(n, mb)).astype(np.int32)
        base = rng.standard_normal((mb, d)).astype(np.float32)
        win = np.zeros((mb, d))
        for t in range(n):
            win += E.astype(np.float64)[cmap[ids[t]]]
        # the slot form: a permutation of n * mb rows of a block with 7 more rows that no slot names
        n_rows = n * mb + 7
        slots = rng.permutation(n_rows)[:n * mb].astype(np.int32)
        R = rng.standard_normal((n_rows, d)).astype(np.float32)
        dX = rng.standard_normal((mb, d)).astype(np.float32)
        db0 = rng.standard_normal((mb, d)).astype(np.float32)
        return dict(T=T, mb=mb, E=E, cmap=cmap, ids=ids, base=base, win=win, n_rows=n_rows, slots=slots, R=R, dX=dX,
                    db0=db0, scale=float(np.float32(0.5 / n)), base_scale=0.5)    # (the float the kernel receives)
    return _once(('window', cu, d, n), build)


def _window_asserts(cu, c, d, n):
    T, mb = c['T'], c['mb']
    assert GT.past(mb, T) and T == GT.window_rows(cu, d) and mb % 4 != 0
    assert 64 // GT.lanes_per_row(d) == {132: 1, 36: 4}[d]
    return T, mb


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("d,n", WINDOW)
def test_gather_window_past_the_grid_cap(dev, d, n, with_base):
    from arx import ops
    cu = _cu()
    c = _window_big(cu, d, n)
    T, mb = _window_asserts(cu, c, d, n)
    tE, tc, tb = _t(dev, c['E']), _t(dev, c['cmap']), _in2d(dev, c['base'])

    def call(lo, hi):
        out = _out2d(dev, hi - lo, d, SENT)
        ops.gather_window(tE, tc, _t(dev, c['ids'][:, lo:hi].reshape(-1)), n, out[1], scale=c['scale'],
                          base=tb[lo:hi] if with_base else None, base_scale=c['base_scale'])
        assert _out2d_ok(out[0], hi - lo, d)
        return _np(out[1])
    big = call(0, mb)
    want = c['scale'] * c['win'] + (c['base_scale'] * c['base'].astype(np.float64) if with_base else 0.0)
    np.testing.assert_allclose(big, want, rtol=1e-4, atol=1e-5)               # (test_window_kernels_gpu.py)
    for lo, hi in GT.slices(mb, T):
        _same_bits(call(lo, hi), big[lo:hi], "rows [%d, %d)" % (lo, hi))


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("d,n", WINDOW)
def test_window_slots_fwd_past_the_grid_cap(dev, d, n, with_base):
    import torch
    from arx import ops
    cu = _cu()
    c = _window_big(cu, d, n)
    T, mb = _window_asserts(cu, c, d, n)
    slots2 = c['slots'].reshape(n, mb)
    tR, tb = _in2d(dev, c['R']), _in2d(dev, c['base'])

    def call(lo, hi):
        out = _out2d(dev, hi - lo, d, SENT)
        ops.window_slots_fwd(tR, _t(dev, slots2[:, lo:hi].reshape(-1)), n, out[1], scale=c['scale'],
                             base=tb[lo:hi] if with_base else None, base_scale=c['base_scale'])
        assert _out2d_ok(out[0], hi - lo, d)
        return _np(out[1])
    big = call(0, mb)
    want = torch.zeros((mb, d), dtype=torch.float64)
    NumpySimilarBackend().window_slots_fwd(torch.from_numpy(c['R']), torch.from_numpy(c['slots']), n, c['scale'],
                                           torch.from_numpy(c['base']) if with_base else None, c['base_scale'], want)
    want = want.numpy()
    np.testing.assert_allclose(big, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())      # (test_sharded_w2v_gpu.py)
    for lo, hi in GT.slices(mb, T):
        _same_bits(call(lo, hi), big[lo:hi], "rows [%d, %d)" % (lo, hi))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("d,n", WINDOW)
def test_window_slots_bwd_past_the_grid_cap(dev, d, n, acc):
    """Every element is one fp32 multiply (acc: and one add): bit for bit the numpy double.  The double multiplies in
    fp64 and stores fp32 -- one rounding of an exact product; base_scale = 1/2 makes the accumulated term exact, and
    a sum of two floats rounded to 53 and then to 24 bits is the sum rounded once."""
    import torch
    from arx import ops
    cu = _cu()
    c = _window_big(cu, d, n)
    T, mb = _window_asserts(cu, c, d, n)
    n_rows = c['n_rows']
    slots2 = c['slots'].reshape(n, mb)
    tX = _in2d(dev, c['dX'])

    def call(lo, hi):
        dbase, dR = _out2d(dev, hi - lo, d, c['db0'][lo:hi]), _out2d(dev, n_rows, d, CANARY)
        ops.window_slots_bwd(tX[lo:hi], _t(dev, slots2[:, lo:hi].reshape(-1)), n, dbase[1], dR[1], scale=c['scale'],
                             base_scale=c['base_scale'], acc_dbase=bool(acc))
        assert _out2d_ok(dbase[0], hi - lo, d) and _out2d_ok(dR[0], n_rows, d)
        return _np(dbase[1]), _np(dR[1])
    gdb, gdr = call(0, mb)
    want_db = torch.from_numpy(c['db0'].copy())
    want_dr = torch.full((n_rows, d), CANARY, dtype=torch.float32)
    NumpySimilarBackend().window_slots_bwd(torch.from_numpy(c['dX']), torch.from_numpy(c['slots']), n, c['scale'],
                                           c['base_scale'], want_db, bool(acc), want_dr)
    _same_bits(gdb, want_db.numpy(), "dbase")
    _same_bits(gdr, want_dr.numpy(), "dR")
    named = np.zeros(n_rows, dtype=bool)
    named[c['slots']] = True
    assert (~named).sum() == 7 and (gdr[~named] == CANARY).all()              # rows no slot names
    for lo, hi in GT.slices(mb, T):
        pdb, pdr = call(lo, hi)
        _same_bits(pdb, gdb[lo:hi], "dbase of rows [%d, %d)" % (lo, hi))
        mine = slots2[:, lo:hi].reshape(-1)
        _same_bits(pdr[mine], gdr[mine], "dR of rows [%d, %d)" % (lo, hi))
        rest = np.ones(n_rows, dtype=bool)
        rest[mine] = False
        assert (pdr[rest] == CANARY).all()


def test_sparse_site_window_past_the_grid_cap(dev):
    import torch
    from arx import ops
    cu = _cu()
    n, row_base, coef = 5, 1000, 0.1
    trip = GT.site_window_items(cu)
    mb = -(-(2 * trip + 11) // n)                                             # n * mb >= 2 * trip + 11
    if (n * mb) % GT.BLOCK == 0:
        mb += 1
    total = n * mb
    assert GT.past(total, trip) and total % GT.BLOCK != 0 and total < 2 ** 31

    def build():
        rng = np.random.default_rng(17)
        cmap = rng.permutation(211)[:150].astype(np.int32)
        ids = rng.integers(0, 150, size=(n, mb)).astype(np.int32)
        ids[rng.random((n, mb)) < 0.02] = -1                                  # empty slots: no update
        ids[[0, 2, 4], [0, mb // 2, mb - 1]] = -1
        return cmap, ids
    cmap, ids = _once(('site', cu), build)
    tc = _t(dev, cmap)

    def call(lo, hi):
        m = n * (hi - lo)
        keys, src = _out1d(dev, m, -7, torch.int32), _out1d(dev, m, -7, torch.int32)
        cf = _out1d(dev, m, SENT)
        ops.sparse_site_window(tc, _t(dev, ids[:, lo:hi].reshape(-1)), n, row_base + lo, coef, keys[1], src[1], cf[1])
        assert int(keys[0][m].item()) == -7 and int(src[0][m].item()) == -7 and float(cf[0][m].item()) == SENT
        return (keys[1].cpu().numpy().reshape(n, -1), src[1].cpu().numpy().reshape(n, -1),
                cf[1].cpu().numpy().reshape(n, -1))
    keys, src, cf = call(0, mb)
    assert (ids < 0).sum() > 3
    np.testing.assert_array_equal(keys, np.where(ids < 0, ops.KEY_NONE, cmap[np.maximum(ids, 0)]).astype(np.int32))
    np.testing.assert_array_equal(src, np.broadcast_to(row_base + np.arange(mb, dtype=np.int32), (n, mb)))
    _same_bits(cf, np.full((n, mb), np.float32(coef)), "coef")
    for lo, hi in GT.slices(mb, trip // n):                                   # n * (hi - lo) <= trip // 2 entries
        assert n * (hi - lo) <= trip // 2
        k2, s2, c2 = call(lo, hi)
        np.testing.assert_array_equal(k2, keys[:, lo:hi])
        np.testing.assert_array_equal(s2, src[:, lo:hi])
        _same_bits(c2, cf[:, lo:hi], "coef of rows [%d, %d)" % (lo, hi))


# ---------------------------------------------------------------------------------------------------------
# slate.hip: k_slate_scores, k_slate_merge_shards
# ---------------------------------------------------------------------------------------------------------
def _slate_shapes(cu):
    """name -> ((B, C, V, d), passes): the unit loop past two trips with eight passes per run and a ragged second run
    (36 slots of 64); the `passes` branches 4 and 2; one lane per pair, 64 slots per load, four trips of rows."""
    return {'units': ((64 * cu + 5, 100, 700, 128), 8), 'passes4': ((16 * cu + 5, 100, 700, 128), 4),
            'passes2': ((10 * cu + 5, 100, 700, 128), 2), 'lane1': ((64 * cu * 4 + 3, 1, 50, 4), 8)}


def _slate_big(cu, name):
    def build():
        shape = _slate_shapes(cu)[name][0]
        B, C, V, d = shape
        assert B * C < 2 ** 31
        rng = np.random.default_rng(sum(shape))
        U, P, b = SO.dyadic(rng, B, V, d)                                     # every score is exact in float32
        cand = SO.slate(rng, B, C, V)                                         # some -1, >= V, ARX_KEY_NONE
        step = max(1, (1 << 21) // (C * d))                                   # the oracle in row blocks of 16 MB
        want = np.concatenate([SO.scores(U[i:i + step], P, b, cand[i:i + step]) for i in range(0, B, step)])
        return U, P, b, cand, want.astype(np.float32)
    return _once(('slate', cu, name), build)


def _slate_call(dev, tP, tb, U, cand):
    """arx_slate_scores into a NaN-filled view of a canary buffer; U, P and cand with wider leading dimensions."""
    import torch
    from arx import ops
    B, C = cand.shape
    cw = torch.full((B, C + 3), 1, dtype=torch.int32, device=dev)
    cw[:, :C] = _t(dev, cand)
    out = _out2d(dev, B, C, float('nan'), pad=5)
    ops.slate_scores(_in2d(dev, U), tP, tb, cw[:, :C], out[1])
    assert _out2d_ok(out[0], B, C)
    return _np(out[1])


@pytest.mark.parametrize("name", ['units', 'passes4', 'passes2', 'lane1'])
def test_slate_scores_past_the_grid_cap(dev, name):
    cu = _cu()
    (B, C, V, d), passes = _slate_shapes(cu)[name]
    plan = GT.slate_plan(cu, B, C, d)
    trip = GT.slate_units(cu)
    assert plan[0] == passes and plan[3] == B * plan[2]
    if name == 'units':
        assert plan[1:3] == (64, 2) and C % 64 == 36 and GT.past(plan[3], trip)
    elif name == 'lane1':
        assert GT.lanes_per_row(d) == 1 and plan[2] == 1 and GT.past(plan[3], trip)
    else:
        assert plan[3] > trip                                                 # these two: the planning branches
    U, P, b, cand, want = _slate_big(cu, name)
    assert (cand == -1).any() and (cand >= V).any() and np.isneginf(want).any() and np.isfinite(want[0, 0])
    tP, tb = _in2d(dev, P, pad=8), _t(dev, b)
    big = _slate_call(dev, tP, tb, U, cand)
    np.testing.assert_array_equal(big, want)                                  # exact on dyadic data; no NaN is left
    # launch-shape invariance: a row alone (one pass per run, other run lengths) carries the same bits
    nruns = plan[2]
    rows = sorted(r for r in {0, 1, trip // nruns - 1, trip // nruns, (trip + nruns - 1) // nruns, 2 * trip // nruns,
                              B - 2, B - 1} if r < B)
    assert rows[-1] == B - 1 and rows[2] > 1
    for r in rows:
        assert GT.slate_plan(cu, 1, C, d)[0] == 1
        alone = _slate_call(dev, tP, tb, U[r:r + 1], cand[r:r + 1])
        _same_bits(alone, big[r:r + 1], "row %d alone" % r)


def test_slate_scores_random_data_past_the_grid_cap(dev):
    """The 'units' shape on Gaussian data: the float32 dot bound of test_slate_scores_within_the_float32_dot_bound on
    a strided sample of rows and the rows at the ends of the trips, and the bits of those rows alone."""
    cu = _cu()
    (B, C, V, d), _ = _slate_shapes(cu)['units']
    plan, trip = GT.slate_plan(cu, B, C, d), GT.slate_units(cu)
    assert plan[0] == 8 and GT.past(plan[3], trip)
    nruns = plan[2]
    edge = [0, trip // nruns - 1, trip // nruns, 2 * trip // nruns - 1, 2 * trip // nruns, B - 1]

    def build():
        rng = np.random.default_rng(100 + d)
        U = rng.standard_normal((B, d)).astype(np.float32)
        P = rng.standard_normal((V, d)).astype(np.float32)
        b = rng.standard_normal(V).astype(np.float32)
        cand = rng.integers(-1, V + 1, size=(B, C)).astype(np.int32)
        cand[:, 3] = -1
        rows = np.unique(np.concatenate([edge, np.arange(0, B, max(1, B // 500))]))
        return U, P, b, cand, rows, SO.scores(U[rows], P, b, cand[rows]), SO.abs_scores(U[rows], P, b, cand[rows])
    U, P, b, cand, rows, ref, scale = _once(('slate_gauss', cu), build)
    tP, tb = _in2d(dev, P, pad=8), _t(dev, b)
    big = _slate_call(dev, tP, tb, U, cand)
    assert not np.isnan(big).any()
    assert np.array_equal(np.isneginf(big), (cand < 0) | (cand >= V))
    got = big[rows]
    dead = np.isneginf(ref)
    err = np.abs(np.where(dead, 0.0, got.astype(np.float64) - np.where(dead, 0.0, ref)))
    print("largest error / bound = %.3g" % float((err[~dead] / (SO.bound(d) * scale)[~dead]).max()))
    assert (err <= SO.bound(d) * scale).all()
    for r in edge:
        _same_bits(_slate_call(dev, tP, tb, U[r:r + 1], cand[r:r + 1]), big[r:r + 1], "row %d alone" % r)


def test_slate_merge_shards_past_the_grid_cap(dev):
    from arx import ops
    cu = _cu()
    W, C = 3, 5
    trip = GT.slate_merge_items(cu)
    B = -(-(2 * trip + 9) // C)                                               # B * C >= 2 * trip + 9
    if (B * C) % GT.BLOCK == 0:
        B += 1
    assert GT.past(B * C, trip) and (B * C) % GT.BLOCK != 0 and B * C < 2 ** 31

    def build():
        rng = np.random.default_rng(W)
        vals = rng.standard_normal((B, C)).astype(np.float32)
        vals[rng.random((B, C)) < 0.1] = -0.0
        owner = rng.integers(0, W, size=(B, C))
        dead = rng.random((B, C)) < 0.2                                       # -inf in every shard
        r_nan = trip // C + 3                                                 # one NaN of an owner behind the first trip
        vals[r_nan, 2], owner[r_nan, 2], dead[r_nan, 2] = np.nan, 1, False
        parts = np.full((W, B, C), -np.inf, dtype=np.float32)
        r, j = np.nonzero(~dead)
        parts[owner[r, j], r, j] = vals[r, j]
        return parts, np.where(dead, np.float32(-np.inf), vals), r_nan
    parts, want, r_nan = _once(('merge', cu), build)

    def call(lo, hi):
        out = _out2d(dev, hi - lo, C, float('nan'), pad=3)
        ops.slate_merge_shards(_t(dev, parts[:, lo:hi]), out[1])
        assert _out2d_ok(out[0], hi - lo, C)
        return _np(out[1])
    big = call(0, B)
    _same_bits(big, want, "merged")                                           # the owner's bits, -0.0 and NaN included
    assert np.isnan(big[r_nan, 2]) and np.isnan(big).sum() == 1
    for lo, hi in GT.slices(B, trip // C):
        assert (hi - lo) * C <= trip // 2
        _same_bits(call(lo, hi), big[lo:hi], "rows [%d, %d)" % (lo, hi))


# ---------------------------------------------------------------------------------------------------------
# similar.hip: k_rows_inv_norm, k_gather_rows_unit, k_cos_chunk_finish
# ---------------------------------------------------------------------------------------------------------
SIMILAR = [(200, 4), (7, 1)]    # (d, pad): the widest group of the float4 route / the scalar route, 8 rows per wave


def _similar_shape(cu, d, pad):
    vec = d % 4 == 0 and (d + pad) % 4 == 0
    T = GT.sim_rows(cu, d, vec)
    n = 2 * T + 3
    L = GT.sim_group(d, vec)
    assert GT.past(n, T) and L == {200: 64, 7: 8}[d] and vec == (d == 200) and (L == 64 or n % (64 // L) != 0)
    return T, n


@pytest.mark.parametrize("d,pad", SIMILAR)
def test_rows_inv_norm_past_the_grid_cap(dev, d, pad):
    from arx import ops
    cu = _cu()
    T, n = _similar_shape(cu, d, pad)

    def build():
        x = (np.random.default_rng(d).standard_normal((n, d)) * 3.0).astype(np.float32)
        x[[T // 2, T + 1, 2 * T + 2]] = 0.0                                   # a zero row in every trip
        return x, S.inv_norm64(x)
    x, want = _once(('inv_norm', cu, d), build)
    E = _in2d(dev, x, pad=pad)
    assert E.stride(0) == d + pad

    def call(lo, hi):
        out = _out1d(dev, hi - lo, SENT)
        ops.rows_inv_norm(E[lo:hi], out[1])
        assert float(out[0][hi - lo].item()) == SENT
        return out[1].cpu().numpy()
    big = call(0, n)
    tol = 2.0 * (d / 2.0 + 2.0) * 2.0 ** -24                                  # (test_rows_inv_norm_gaussian)
    assert np.all(np.abs(big - want) <= tol * want)
    zero = big[[T // 2, T + 1, 2 * T + 2]]
    assert not zero.any() and not np.signbit(zero).any()
    for lo, hi in GT.slices(n, T):
        _same_bits(call(lo, hi), big[lo:hi], "rows [%d, %d)" % (lo, hi))


@pytest.mark.parametrize("d,pad", SIMILAR)
def test_gather_rows_unit_past_the_grid_cap(dev, d, pad):
    import torch
    from arx import ops
    cu = _cu()
    T, B = _similar_shape(cu, d, pad)
    n_tab = 1000

    def build():
        rng = np.random.default_rng(50 + d)
        x = (rng.standard_normal((n_tab, d)) * 2.0).astype(np.float32)
        x[S.ZERO_ROW] = 0.0
        rows = rng.integers(0, n_tab, size=B).astype(np.int32)
        rows[rng.random(B) < 0.02] = -1                                       # zero rows, nothing read
        rows[[0, T - 1, T, 2 * T, B - 1]] = [-1, S.ZERO_ROW, -5, n_tab - 1, -1]
        want = torch.zeros((B, d), dtype=torch.float64)
        NumpySimilarBackend().gather_rows_unit(torch.from_numpy(x), torch.from_numpy(rows), want)
        return x, rows, want.numpy()
    x, rows, want = _once(('unit', cu, d), build)
    E, tr = _in2d(dev, x, pad=pad), _t(dev, rows)

    def call(lo, hi):
        out = _out2d(dev, hi - lo, d, SENT, pad=4)                            # ldo = d + 4
        ops.gather_rows_unit(E, tr[lo:hi], out[1])
        assert _out2d_ok(out[0], hi - lo, d)
        return _np(out[1])
    big = call(0, B)
    tol = 2.0 * (d / 2.0 + 3.0) * 2.0 ** -24                                  # (test_gather_rows_unit)
    assert np.all(np.abs(big - want) <= tol * np.abs(want) + 1e-30)
    assert not big[rows < 0].any() and not big[rows == S.ZERO_ROW].any() and (rows < 0).sum() > 3
    for lo, hi in GT.slices(B, T):
        _same_bits(call(lo, hi), big[lo:hi], "rows [%d, %d)" % (lo, hi))


def _finish_want(L, scale, col0, self_col):
    want = (L * scale[None, col0:col0 + L.shape[1]] + np.float32(0.0)).astype(np.float32)   # (test_cos_chunk_finish)
    c = self_col.astype(np.int64) - col0
    hit = (c >= 0) & (c < L.shape[1])
    want[np.nonzero(hit)[0], c[hit]] = -np.inf
    return want


@pytest.mark.parametrize("k", [1, 2])
def test_cos_chunk_finish_rows_past_the_grid_cap(dev, k):
    """B = 4096 + 5 (the row stride takes its second trip, ragged) and 2 * 4096 + 5 (its third)."""
    from arx import ops
    trip = GT.COS_FINISH_ROWS
    B, ncols, col0 = k * trip + 5, 70, 130
    assert B > k * trip and (k == 1 or GT.past(B, trip))

    def build():
        rng = np.random.default_rng(5)
        L = rng.standard_normal((B, ncols)).astype(np.float32)
        L[trip + 2, 5] = -1.5
        scale = rng.random(col0 + ncols).astype(np.float32)
        scale[col0 + 5] = 0.0                                                 # a zero column: -1.5 * 0 -> +0
        sc = np.full(B, S.KEY_NONE, dtype=np.int32)
        sc[[0, 17, trip - 1, trip, trip + 4]] = [col0, col0 + 20, col0 + ncols - 1, col0 + 3, col0 + ncols - 1]
        sc[[1, trip + 1]] = [col0 - 1, col0 + ncols]                          # just outside the chunk
        return L, scale, sc, _finish_want(L, scale, col0, sc)
    L, scale, sc, want = _once(('finish_rows', k), build)
    ts, tsc = _t(dev, scale), _t(dev, sc)

    def call(lo, hi):
        lg = _out2d(dev, hi - lo, ncols, L[lo:hi], pad=8)
        ops.cos_chunk_finish(lg[1], col0, ts, tsc[lo:hi])
        assert _out2d_ok(lg[0], hi - lo, ncols)
        return _np(lg[1])
    big = call(0, B)
    _same_bits(big, want, "finished chunk")
    assert np.isneginf(big[trip, 3]) and np.isneginf(big[trip + 4, ncols - 1]) and np.isneginf(big).sum() == 5
    assert big[trip + 2, 5] == 0.0 and not np.signbit(big[trip + 2, 5])
    for lo, hi in sorted({(0, trip // 2), (trip - trip // 4, trip + 5), (B - 5 - trip // 4, B)}):
        assert hi - lo <= trip // 2
        _same_bits(call(lo, hi), big[lo:hi], "rows [%d, %d)" % (lo, hi))


@pytest.mark.parametrize("k", [1, 2])
def test_cos_chunk_finish_columns_past_the_grid_cap(dev, k):
    """ncols = 65536 + 300 (the column stride takes its second trip, ragged) and 2 * 65536 + 300 (its third)."""
    from arx import ops
    trip = GT.COS_FINISH_COLS
    B, ncols, col0 = 2, k * trip + 300, 130
    assert ncols > k * trip and ncols % GT.BLOCK != 0 and (k == 1 or GT.past(ncols, trip))

    def build():
        rng = np.random.default_rng(6)
        L = rng.standard_normal((B, ncols)).astype(np.float32)
        scale = rng.random(col0 + ncols).astype(np.float32)
        scale[col0 + trip + 7] = 0.0
        L[0, trip + 7] = -1.5
        sc = np.array([col0 + trip + 100, col0 + 20], dtype=np.int32)         # row 0: in the second trip
        return L, scale, sc, _finish_want(L, scale, col0, sc)
    L, scale, sc, want = _once(('finish_cols', k), build)
    ts, tsc = _t(dev, scale), _t(dev, sc)

    def call(lo, hi):
        lg = _out2d(dev, B, hi - lo, L[:, lo:hi], pad=8)
        ops.cos_chunk_finish(lg[1], col0 + lo, ts, tsc)
        assert _out2d_ok(lg[0], B, hi - lo)
        return _np(lg[1])
    big = call(0, ncols)
    _same_bits(big, want, "finished chunk")
    assert np.isneginf(big[0, trip + 100]) and np.isneginf(big[1, 20]) and np.isneginf(big).sum() == 2
    assert big[0, trip + 7] == 0.0 and not np.signbit(big[0, trip + 7])
    h = trip // 2
    for lo, hi in sorted({(0, h), (trip - h // 2, trip + 300), (ncols - 299 - h // 2, ncols)}):
        assert hi - lo <= h
        _same_bits(call(lo, hi), big[:, lo:hi], "columns [%d, %d)" % (lo, hi))
