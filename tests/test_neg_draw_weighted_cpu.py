"""The host half of the weighted pair draw (arx_neg_draw_weighted, csrc/pair.hip) without a GPU: the export's argument
validation, the two-search statement in numpy against a brute-force masked cumulative sum, the host tables
(arx.utils.prepare_train.pair_draw_tables), and ShardedHMF.prepare_pair_negatives(power=...) on two gloo ranks over the
numpy compute double."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MASK64 = (1 << 64) - 1


def mix64(z):
    """csrc/common.h mix64 in Python integers: all 64 bits of the splitmix64 finaliser (mix32 is its high half)."""
    z = (z + 0x9e3779b97f4a7c15) & MASK64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK64
    return z ^ (z >> 31)


def draw_key(seed, step, r):
    """The 64-bit random number of row r: the keying of arx_neg_draw_uniform / arx_neg_draw_weighted."""
    s = (seed + step * 0x9e3779b97f4a7c15) & MASK64
    return mix64((s * 0x100000001b3 + r) & MASK64)


def eligible_mass(cum, lst):
    q = np.diff(np.asarray(cum, dtype=np.int64))
    return int(cum[-1]) - int(q[np.asarray(lst, dtype=np.int64)].sum())


def brute(cum, lst, t):
    """The column that holds point t of the eligible mass: the weights of the listed columns are set to zero and the
    first column whose running sum exceeds t is taken -- the independent statement of the draw."""
    q = np.diff(np.asarray(cum, dtype=np.int64)).copy()
    q[np.asarray(lst, dtype=np.int64)] = 0
    return int(np.searchsorted(np.cumsum(q), t, side='right'))


def two_search(cum, lst, t):
    """The statement the kernel evaluates: a = #{ j : cum[p_j] - H(j) <= t }, then the largest c < V with
    cum[c] <= t + H(a)."""
    cum = np.asarray(cum, dtype=np.int64)
    lst = np.asarray(lst, dtype=np.int64)
    V = len(cum) - 1
    H = np.zeros(len(lst) + 1, dtype=np.int64)
    np.cumsum(cum[lst + 1] - cum[lst], out=H[1:])
    below = cum[lst] - H[:-1]
    assert (np.diff(below) >= 0).all()
    a = int(np.searchsorted(below, t, side='right'))
    return int(np.searchsorted(cum[:V], t + H[a], side='right')) - 1


def test_weighted_draw_export_validates_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib
    EINVAL = -1

    def err():
        m = lib.arx_last_error()
        return m.decode() if m else ""
    P = 4096          # (pointers are only compared with NULL before the first HIP call)

    def draw(users=P, B=8, n_users=4, ptr=P, cols=P, ex_cum=P, cum=P, V=100, out=P):
        return lib.arx_neg_draw_weighted(users, B, n_users, ptr, cols, ex_cum, cum, V, None, 0, None, 0, out, None,
                                         None, None)
    for bad in (dict(users=None), dict(ptr=None), dict(cols=None), dict(ex_cum=None), dict(cum=None), dict(out=None),
                dict(B=-1), dict(n_users=-1), dict(V=0), dict(V=-3), dict(V=1 << 31)):
        assert draw(**bad) == EINVAL and "arx_neg_draw_weighted" in err(), bad
    assert draw(B=0) == 0


def test_two_searches_find_the_column_of_the_masked_cumulative_sum():
    """Every point t of the eligible mass, over random small weights (zeros next to list entries included) and random
    lists: the two binary searches name the column the masked running sum names, it is outside the list and it has
    weight."""
    rng = np.random.default_rng(0)
    n = 0
    for case in range(300):
        V = int(rng.integers(1, 13))
        q = rng.choice(np.asarray([0, 0, 1, 1, 2, 3, 7]), size=V)
        cum = np.concatenate([[0], np.cumsum(q)]).astype(np.int64)
        lst = np.sort(rng.choice(V, size=int(rng.integers(0, V + 1)), replace=False))
        M = eligible_mass(cum, lst)
        assert M == int(np.delete(q, lst).sum())
        for t in range(M):
            col = two_search(cum, lst, t)
            assert col == brute(cum, lst, t), (q, lst, t)
            assert col not in set(lst.tolist()) and q[col] > 0
            n += 1
    assert n > 2000
    # 64-bit masses: the heaviest weight is 2^32 and the whole exceeds it
    q = np.asarray([1 << 32, 0, 5, 1 << 32, 0, 0, (1 << 32) - 1, 1], dtype=np.int64)
    cum = np.concatenate([[0], np.cumsum(q)]).astype(np.int64)
    for lst in ([], [0], [3, 6], [1, 2, 4], [0, 3, 6, 7]):
        M = eligible_mass(cum, lst)
        edge = [t for t in (0, 1, 4, 5, M // 3, M // 2, M - 2, M - 1) if 0 <= t < M]
        for t in edge + [int(x) for x in rng.integers(0, M, size=50)]:
            assert two_search(cum, lst, t) == brute(cum, lst, t), (lst, t)


def test_multiply_high_of_64_bits_covers_the_mass():
    for M in (1, 3, (1 << 32) + 5, (1 << 62) + 1):
        assert (0 * M) >> 64 == 0 and (MASK64 * M) >> 64 == M - 1
    assert mix64(0) >> 32 == 0xe220a839 and mix64(0) == 0xe220a8397b1dcdaf          # splitmix64's first output


def test_pair_draw_tables_check_their_arguments():
    from arx.utils.prepare_train import pair_draw_tables
    ptr, cols = np.asarray([0, 2, 2]), np.asarray([1, 3])
    counts = np.asarray([4, 0, 9, 1])
    cum, ex_cum = pair_draw_tables(counts, 1.0, 0.0, ptr, cols)
    assert cum.dtype == np.int64 and ex_cum.dtype == np.int64
    q = np.diff(cum)
    assert cum[0] == 0 and q[2] == 1 << 32 and q[1] == 0 and q[3] == (1 << 32) // 9
    np.testing.assert_array_equal(ex_cum, [0, 0])                     # H(0) = 0, H(1) = q[1] = 0
    assert (np.diff(pair_draw_tables(counts, 0.0, 0.0, ptr, cols)[0]) == [1 << 32, 0, 1 << 32, 1 << 32]).all()
    with pytest.raises(ValueError):
        pair_draw_tables(np.zeros(4), 0.75, 0.0, ptr, cols)           # every weight zero
    with pytest.raises(ValueError):
        pair_draw_tables(np.zeros(4), 0.0, 0.0, ptr, cols)            # (power 0 does not revive a zero count)
    with pytest.raises(ValueError):
        pair_draw_tables(counts, -0.5, 1.0, ptr, cols)
    with pytest.raises(ValueError):
        pair_draw_tables(counts, 0.75, -1.0, ptr, cols)
    # a tiny weight keeps one quantum
    assert np.diff(pair_draw_tables(np.asarray([1, 10 ** 12]), 1.0, 0.0, [0, 0], [0])[0])[0] == 1


def test_pair_draw_tables_match_their_restatement():
    """power 0 and 1 involve no rounding beyond one divide and one multiply by 2^32: equal to the direct statement.
    power 0.75: the double and the long-double evaluation are both within a few ulp of a value below 2^32, whose
    double spacing is at most 2^-20 -- their floors differ by at most one quantum.  (Needs no device.)"""
    from arx.utils.prepare_train import pair_draw_tables
    rng = np.random.default_rng(4)
    V = 1000
    counts = rng.integers(0, 5000, V)
    counts[rng.choice(V, 100, replace=False)] = 0
    lists = [np.sort(rng.choice(V, n, replace=False)) for n in (0, 1, 40, V, 7)]
    ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    cols = np.concatenate(lists)
    for power, smooth in ((0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (0.75, 0.0), (0.75, 1.0)):
        cum, ex_cum = pair_draw_tables(counts, power, smooth, ptr, cols)
        q = np.diff(cum)
        base = counts + smooth
        if power == 0.0:
            want = np.where(base == 0, 0, 1 << 32)
        elif power == 1.0:
            want = np.where(base == 0, 0, np.maximum(1, np.floor(base / base.max() * 2.0 ** 32))).astype(np.int64)
        if power in (0.0, 1.0):
            np.testing.assert_array_equal(q, want)
        else:
            w = np.power(base.astype(np.longdouble), np.longdouble(0.75))
            ref = np.where(base == 0, 0, np.maximum(1, np.floor(w / w.max() * np.longdouble(2.0) ** 32)))
            assert np.abs(q - ref.astype(np.int64)).max() <= 1
            assert ((q == 0) == (base == 0)).all() and q.max() == 1 << 32
        assert cum[0] == 0 and cum.dtype == np.int64 and len(cum) == V + 1
        np.testing.assert_array_equal(cum[1:], np.cumsum(q))
        for k, lst in enumerate(lists):                      # exact prefix sums along every list
            np.testing.assert_array_equal(ex_cum[ptr[k]:ptr[k + 1]],
                                          np.concatenate([[0], np.cumsum(q[lst])])[:len(lst)].astype(np.int64))


# ---------------------------------------------------------------------------------------------- two gloo ranks
N_USERS, N_ITEMS, D, B_LOC, LR = 60, 90, 16, 8, 0.5
ONLY_RANK1, UNSEEN = 11, 23          # an item only rank 1's users have seen; an item nobody has seen


def _weighted_backend():
    from numpy_backend import _n
    from numpy_backend_pair import NumpyPairBackend

    class Backend(NumpyPairBackend):
        def neg_draw_weighted(self, urows, ex_ptr, ex_cols, ex_cum, cum, V, seed, counter, out):
            """The masked cumulative sum (the statement of arx_neg_draw_weighted; the random numbers are numpy's,
            keyed by (seed, counter)); -1 where no weight is left outside the list."""
            ptr, cols, c = _n(ex_ptr), _n(ex_cols), _n(cum).astype(np.int64)
            assert len(c) == int(V) + 1 and len(_n(ex_cum)) == len(cols)
            rng = np.random.default_rng([int(seed) & 0xFFFFFFFF, int(seed) >> 32, int(counter)])
            o = _n(out)
            for r, u in enumerate(_n(urows)):
                lst = cols[ptr[u]:ptr[u + 1]].astype(np.int64)
                assert (np.diff(lst) > 0).all(), "the draw needs sorted, unique lists"
                np.testing.assert_array_equal(_n(ex_cum)[ptr[u]:ptr[u + 1]],
                                              np.concatenate([[0], np.cumsum(np.diff(c)[lst])])[:len(lst)])
                M = eligible_mass(c, lst)
                o[r] = brute(c, lst, int(rng.integers(0, M))) if M > 0 else -1
    return Backend()


def _global_lists():
    """{user: items} of the synthetic positives with UNSEEN taken out everywhere, ONLY_RANK1 taken out of the even
    users (rank 0 of two) and given to user 1."""
    from arx.utils.synthetic import SyntheticHMF
    syn = SyntheticHMF(n_users=N_USERS, n_items=N_ITEMS, seed=1, permute_logits=False, n_pos=6)
    lists = {}
    for u in range(N_USERS):
        its = [int(v) for v in syn.pos_items[syn.pos_ptr[u]:syn.pos_ptr[u + 1]]]
        its = [v for v in its if v != UNSEEN and not (v == ONLY_RANK1 and u % 2 == 0)]
        lists[u] = its + ([ONLY_RANK1] if u == 1 else [])
    return syn, lists


def _weighted_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from arx.dist import ShardedHMF
    from arx.utils.prepare_train import pair_draw_tables
    syn, lists = _global_lists()
    params = syn.glorot_params(D, seed=2, scale=0.5)
    tables = {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
              'item_bias': params['item_bias_cat_0'][2:]}
    model = ShardedHMF(N_USERS, N_ITEMS, D, B_LOC, 0, LR, rank, world, 'cpu', backend=_weighted_backend(),
                       tables=tables, loss='bpr', seed=7)
    own = np.arange(rank, N_USERS, world)
    ptr, items = np.zeros(len(own) + 2, dtype=np.int32), []
    for k, u in enumerate(own):
        items.extend(lists[int(u)][::-1] + lists[int(u)][:1])            # unsorted, one entry doubled
        ptr[k + 1] = len(items)
    ptr[-1] = ptr[-2]
    model.set_positives(ptr, np.asarray(items, dtype=np.int32))
    model.prepare_pair_negatives(power=0.75, smooth=0.0)
    ex_cum, cum = (t.numpy() for t in model._neg_tables)
    # every rank holds the table of the GLOBAL counts
    counts = np.zeros(N_ITEMS, dtype=np.int64)
    for u, its in lists.items():
        counts[np.unique(its)] += 1
    assert counts[UNSEEN] == 0 and counts[ONLY_RANK1] > 0
    want_cum, _ = pair_draw_tables(counts, 0.75, 0.0, [0, 0], [0])
    np.testing.assert_array_equal(cum, want_cum)
    both = [None] * world
    dist.all_gather_object(both, cum.tolist())
    assert both[0] == both[1]
    q = np.diff(cum)
    assert q[ONLY_RANK1] > 0 and q[UNSEEN] == 0           # on rank 0 too, whose users never saw ONLY_RANK1
    if rank == 0:
        assert all(ONLY_RANK1 not in lists[int(u)] for u in own)
    rng = np.random.default_rng(20 + rank)
    seq = []
    for step in range(4):
        u = rng.choice(own, size=B_LOC).astype(np.int32)
        it = rng.integers(0, N_ITEMS, size=B_LOC).astype(np.int32)
        route = model.prepare_route(u, it)
        ng = route['neg_items'].numpy()
        assert (ng >= 0).all() and ng.max() < N_ITEMS
        assert all(int(ng[r]) not in lists[int(u[r])] for r in range(B_LOC))       # outside the LOCAL histories
        assert (counts[ng] > 0).all()                                              # smooth 0: no unseen item
        model.step(route)
        assert np.isfinite(float(model.read_loss().item()))
        seq.append(ng.copy())
    assert any((seq[i] != seq[i + 1]).any() for i in range(3))
    # explicit counts need no collective; without power the draw is the uniform one again
    model.prepare_pair_negatives(power=1.0, smooth=1.0, counts=np.arange(N_ITEMS))
    np.testing.assert_array_equal(model._neg_tables[1].numpy(),
                                  pair_draw_tables(np.arange(N_ITEMS), 1.0, 1.0, [0, 0], [0])[0])
    with pytest.raises(ValueError, match="counts"):
        model.prepare_pair_negatives(power=1.0, counts=np.ones(N_ITEMS - 1))
    model.prepare_pair_negatives()
    assert model._neg_tables is None
    assert (model.prepare_route(u, it)['neg_items'].numpy() >= 0).all()
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_sharded_weighted_draw_shares_one_table_over_two_gloo_ranks(tmp_path):
    import torch.multiprocessing as mp
    port = 29300 + (os.getpid() % 400)
    mp.spawn(_weighted_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))
