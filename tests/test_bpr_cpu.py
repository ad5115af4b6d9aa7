"""The host half of the pairwise losses 'bpr' / 'bpr-hinge' (csrc/pair.hip): argument validation of the three exports
without a device, and the rank-select identity of the negative draw stated in numpy."""
import numpy as np


def rank_select(cols, k):
    """The k-th (from 0) column that is NOT in the sorted, unique list `cols`: k + #{j : cols[j] - j <= k} -- the
    statement arx_neg_draw_uniform evaluates with one binary search (cols[j] - j does not decrease with j)."""
    cols = np.asarray(cols, dtype=np.int64)
    shifted = cols - np.arange(len(cols))
    assert (np.diff(shifted) >= 0).all()
    return int(k) + int(np.searchsorted(shifted, k, side='right'))


def test_pair_exports_validate_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib
    EINVAL = -1

    def err():
        m = lib.arx_last_error()
        return m.decode() if m else ""
    # (pointers are only compared with NULL and checked for alignment before the first HIP call: multiples of 16
    # stand in for them)
    P = 4096

    def pair(U=P, B=8, d=64, kind=0, ld=64, grads=(None, None, None, None, None)):
        dU, dP, dpb, dN, dnb = grads
        return lib.arx_pair_loss_fwdbwd(U, ld, P, ld, P, P, ld, P, None, None, B, d, kind, 1.0, P, P, P,
                                        dU, ld, 0, dP, ld, dpb, dN, ld, dnb, None)
    assert pair(U=None) == EINVAL and "arx_pair_loss_fwdbwd" in err()
    assert pair(d=62) == EINVAL and "arx_pair_loss_fwdbwd" in err() and "d=62" in err()
    assert pair(kind=2) == EINVAL and "arx_pair_loss_fwdbwd" in err()
    assert pair(B=-1) == EINVAL and "arx_pair_loss_fwdbwd" in err()
    assert pair(ld=66) == EINVAL and "arx_pair_loss_fwdbwd" in err()                 # leading dim % 4
    assert pair(U=P + 4) == EINVAL and "arx_pair_loss_fwdbwd" in err()               # 16-byte alignment
    assert pair(grads=(P, P, None, P, P)) == EINVAL and "arx_pair_loss_fwdbwd" in err()   # some, not all
    assert pair(B=0) == 0
    assert pair(B=0, grads=(P, P, P, P, P)) == 0

    assert lib.arx_pair_auc(None, P, None, 8, P, None) == EINVAL and "arx_pair_auc" in err()
    assert lib.arx_pair_auc(P, P, None, 8, None, None) == EINVAL and "arx_pair_auc" in err()
    assert lib.arx_pair_auc(P, P, None, -1, P, None) == EINVAL and "arx_pair_auc" in err()
    assert lib.arx_pair_auc(P, P, None, 0, P, None) == 0

    def draw(users=P, B=8, n_users=4, V=100, out=P):
        return lib.arx_neg_draw_uniform(users, B, n_users, P, P, V, None, 0, None, 0, out, None, None, None)
    assert draw(users=None) == EINVAL and "arx_neg_draw_uniform" in err()
    assert draw(out=None) == EINVAL and "arx_neg_draw_uniform" in err()
    assert draw(B=-1) == EINVAL and "arx_neg_draw_uniform" in err()
    assert draw(V=0) == EINVAL and "arx_neg_draw_uniform" in err()
    assert draw(V=1 << 31) == EINVAL and "arx_neg_draw_uniform" in err()
    assert draw(B=0) == 0


def test_rank_select_is_the_kth_column_outside_the_list():
    V = 12
    lists = [[], [c for c in range(V) if c != 5], [0, 1, 2, 3], [8, 9, 10, 11], [0], [V - 1], [1, 4, 5, 9],
             list(range(V - 1)), list(range(1, V))]
    for cols in lists:
        free = [c for c in range(V) if c not in set(cols)]          # brute force
        assert len(free) == V - len(cols)
        for k in range(len(free)):
            assert rank_select(cols, k) == free[k], (cols, k)


def test_multiply_high_covers_every_rank():
    """k = (rand32 * n_elig) >> 32 lies in [0, n_elig) and reaches both ends."""
    for n in (1, 2, 37, 1000003):
        for r, want in ((0, 0), (2 ** 32 - 1, n - 1)):
            assert (r * n) >> 32 == want
