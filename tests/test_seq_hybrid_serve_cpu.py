"""Serving side of the row-striped sequence model (arx.dist.SeqHybridParallel) without a GPU: the host helpers that
re-express the logit vocabulary per shard -- col2logit and the per-shard exclusion CSR against brute force, worlds 1 to
4, on a permuted logit map with items outside the vocabulary -- the refusal of an output feature whose logit -> row
map is not injective, and the argument checks of arx_topk_softmax_merge_shards (no launch needed)."""
import numpy as np
import pytest

N_ITEMS, N_LOGITS, N_USERS = 53, 40, 17
TABLE_ROWS = N_ITEMS + 1                                   # (the START row: never a logit)


def _cmap(seed=0):
    """logit -> global table row: N_LOGITS of the N_ITEMS items, in no order."""
    rng = np.random.default_rng(seed)
    return rng.permutation(N_ITEMS)[:N_LOGITS].astype(np.int64)


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_col2logit_matches_brute_force(world):
    from arx.dist import SeqHybridParallel
    cmap = _cmap()
    rows = (TABLE_ROWS + world - 1) // world
    seen = []
    for rank in range(world):
        got = SeqHybridParallel.serve_col2logit(cmap, rows, world, rank)
        assert got.dtype == np.int32 and got.shape == (rows,)
        for lr in range(rows):
            g = lr * world + rank
            hit = np.nonzero(cmap == g)[0]
            assert got[lr] == (hit[0] if len(hit) else -1), (world, rank, lr)
        seen += [int(x) for x in got if x >= 0]
    assert sorted(seen) == list(range(N_LOGITS))            # every logit on exactly one shard


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_shard_exclusion_csr_matches_brute_force(world):
    from arx.attributes.embed_attribute import exclusion_csr
    from arx.dist import SeqHybridParallel
    cmap = _cmap(1)
    item2logit = np.full(N_ITEMS + 1, -1, dtype=np.int32)
    item2logit[cmap] = np.arange(N_LOGITS, dtype=np.int32)
    rng = np.random.default_rng(2)
    sets = {u: rng.integers(0, N_ITEMS, size=rng.integers(0, 30)).tolist() for u in range(0, N_USERS, 2)}
    sets[3] = list(range(N_ITEMS))                          # everything: every shard's whole vocabulary
    sets[5] = []
    ptr, cols = exclusion_csr(sets, N_USERS + 1, item2logit)
    total = 0
    for rank in range(world):
        p, c = SeqHybridParallel.serve_shard_csr(ptr, cols, cmap, world, rank)
        assert p.dtype == np.int32 and c.dtype == np.int32 and len(p) == N_USERS + 2 and len(c) >= 1
        for u in range(N_USERS + 1):
            want = sorted({int(i) // world for i in sets.get(u, ()) if item2logit[i] >= 0 and i % world == rank})
            assert c[p[u]:p[u + 1]].tolist() == want, (world, rank, u)
        total += int(p[-1])
    assert total == int(ptr[-1])                            # every (user, logit) pair on exactly one shard
    # the local columns name the rows col2logit maps back
    rows = (TABLE_ROWS + world - 1) // world
    for rank in range(world):
        p, c = SeqHybridParallel.serve_shard_csr(ptr, cols, cmap, world, rank)
        c2l = SeqHybridParallel.serve_col2logit(cmap, rows, world, rank)
        assert (c2l[c[:p[-1]]] >= 0).all()
    # no lists at all: empty pointers, one dummy column
    p, c = SeqHybridParallel.serve_shard_csr(np.zeros(N_USERS + 2, dtype=np.int32), np.zeros(1, dtype=np.int32), cmap,
                                             world, 0)
    assert not p.any() and len(c) == 1


def test_non_injective_output_feature_is_refused():
    from arx.dist import SeqHybridParallel
    cmap = _cmap()
    cmap[7] = cmap[3]                                       # two logits on one table row (an attribute feature)
    with pytest.raises(NotImplementedError, match="injective"):
        SeqHybridParallel.serve_col2logit(cmap, TABLE_ROWS, 1, 0)
    with pytest.raises(ValueError):
        SeqHybridParallel.serve_col2logit(np.asarray([0, TABLE_ROWS + 5]), TABLE_ROWS, 1, 0)


def test_topk_softmax_merge_shards_argument_validation_without_gpu():
    """arx_topk_softmax_merge_shards refuses null pointers, W outside [1, 64] and k outside [1, 1024] before any launch
    (small integers stand in for device pointers: they are only compared with NULL); lse_out may be NULL."""
    from arx import _lib
    lib = _lib.lib
    EINVAL = -1
    f = lib.arx_topk_softmax_merge_shards

    def err():
        m = lib.arx_last_error()
        return m.decode() if m else ""
    # (v, id, lse_part, B, W, k, po, io, lse_out)
    for args in ((None, 1, 1, 4, 2, 10, 1, 1, 1), (1, None, 1, 4, 2, 10, 1, 1, 1), (1, 1, None, 4, 2, 10, 1, 1, 1),
                 (1, 1, 1, 4, 2, 10, None, 1, 1), (1, 1, 1, 4, 2, 10, 1, None, 1), (1, 1, 1, 4, 0, 10, 1, 1, 1),
                 (1, 1, 1, 4, 65, 10, 1, 1, 1), (1, 1, 1, 4, 2, 0, 1, 1, 1), (1, 1, 1, 4, 2, 1025, 1, 1, 1),
                 (1, 1, 1, -1, 2, 10, 1, 1, 1)):
        assert f(*args, None) == EINVAL, args
        assert "arx_topk_softmax_merge_shards" in err()
    assert f(1, 1, 1, 0, 64, 1024, 1, 1, 1, None) == 0       # B = 0: nothing to do, no launch
    assert f(1, 1, 1, 0, 1, 1, 1, 1, None, None) == 0        # ... and without lse_out
