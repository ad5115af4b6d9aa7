"""similar_items of the row-sharded models on the device, world 1 (an nccl group of one): ShardedHMF and ShardedW2V on
exact data (ids and cosines equal to the float64 oracle, ties included) and on Gaussian tables (the random rule at
atol = 2 (d + 4) 2^-24), ShardedHMFRepTokens through its serving view.  Shards of about 1500 rows with a first chunk
of 128 columns (HipBackend.sim_chunk), so the fused filter GEMM runs behind it; d = 64 and 128."""
import os

import numpy as np
import pytest

import similar_oracle as S
from test_kernels_direct_gpu import _t

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, B_LOC = 50, 1503, 16


def _init_world1(dev, port):
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)


def _model(kind, dev, d):
    from arx import dist as adist
    if kind == 'hmf':
        m = adist.ShardedHMF(N_USERS, N_ITEMS, d, B_LOC, 64, 0.1, 0, 1, dev, graphs=False)
    else:
        m = adist.ShardedW2V(N_USERS, N_ITEMS, d, B_LOC, 64, 2, 0.1, 0, 1, dev, cbow=True, loss='mw', graphs=False)
    m.be.sim_chunk = 128
    return m


def _fused_ran(model):
    scans = list(model.be._sim_scans.values())
    return bool(scans) and all(s.fused and int(s.overflow.item()) == 0 for s in scans)


@pytest.mark.parametrize("kind", ['hmf', 'w2v'])
@pytest.mark.parametrize("d", [64, 128])
def test_sharded_similar_world1(dev, kind, d):
    import torch.distributed as dist
    _init_world1(dev, 29791)
    try:
        model = _model(kind, dev, d)
        rng = np.random.default_rng(d)
        # ---- exact data: the oracle's ids and values, bit for bit
        E = S.exact_table(rng, N_ITEMS, d)
        model.E_item[:N_ITEMS].copy_(_t(dev, E))
        q = np.array([0, 1, 2, 3, S.ZERO_ROW, 5, 700, 700, N_ITEMS - 1], dtype=np.int64)
        C = S.cos64(E[q], E)
        for include_self in (False, True):
            for k in (1, 12):
                ids, vals = model.similar_items(q, k, include_self=include_self, return_values=True)
                wv, wi = S.topk_cos(C, k, None if include_self else q)
                np.testing.assert_array_equal(ids.cpu().numpy(), wi)
                np.testing.assert_array_equal(vals.cpu().numpy().astype(np.float64), wv)
        assert _fused_ran(model)
        ids, vals = model.similar_items(q[:2], 1024, return_values=True)
        np.testing.assert_array_equal(ids.cpu().numpy(), S.topk_cos(C[:2], 1024, q[:2])[1])
        assert tuple(model.similar_items(q[:0], 5).shape) == (0, 5)                 # a rank without queries
        # ---- Gaussian data: the random rule
        G = rng.standard_normal((N_ITEMS, d)).astype(np.float32)
        model.E_item[:N_ITEMS].copy_(_t(dev, G))
        q = rng.choice(N_ITEMS, B_LOC, replace=False)
        ids, vals = model.similar_items(q, 12, return_values=True)
        worst = S.check_random(ids.cpu().numpy(), vals.cpu().numpy(), S.cos64(G[q], G), 12, q, S.cos_atol(d))
        assert np.array_equal(model.similar_items(q, 3, include_self=True).cpu().numpy()[:, 0], q)
        print("%s d=%d: largest |cosine - float64| = %.3g (bound %.3g)" % (kind, d, worst, S.cos_atol(d)))
        with pytest.raises(ValueError):
            model.similar_items([N_ITEMS], 3)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("d", [64, 128])
def test_rep_tokens_similar_items_through_the_view(dev, d):
    import torch
    import torch.distributed as dist
    from arx import dist as adist
    _init_world1(dev, 29793)
    try:
        n_tok = 300
        rng = np.random.default_rng(31 + d)
        lens = rng.integers(1, 9, size=N_ITEMS).astype(np.int32)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
        bags = (rng.integers(0, n_tok, size=int(lens.sum())).astype(np.int32), starts, lens)
        model = adist.ShardedHMFRepTokens(N_USERS, N_ITEMS, d, B_LOC, 64, 0.1, 0, 1, dev, bags, n_tok, seed=3,
                                          graphs=False)
        model.be.sim_chunk = 128
        q = rng.choice(N_ITEMS, B_LOC - 3, replace=False)
        ids, vals = model.similar_items(q, 12, return_values=True)
        view = model._sim_view
        assert isinstance(view, adist.ShardedHetView) and view.n_refresh == 1
        # the latents the view materialised: 1/2 (id row + bag mean), and the cosines over them
        L = view.E_item[:N_ITEMS].cpu().numpy()
        Eid, Etok = model.E_item.cpu().numpy().astype(np.float64), model.E_tok.cpu().numpy().astype(np.float64)
        host = np.stack([0.5 * (Eid[j] + Etok[bags[0][starts[j]:starts[j] + lens[j]]].mean(0))
                         for j in range(N_ITEMS)])
        np.testing.assert_allclose(L, host, rtol=1e-5, atol=1e-7)
        worst = S.check_random(ids.cpu().numpy(), vals.cpu().numpy(), S.cos64(L[q], L), 12, q, S.cos_atol(d))
        assert _fused_ran(model) and view.n_refresh == 1
        inc = model.similar_items(q, 2, include_self=True)
        assert torch.equal(inc[:, 0].cpu(), torch.from_numpy(q).int()) and view.n_refresh == 1
        print("rep-tokens d=%d: largest |cosine - float64| = %.3g (bound %.3g)" % (d, worst, S.cos_atol(d)))
    finally:
        dist.destroy_process_group()
