"""The GRU encoder's host half (no GPU).

 1. include/arx_gru.h against GRU_PROTOTYPES of arx/_lib.py by TYPE, with the parser and the comparator of
    tests/test_abi_signatures_cpu.py; arx.h includes the header and the library exports the two symbols;
 2. tests/gru_oracle.py: its gradients against torch.autograd on a float64 torch restatement of the same three lines
    (L in {1, 3}, B = 4, din = 6, h = 8, to 1e-12), and its forward against two hand-unrolled steps;
 3. arx_gru_fwd / arx_gru_bwd refuse bad arguments with ARX_EINVAL and a message before any HIP call;
 4. tests/gru_paths.py agrees with itself on the shapes the GPU matrix uses.
"""
import os

import numpy as np
import pytest

import gru_oracle as GO
import gru_paths as GP

EINVAL = -1


# ---------------------------------------------------------------- 1. the ABI
def test_gru_header_and_its_table_stay_in_step():
    import test_abi_signatures_cpu as A
    from arx import _lib
    decls = A.parse_header(open(os.path.join(A.ROOT, "include", "arx_gru.h")).read())
    assert sorted(decls) == ["arx_gru_bwd", "arx_gru_fwd"]
    lines = open(os.path.join(A.ROOT, "a-recsys_amd", "arx", "_lib.py")).read().split("\n")
    end = next(i for i, l in enumerate(lines) if l.startswith("class ArxError"))
    ns = {"__file__": "_lib.py"}
    exec(compile("\n".join(l for l in lines[:end] if not l.startswith("import torch")), "_lib.py(gru)", "exec"), ns)
    protos = ns["GRU_PROTOTYPES"]
    assert sorted(protos) == sorted(decls) == sorted(_lib.GRU_PROTOTYPES)
    bad = [m for name in sorted(decls) for m in A.mismatches(name, decls[name], protos[name])]
    assert not bad, "\n".join(bad)
    # not vacuous: one i64 narrowed to i32 is reported
    res, args = protos["arx_gru_fwd"]
    k64 = next(k for k, a in enumerate(args) if a is A.C.c_int64)
    narrowed = list(args)
    narrowed[k64] = A.C.c_int32
    assert A.mismatches("arx_gru_fwd", decls["arx_gru_fwd"], (res, narrowed))
    for name in decls:
        assert hasattr(_lib.lib, name) and name not in _lib.PROTOTYPES
        assert getattr(_lib.lib, name).argtypes == list(protos[name][1])
    assert '#include "arx_gru.h"' in open(os.path.join(A.ROOT, "include", "arx.h")).read()


def test_ops_wrappers_exist():
    from arx import ops
    assert callable(ops.gru_fwd) and callable(ops.gru_bwd)


# ---------------------------------------------------------------- 2. the oracle
def _inputs(L, B, din, h, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((L, B, din)) * 0.5
    Wg = rng.standard_normal((din + h, 2 * h)) * 0.3
    bg = rng.standard_normal(2 * h) * 0.1 + 1.0
    Wc = rng.standard_normal((din + h, h)) * 0.3
    bc = rng.standard_normal(h) * 0.1
    dhs = rng.standard_normal((L, B, h))
    return x, Wg, bg, Wc, bc, dhs


def _torch_gru(x, Wg, bg, Wc, bc):
    import torch
    L, B, _ = x.shape
    h = Wc.shape[1]
    hp = torch.zeros((B, h), dtype=torch.float64)
    out = []
    for t in range(L):
        g = torch.sigmoid(torch.cat([x[t], hp], 1) @ Wg + bg)
        r, u = g[:, :h], g[:, h:]
        c = torch.tanh(torch.cat([x[t], r * hp], 1) @ Wc + bc)
        hp = u * hp + (1 - u) * c
        out.append(hp)
    return torch.stack(out)


@pytest.mark.parametrize("L", [1, 3])
def test_oracle_gradients_against_autograd(L):
    import torch
    B, din, h = 4, 6, 8
    x, Wg, bg, Wc, bc, dhs = _inputs(L, B, din, h, 10 + L)
    hs, gates, rh = GO.gru_fwd(x, Wg, bg, Wc, bc)
    assert hs.dtype == np.float64
    _, _, dx, dWg, dbg, dWc, dbc = GO.gru_bwd(x, Wg, Wc, hs, gates, dhs)
    ts = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, Wg, bg, Wc, bc)]
    ths = _torch_gru(*ts)
    np.testing.assert_allclose(hs, ths.detach().numpy(), rtol=0, atol=1e-12)
    (ths * torch.tensor(dhs)).sum().backward()
    for name, got, t in (('dx', dx, ts[0]), ('dWg', dWg, ts[1]), ('dbg', dbg, ts[2]), ('dWc', dWc, ts[3]),
                         ('dbc', dbc, ts[4])):
        np.testing.assert_allclose(got, t.grad.numpy(), rtol=0, atol=1e-12, err_msg=name)
    if L == 1:                  # the zero state: no gradient reaches the h rows of either matrix
        assert not dWg[din:].any() and not dWc[din:].any() and not rh.any()


def test_oracle_forward_two_hand_unrolled_steps():
    B, din, h = 4, 6, 8
    x, Wg, bg, Wc, bc, _ = _inputs(2, B, din, h, 3)
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    # step 0: h_{-1} = 0, so only the x rows of the weights matter and r * h_prev = 0
    g0 = sig(x[0] @ Wg[:din] + bg)
    c0 = np.tanh(x[0] @ Wc[:din] + bc)
    h0 = (1.0 - g0[:, h:]) * c0
    # step 1
    g1 = sig(x[1] @ Wg[:din] + h0 @ Wg[din:] + bg)
    rh1 = g1[:, :h] * h0
    c1 = np.tanh(x[1] @ Wc[:din] + rh1 @ Wc[din:] + bc)
    h1 = g1[:, h:] * h0 + (1.0 - g1[:, h:]) * c1
    hs, gates, rh = GO.gru_fwd(x, Wg, bg, Wc, bc)
    np.testing.assert_allclose(hs[0], h0, rtol=0, atol=1e-14)
    np.testing.assert_allclose(hs[1], h1, rtol=0, atol=1e-14)
    np.testing.assert_allclose(gates[1], np.concatenate([g1, c1], 1), rtol=0, atol=1e-14)
    np.testing.assert_allclose(rh[1], rh1, rtol=0, atol=1e-14)
    assert not rh[0].any()


def test_oracle_keeps_float32():
    a = [v.astype(np.float32) for v in _inputs(2, 3, 4, 5, 1)]
    hs, gates, rh = GO.gru_fwd(*a[:5])
    outs = GO.gru_bwd(a[0], a[1], a[3], hs, gates, a[5])
    assert all(o.dtype == np.float32 for o in (hs, gates, rh) + tuple(outs))


# ---------------------------------------------------------------- 3. the C ABI without a GPU
def _err(lib):
    m = lib.arx_last_error()
    return m.decode() if m else ""


def test_gru_argument_validation_without_gpu():
    from arx import _lib
    lib = _lib.lib
    P = 256                                   # stands in for a device pointer: only compared with NULL
    fwd, bwd = lib.arx_gru_fwd, lib.arx_gru_bwd
    #        x  Wg bg Wc bc  L  B  din h   hs gates rh stream
    good_f = [P, P, P, P, P, 3, 5, 6, 8, P, P, P, None]
    #        Wg Wc hs gates dhs L  B  din h  dzg dzc stream
    good_b = [P, P, P, P, P, 3, 5, 6, 8, P, P, None]
    for f, good, ptrs, name in ((fwd, good_f, (0, 1, 2, 3, 4, 9, 10, 11), "arx_gru_fwd"),
                                (bwd, good_b, (0, 1, 2, 3, 4, 9, 10), "arx_gru_bwd")):
        for k in ptrs:
            a = list(good)
            a[k] = None
            assert f(*a) == EINVAL, (name, k)
            assert name + ": null pointer" in _err(lib)
        for k, v in ((5, -1), (6, -1), (7, 0), (7, -4), (8, 0), (8, -64)):
            a = list(good)
            a[k] = v
            assert f(*a) == EINVAL, (name, k, v)
            assert name + ": bad size" in _err(lib)
        # the generic path's LDS demand past 160 KB (forward 4 * (din + 4h), backward 4 * 5h bytes)
        a = list(good)
        a[7], a[8] = 4, 10241
        assert GP.path(4, 10241) == 'generic'
        assert GP.fwd_lds_bytes(4, 10241) > GP.LDS_LIMIT and GP.bwd_lds_bytes(10241, 'generic') > GP.LDS_LIMIT
        assert f(*a) == EINVAL, name
        assert name + ": sizes exceed LDS" in _err(lib)
        # the streaming path's: din = 4096 at h = 128
        if f is fwd:
            a[7], a[8] = 4096, 128
            assert GP.fwd_lds_bytes(4096, 128) > GP.LDS_LIMIT
            assert f(*a) == EINVAL and "sizes exceed LDS" in _err(lib)
        # nothing to do is not an error (and launches nothing)
        for k in (5, 6):
            a = list(good)
            a[k] = 0
            assert f(*a) == 0, (name, k)


# ---------------------------------------------------------------- 4. the dispatch table
def test_paths_table():
    assert GP.path(64, 64) == 'wreg'
    assert GP.path(4, 64) == 'mfma1' and GP.path(68, 64) == 'mfma1'
    assert GP.path(64, 128) == 'mfma2' and GP.path(132, 128) == 'mfma2'
    assert GP.path(6, 64) == 'generic' and GP.path(64, 96) == 'generic' and GP.path(64, 192) == 'generic'
    for name, (shapes, Bs, Ls) in GP.table().items():
        for din, h in shapes:
            assert GP.on_path(name, din, h), (name, din, h)
            assert GP.fwd_lds_bytes(din, h) <= GP.LDS_DEFAULT
    assert GP.bwd_lds_bytes(8192, 'generic') == GP.LDS_LIMIT
