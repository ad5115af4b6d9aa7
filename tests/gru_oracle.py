"""numpy forward and BPTT of the GRU cell of csrc/gru.hip (TF 1.0 tf.contrib.rnn.GRUCell, zero initial state, all L
steps run) -- the float64 twin the GRU tests compare with.  Every function keeps the dtype of its inputs, so the same
code on float32 arrays is the plain f32 restatement whose distance from float64 is the tests' error yardstick.

    [r | u] = sigmoid([x_t, h_{t-1}] . Wg + bg)        Wg [din+h, 2h], bg [2h]; columns: r first, then u
    c       = tanh([x_t, r * h_{t-1}] . Wc + bc)       Wc [din+h, h],  bc [h]
    h_t     = u * h_{t-1} + (1 - u) * c

Plain helpers, no fixtures; nothing here is imported by the package."""
import numpy as np


def _sigmoid(z):
    one = z.dtype.type(1)
    return one / (one + np.exp(-z))


def gru_fwd(x, Wg, bg, Wc, bc):
    """x [L, B, din] -> hs [L, B, h], gates [L, B, 3h] (r, u, c post-activation), rh [L, B, h] = r * h_{t-1}."""
    L, B, din = x.shape
    h = Wc.shape[1]
    dt = x.dtype
    one = dt.type(1)
    hs = np.zeros((L, B, h), dt)
    gates = np.zeros((L, B, 3 * h), dt)
    rh = np.zeros((L, B, h), dt)
    hp = np.zeros((B, h), dt)
    for t in range(L):
        g = _sigmoid(np.concatenate([x[t], hp], axis=1) @ Wg + bg)
        r, u = g[:, :h], g[:, h:]
        rhp = r * hp
        c = np.tanh(np.concatenate([x[t], rhp], axis=1) @ Wc + bc)
        hp = u * hp + (one - u) * c
        hs[t], rh[t] = hp, rhp
        gates[t, :, :h], gates[t, :, h:2 * h], gates[t, :, 2 * h:] = r, u, c
    return hs, gates, rh


def gru_bwd(x, Wg, Wc, hs, gates, dhs):
    """BPTT from the saved hs and gates, given dhs [L, B, h] (the gradient of every output).
    -> dzg [L, B, 2h] (dzr, dzu), dzc [L, B, h], dx [L, B, din], dWg, dbg, dWc, dbc."""
    L, B, din = x.shape
    h = Wc.shape[1]
    dt = x.dtype
    one = dt.type(1)
    dzg = np.zeros((L, B, 2 * h), dt)
    dzc = np.zeros((L, B, h), dt)
    dx = np.zeros((L, B, din), dt)
    dWg, dWc = np.zeros_like(Wg), np.zeros_like(Wc)
    dbg, dbc = np.zeros(2 * h, dt), np.zeros(h, dt)
    dh_rec = np.zeros((B, h), dt)
    for t in range(L - 1, -1, -1):
        r, u, c = gates[t, :, :h], gates[t, :, h:2 * h], gates[t, :, 2 * h:]
        hp = hs[t - 1] if t > 0 else np.zeros((B, h), dt)
        dh = dhs[t] + dh_rec
        du = dh * (hp - c)
        dc = dh * (one - u)
        zc = dc * (one - c * c)
        q = zc @ Wc[din:].T
        dr = q * hp
        zr = dr * r * (one - r)
        zu = du * u * (one - u)
        zg = np.concatenate([zr, zu], axis=1)
        dh_rec = dh * u + q * r + zg @ Wg[din:].T
        dzg[t], dzc[t] = zg, zc
        dx[t] = zg @ Wg[:din].T + zc @ Wc[:din].T
        dWg += np.concatenate([x[t], hp], axis=1).T @ zg
        dWc += np.concatenate([x[t], r * hp], axis=1).T @ zc
        dbg += zg.sum(axis=0)
        dbc += zc.sum(axis=0)
    return dzg, dzc, dx, dWg, dbg, dWc, dbc
