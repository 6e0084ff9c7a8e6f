"""float64 statement of ops.aggregate_gru (csrc/mp_gru.h) on numpy arrays that hold the stored values.  The
narrowings of m and of r * h go through torch's CPU conversion (dt None: none)."""
import numpy as np
import torch


def narrow(a, dt):
    return a if dt is None else torch.as_tensor(a).to(dt).double().numpy()


def segment_sum(op, table, gi, seg):
    seg = np.asarray(seg, dtype=np.int64)
    lens, rows = np.diff(seg), table.shape[0]
    m = np.zeros((len(lens), table.shape[1]))
    for j in range(int(lens.max()) if len(lens) else 0):
        live = np.nonzero(j < lens)[0]
        p = seg[live] + j
        g = p if gi is None else gi[p].astype(np.int64)
        ok = (g >= 0) & (g < rows)              # an index outside the table: a row of +0 that still counts
        m[live[ok]] += table[g[ok]]
    return m / np.maximum(lens, 1)[:, None] if op == "mean" else m


def gru_ref(op, table, gi, seg, state, wg, wc, bg, bc, dt):
    """-> (out, parts): parts holds m, the pre-activations and r, u, c, for the bound of the tests"""
    u_dim = state.shape[1]
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    m = narrow(segment_sum(op, table, gi, seg), dt)
    zg = np.concatenate([m, state], 1) @ wg + (0.0 if bg is None else bg)
    r, u = sig(zg[:, :u_dim]), sig(zg[:, u_dim:])
    rh = narrow(r * state, dt)
    c = np.tanh(np.concatenate([m, rh], 1) @ wc + (0.0 if bc is None else bc))
    return u * state + (1.0 - u) * c, dict(m=m, r=r, u=u, c=c, rh=rh)
