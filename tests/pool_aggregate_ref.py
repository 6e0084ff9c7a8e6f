"""Plain float64 reference of euler_amd.ops.pool_aggregate (csrc/mp_pool.h): gather with the
zero-row rule, matmul, bias, activation, then a per-segment reduce in numpy."""
import numpy as np


def pool_ref(op, table, weight, gi, seg, bias=None, act="relu"):
    """table [rows, d], weight [d, F], bias [F] | None: float64 arrays of the stored values;
    gi: integer array [e] | None (position p reads row p); seg: the size + 1 segment boundaries"""
    rows = table.shape[0]
    g = np.arange(seg[-1], dtype=np.int64) if gi is None else np.asarray(gi, dtype=np.int64)
    ok = (g >= 0) & (g < rows)
    x = np.where(ok[:, None], table[np.where(ok, g, 0)], 0.0)
    h = x @ weight + (0.0 if bias is None else bias)
    if act == "relu":
        h = np.maximum(h, 0.0)
    out = np.zeros((len(seg) - 1, weight.shape[1]))
    for r in range(len(seg) - 1):
        t = h[seg[r]:seg[r + 1]]
        if len(t):
            out[r] = t.max(0) if op == "max" else t.sum(0) if op == "add" else t.mean(0)
    return out
