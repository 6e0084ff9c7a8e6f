"""float64 statement of ops.aggregate_dense (csrc/mp_dense.h) on numpy arrays that hold the stored values.
The one narrowing of the aggregate goes through torch's CPU conversion (dt None: none, for magnitudes)."""
import numpy as np
import torch


def dense_ref(op, table, w, gi, seg, b, act, dt, root=None, ws=None, combine=None, scale=None):
    seg = np.asarray(seg, dtype=np.int64)
    lens, rows = np.diff(seg), table.shape[0]
    a = np.zeros((len(lens), table.shape[1]))
    n = lens.astype(np.float64)
    if combine == "fold":                       # the root row is the first term of the reduce
        a = a + root * (1.0 if scale is None else float(np.float32(scale)))
        n = n + 1
    for j in range(int(lens.max()) if len(lens) else 0):
        live = np.nonzero(j < lens)[0]
        p = seg[live] + j
        g = p if gi is None else gi[p].astype(np.int64)
        ok = (g >= 0) & (g < rows)              # an index outside the table: a row of +0 that still counts
        a[live[ok]] += table[g[ok]]
    if op == "mean":
        a = a / np.maximum(n, 1)[:, None]
    if dt is not None:
        a = torch.as_tensor(a).to(dt).double().numpy()
    f_act = (lambda z: np.where(z > 0, z, 0.0)) if act == "relu" else (lambda z: z)
    out = f_act(a @ w + (0.0 if b is None else b))
    if combine in ("add", "concat"):
        s = f_act(root @ ws)
        out = out + s if combine == "add" else np.concatenate([s, out], 1)
    return out
