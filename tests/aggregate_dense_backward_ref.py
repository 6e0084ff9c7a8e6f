"""aggregate_dense in float64 torch on the CPU, for autograd: the formulas of csrc/mp_dense.h over any seg_ptr."""
import torch


def composed64(op, comb, scale, act, seg, table, w, b, root, ws, gi, masks=None, a_pad=0.0):
    """seg: int64 [size + 1] from 0; gi: int64 [e]; masks: fixed 0/1 masks in place of the activation (for
    magnitudes); a_pad: added to every element of A (the absolute part of a narrowing's error) -> (out, [Zn, Zs])"""
    size, lens = len(seg) - 1, seg[1:] - seg[:-1]
    dst = torch.repeat_interleave(torch.arange(size), lens)
    ok = (gi >= 0) & (gi < table.shape[0])
    x = table[torch.where(ok, gi, torch.zeros_like(gi))] * ok[:, None]
    a = torch.zeros((size, table.shape[1]), dtype=torch.float64).index_add(0, dst, x)
    n = lens.double()
    if comb == "fold":
        a, n = a + (1.0 if scale is None else scale) * root, n + 1
    if op == "mean":
        a = a / n.clamp(min=1)[:, None]
    zs = [(a + a_pad) @ w + (0.0 if b is None else b)] + ([root @ ws] if comb in ("add", "concat") else [])
    if masks is None:
        masks = [(z > 0).double() if act == "relu" else torch.ones_like(z) for z in zs]
    hs = [z * m for z, m in zip(zs, masks)]
    out = hs[0] if len(hs) == 1 else hs[0] + hs[1] if comb == "add" else torch.cat([hs[1], hs[0]], 1)
    return out, zs
