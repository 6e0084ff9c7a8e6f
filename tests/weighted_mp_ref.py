"""numpy restatement of the edge-weighted reduces (include/euler_gpu.h: euler_gpu_gather_scatter_w
and its siblings), independent of the kernels: a Python loop over a segment's updates in input
order, every product and every sum rounded to float32 on its own."""
import numpy as np

INIT = {"add": 0.0, "mean": 0.0, "max": -1e9}


def reduce_segment(op, x, w, rows, positions):
    """One destination: x [n, d] float32, w [E, H] float32, rows[k] / positions[k] = the table row
    and the weight row of its k-th update (input order).  -> [d] float32"""
    d = x.shape[1]
    dh = d // w.shape[1]
    acc = np.full(d, INIT[op], np.float32)
    for row, pos in zip(rows, positions):
        m = (x[row] * np.repeat(w[pos], dh)).astype(np.float32)      # fl(x * w), per column
        if op == "max":
            acc = np.where(m > acc, m, acc)
        else:
            acc = (acc + m).astype(np.float32)                       # fl(acc + fl(x * w))
    if op == "mean":
        acc = (acc / np.float32(np.float32(len(rows)) + np.float32(1e-7))).astype(np.float32)
    return acc


def gather_scatter_ref(op, x, gather, dst, size, w):
    """scatter_(op, x[gather] * w_expanded, dst, size); gather None: update p is row p.  Updates of
    a destination are taken in input order; dst >= size is left out."""
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32).reshape(len(dst), -1)
    out = np.empty((size, x.shape[1]), np.float32)
    dst = np.asarray(dst)
    order = np.argsort(dst, kind="stable")
    lo = np.searchsorted(dst[order], np.arange(size), "left")
    hi = np.searchsorted(dst[order], np.arange(size), "right")
    for r in range(size):
        pos = order[lo[r]:hi[r]]
        rows = pos if gather is None else np.asarray(gather)[pos]
        out[r] = reduce_segment(op, x, w, rows, pos)
    return out


def segment_dst(size, seg_ptr=None, count=None):
    if seg_ptr is None:
        return np.repeat(np.arange(size), count)
    return np.repeat(np.arange(size), np.diff(np.asarray(seg_ptr)))
