"""numpy restatement of the fp32 message-passing base ops - gather, scatter_add / _max / _mean,
gather_scatter, gather_segment_reduce (include/euler_gpu.h) - and of their gradients, independent
of the package: nothing here imports euler_amd.

Forward: a Python loop over the updates of a destination in input order, every sum rounded to
float32 on its own.  Gradients: the definitions of tf_euler/python/euler_ops/mp_ops.py:39-79
written out in float64.  An update whose key lies outside [0, size) belongs to no destination: it
is left out of the output and contributes 0 to every gradient."""
import numpy as np

INIT = {"add": 0.0, "mean": 0.0, "max": -1e9}


def valid_keys(keys, size):
    keys = np.asarray(keys)
    return (keys >= 0) & (keys < size)


def mean_denominator(lengths):
    """fl(float32(len) + float32(1e-7)), the float32 the mean divides by"""
    return (np.asarray(lengths).astype(np.float32) + np.float32(1e-7)).astype(np.float32)


def reduce_rows(op, rows, d):
    """One destination: rows [m, d] float32, its updates in input order.  -> [d] float32"""
    acc = np.full(d, INIT[op], np.float32)
    for v in rows:
        if op == "max":
            acc = np.where(v > acc, v, acc)
        else:
            acc = (acc + v).astype(np.float32)
    if op == "mean":
        acc = (acc / mean_denominator(len(rows))).astype(np.float32)
    return acc


def segments(keys, size):
    """positions of the updates of every destination, in input order: a list of `size` arrays"""
    keys = np.asarray(keys)
    order = np.argsort(keys, kind="stable")
    lo = np.searchsorted(keys[order], np.arange(size), "left")
    hi = np.searchsorted(keys[order], np.arange(size), "right")
    return [order[lo[r]:hi[r]] for r in range(size)]


def scatter_ref(op, x, keys, size):
    """scatter_(op, x, keys, size) for op add / max / mean"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty((size, x.shape[1]), np.float32)
    for r, pos in enumerate(segments(keys, size)):
        out[r] = reduce_rows(op, x[pos], x.shape[1])
    return out


def gather_ref(params, idx):
    return np.ascontiguousarray(np.asarray(params)[np.asarray(idx)])


def gather_scatter_ref(op, params, gi, keys, size):
    return scatter_ref(op, gather_ref(params, gi), keys, size)


def segment_keys(size, seg_ptr=None, count=None):
    """the destination of every update of a segmented block"""
    if seg_ptr is None:
        return np.repeat(np.arange(size), count)
    return np.repeat(np.arange(size), np.diff(np.asarray(seg_ptr)))


def id_rows(ids, rows):
    """the table row an int64 id reads: its low 32-bit word, unsigned, capped at the last row"""
    low = np.asarray(ids, np.int64) & 0xFFFFFFFF
    return np.minimum(low, rows - 1).astype(np.int64)


# ---- gradients -------------------------------------------------------------------------------
def _rows_by_key(t, keys):
    """t[keys[p]] per update, 0 for an update that belongs to no destination; dtype of t"""
    keys = np.asarray(keys)
    ok = valid_keys(keys, t.shape[0])
    out = np.zeros((len(keys), t.shape[1]), t.dtype)
    out[ok] = t[keys[ok]]
    return out


def scatter_add_grad(g, keys):
    """gx[p] = g[k[p]]: a copy, so the dtype (and the bits) of g are kept"""
    return _rows_by_key(np.asarray(g), keys)


def gather_grad(g, idx, rows):
    """gparams[n] = the sum of g[p] over idx[p] == n: a scatter_add, so float32 in input order"""
    return scatter_ref("add", g, idx, rows)


def scatter_mean_grad(g, keys, size):
    """gx[p] = g[k[p]] / fl(cnt + 1e-7), float64 with the float32 denominator taken exactly"""
    keys = np.asarray(keys)
    cnt = np.bincount(keys[valid_keys(keys, size)], minlength=size)
    denom = mean_denominator(cnt).astype(np.float64)
    return _rows_by_key(np.asarray(g, np.float64) / denom[:, None], keys)


def max_selected(x, keys, size):
    """(is_max [E, d] bool, n_max [E, d]: the number of equal maxima of the update's destination and
    column - 1 where the update is not a maximum, so that it divides)"""
    x = np.asarray(x, np.float64)
    keys = np.asarray(keys)
    ok = valid_keys(keys, size)
    top = np.full((size, x.shape[1]), INIT["max"], np.float64)
    np.maximum.at(top, keys[ok], x[ok])
    is_max = np.zeros(x.shape, bool)
    is_max[ok] = x[ok] == top[keys[ok]]
    n_dst = np.zeros((size, x.shape[1]), np.int64)
    np.add.at(n_dst, keys[ok], is_max[ok].astype(np.int64))
    n_max = np.ones(x.shape, np.int64)
    n_max[ok] = n_dst[keys[ok]]
    n_max[~is_max] = 1
    return is_max, n_max


def scatter_max_grad(x, g, keys, size):
    """gx[p, c] = [x[p, c] == max] / (number of equal maxima) * g[k[p], c], float64"""
    is_max, n_max = max_selected(x, keys, size)
    return is_max / n_max.astype(np.float64) * _rows_by_key(np.asarray(g, np.float64), keys)


def edge_terms(op, x_edges, g, keys, size):
    """the gradient of scatter_(op, x_edges, keys, size) per update, float64"""
    if op == "add":
        return scatter_add_grad(np.asarray(g, np.float64), keys)
    if op == "mean":
        return scatter_mean_grad(g, keys, size)
    return scatter_max_grad(x_edges, g, keys, size)


def gather_scatter_grad(op, params, gi, g, keys, size):
    """gradient of scatter_(op, params[gi], keys, size) with respect to params.  -> (want [rows, d]
    float64: the per-edge terms summed per table row; mag: the sum of their magnitudes; m [rows]:
    the number of edges that read the row)"""
    params = np.asarray(params)
    gi = np.asarray(gi)
    t = edge_terms(op, params[gi], g, keys, size)
    want = np.zeros(params.shape, np.float64)
    mag = np.zeros(params.shape, np.float64)
    np.add.at(want, gi, t)
    np.add.at(mag, gi, np.abs(t))
    return want, mag, np.bincount(gi, minlength=params.shape[0])
