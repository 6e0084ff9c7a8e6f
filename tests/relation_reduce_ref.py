"""numpy restatement of the per-relation aggregation (include/euler_gpu.h:
euler_gpu_relation_reduce), independent of the kernels: a Python loop over the updates of one
bucket in input order, every sum rounded to float32 on its own."""
import numpy as np

OPS = ("add", "max", "mean", "mean_rel")
MODE = {"add": 0, "max": 1, "mean": 2, "mean_rel": 3}
EMPTY = {"add": 0.0, "max": -1e9, "mean": 0.0, "mean_rel": 0.0}


def reduce_dest(op, x, rows, types, num_relations):
    """One destination: x [n, d] float32; rows[k] / types[k] = the table row and the relation of
    its k-th update (input order).  -> (out [R, d] float32, counts [R] int32)"""
    d = x.shape[1]
    out = np.empty((num_relations, d), np.float32)
    cnt = np.zeros(num_relations, np.int32)
    n_valid = sum(1 for t in types if 0 <= t < num_relations)
    for t in range(num_relations):
        acc = np.full(d, EMPTY["max"] if op == "max" else 0.0, np.float32)
        for row, ty in zip(rows, types):
            if ty != t:
                continue
            cnt[t] += 1
            v = x[row].astype(np.float32)
            acc = np.where(v > acc, v, acc) if op == "max" else (acc + v).astype(np.float32)
        if op == "mean":
            acc = (acc / np.float32(np.float32(n_valid) + np.float32(1e-7))).astype(np.float32)
        elif op == "mean_rel":
            acc = (acc / np.float32(np.float32(cnt[t]) + np.float32(1e-7))).astype(np.float32)
        out[t] = acc
    return out, cnt


def relation_reduce_ref(op, x, gather, types, num_relations, dst, size):
    """The whole op: update p reads row gather[p] (None: row p), has relation types[p] and the
    destination dst[p]; destinations outside [0, size) and relations outside [0, R) are left out.
    -> (out [size, R, d] float32, counts [size, R] int32)"""
    x = np.asarray(x, np.float32)
    dst, types = np.asarray(dst), np.asarray(types)
    out = np.empty((size, num_relations, x.shape[1]), np.float32)
    counts = np.empty((size, num_relations), np.int32)
    order = np.argsort(dst, kind="stable")
    lo = np.searchsorted(dst[order], np.arange(size), "left")
    hi = np.searchsorted(dst[order], np.arange(size), "right")
    for r in range(size):
        pos = order[lo[r]:hi[r]]
        rows = pos if gather is None else np.asarray(gather)[pos]
        out[r], counts[r] = reduce_dest(op, x, rows, types[pos], num_relations)
    return out, counts


def segment_dst(size, seg_ptr=None, count=None):
    if seg_ptr is None:
        return np.repeat(np.arange(size), count)
    return np.repeat(np.arange(size), np.diff(np.asarray(seg_ptr)))
