"""numpy restatement of the GCN-normalised aggregation (include/euler_gpu.h: euler_gpu_gcn_norm and
euler_gpu_gather_reduce_norm_t), independent of the kernels: degrees by np.bincount over the counted
edges, norm = float32(1) / sqrt(float32(deg)) (0 at degree 0), a Python loop over a segment's
updates in input order with every product and every sum rounded to float32 on its own, and the
root epilogue."""
import numpy as np

f32 = np.float32


def degrees(dst, src, n_dst, n_src):
    """an edge counts iff both keys are in range"""
    dst, src = np.asarray(dst, np.int64), np.asarray(src, np.int64)
    ok = (dst >= 0) & (dst < n_dst) & (src >= 0) & (src < n_src)
    return (np.bincount(dst[ok], minlength=n_dst).astype(np.int64),
            np.bincount(src[ok], minlength=n_src).astype(np.int64))


def norm_of(deg):
    deg = np.asarray(deg)
    out = np.zeros(deg.shape, f32)
    nz = deg > 0
    out[nz] = f32(1) / np.sqrt(deg[nz].astype(f32))          # two correctly rounded fp32 operations
    return out


def gcn_norm(dst, src, n_dst, n_src):
    dd, ds = degrees(dst, src, n_dst, n_src)
    return norm_of(dd), norm_of(ds)


def reduce_segment(op, x, rows, nd, norm_src):
    """One destination with norm nd: x [n, d] float32, rows = the gather indices of its updates in
    input order (one outside [0, n) contributes nothing).  -> [d] float32"""
    acc = np.zeros(x.shape[1], f32)
    for g in rows:
        if 0 <= g < x.shape[0]:
            w = f32(f32(nd) * norm_src[g])                    # fl(norm_i * norm_j)
            m = (x[g] * w).astype(f32)                        # fl(x * w), per column
            acc = (acc + m).astype(f32)                       # fl(acc + m)
    if op == "mean":
        acc = (acc / f32(f32(len(rows)) + f32(1e-7))).astype(f32)
    return acc


def epilogue(agg, root, a, b):
    """fl(fl(agg * a) + fl(root * b)) in float32"""
    return ((agg * f32(a)).astype(f32) + (np.asarray(root, f32) * f32(b)).astype(f32)).astype(f32)


def segments(dst, size):
    """positions of every destination's updates, input order kept; keys outside [0, size) left out"""
    dst = np.asarray(dst, np.int64)
    order = np.argsort(dst, kind="stable")
    lo = np.searchsorted(dst[order], np.arange(size), "left")
    hi = np.searchsorted(dst[order], np.arange(size), "right")
    return [order[lo[r]:hi[r]] for r in range(size)]


def gcn_aggregate(op, x, dst, src, n_dst, norm_dst, norm_src, root=None, a=1.0, b=1.0):
    """x float32 [n_src, d] (16-bit data widened by the caller) -> float32 [n_dst, d], before the
    rounding to a 16-bit out_dtype"""
    x = np.ascontiguousarray(x, f32)
    src = np.asarray(src, np.int64)
    out = np.empty((n_dst, x.shape[1]), f32)
    for r, pos in enumerate(segments(dst, n_dst)):
        out[r] = reduce_segment(op, x, src[pos], norm_dst[r], norm_src)
    if root is not None:
        out = epilogue(out, root, a, b)
    return out


def segment_dst(size, seg_ptr=None, count=None):
    if seg_ptr is None:
        return np.repeat(np.arange(size), count)
    return np.repeat(np.arange(size), np.diff(np.asarray(seg_ptr)))


def exact_f64(op, x, dst, src, n_dst, n_src):
    """(ref, scale) in float64 with exact integer degrees and w = 1 / sqrt(deg_i * deg_j):
    ref = the aggregate, scale[r] = sum_p |w_p x_p| per column (before a mean's division)"""
    dd, ds = degrees(dst, src, n_dst, n_src)
    x = np.asarray(x, np.float64)
    src = np.asarray(src, np.int64)
    ref = np.zeros((n_dst, x.shape[1]))
    scale = np.zeros_like(ref)
    lens = np.zeros(n_dst)
    for r, pos in enumerate(segments(dst, n_dst)):
        lens[r] = len(pos)
        for g in src[pos]:
            if 0 <= g < n_src:
                w = 1.0 / np.sqrt(float(dd[r]) * float(ds[g]))
                ref[r] += w * x[g]
                scale[r] += np.abs(w * x[g])
    if op == "mean":
        # the denominator is the contract's own fp32 number fl(length + 1e-7f), taken exactly
        den = (lens.astype(f32) + f32(1e-7)).astype(f32).astype(np.float64)[:, None]
        ref, scale = ref / den, scale / den
    return ref, scale, lens
