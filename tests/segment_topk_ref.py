"""The per-column top-k over the gathered rows of a segment (euler_amd/csrc/mp_topk.h) restated in
numpy: the stable descending sort of every column of a segment, NaN greatest - what the
reference's LGCEncoder computes with transpose / tf.nn.top_k / transpose
(tf_euler/python/utils/encoders.py:911-914).  This is the reference of the host check and of the
GPU tests; a top-k is a pure selection, so every comparison with it is bit equality (a NaN must be
a NaN: the narrowing may quiet its payload).

A table / out array is float32, or uint16 holding the bits of bf16 / fp16; `dt` names which."""
import numpy as np

from embed_store_ref import DTYPES, narrow, widen, zeros  # noqa: F401

NP = {"f32": np.float32, "bf16": np.uint16, "f16": np.uint16}
QNAN = {"f32": 0x7fc00000, "bf16": 0x7fc0, "f16": 0x7e00}


def segments(size, e, seg_ptr=None, count=None):
    """[(begin, end)] of every destination, kept inside [0, e]"""
    if seg_ptr is None:
        return [(r * count, (r + 1) * count) for r in range(size)]
    out = []
    for r in range(size):
        b = min(max(int(seg_ptr[r]), 0), e)
        out.append((b, min(max(int(seg_ptr[r + 1]), b), e)))
    return out


def candidates(params, dt, gather, e):
    """-> the [e, d] block of candidate rows as stored (a row of +0 where the index names no row)
    and the bool [e] of the positions whose index names a row"""
    rows = params.shape[0]
    g = np.arange(e, dtype=np.int64) if gather is None else np.asarray(gather).astype(np.int64)
    live = (g >= 0) & (g < rows)
    block = zeros((e, params.shape[1]), dt)
    block[live] = params[g[live]]
    return block, live


def topk(params, dt, gather, size, k, seg_ptr=None, count=None, fill=0.0, out_dt=None, e=None):
    """-> (out [size, k, d] stored as out_dt, sel [size, k, d] int32)"""
    out_dt = out_dt or dt
    if e is None:
        e = len(gather) if gather is not None else (size * count if seg_ptr is None else params.shape[0])
    d = params.shape[1]
    block, _ = candidates(params, dt, gather, e)
    wide = widen(block, dt)
    out = np.empty((size, k, d), NP[out_dt])
    out[:] = narrow(np.float32(fill), out_dt)
    sel = np.full((size, k, d), -1, np.int32)
    for r, (b, en) in enumerate(segments(size, e, seg_ptr, count)):
        v = wide[b:en]
        nan = np.isnan(v)
        # stable; primary key: NaN first, secondary: descending value (+0 == -0)
        order = np.lexsort((-np.where(nan, np.float32(0), v), ~nan), axis=0)[:k]
        n = order.shape[0]
        sel[r, :n] = order + b
        picked = np.take_along_axis(block[b:en], order, axis=0)
        out[r, :n] = picked if out_dt == dt else widen(picked, dt)
    return out, sel


def per_edge(grad, sel, e):
    """-> [e, d] float32: grad at the selected positions, +0 elsewhere"""
    size, k, d = sel.shape
    pe = np.zeros((e, d), np.float32)
    r, j, c = np.nonzero(sel >= 0)
    pe[sel[r, j, c], c] = np.asarray(grad, np.float32)[r, j, c]
    return pe


def table_grad(pe, gather, rows):
    """-> [rows, d] float32: the per-edge block added in input order at the indices that name a row"""
    g = np.arange(pe.shape[0], dtype=np.int64) if gather is None else np.asarray(gather).astype(np.int64)
    out = np.zeros((rows, pe.shape[1]), np.float32)
    for p in range(pe.shape[0]):
        if 0 <= g[p] < rows:
            out[g[p]] = (out[g[p]] + pe[p]).astype(np.float32)
    return out


def same(a, b, dt):
    """bit equality of two stored arrays, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(widen(a, dt)), np.isnan(widen(b, dt))
    v = np.uint32 if a.dtype == np.float32 else np.uint16
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(v)[~na], b.view(v)[~nb]))


# ---- the inputs the host check and the GPU tests share ------------------------------------------
def tie_pool(rng, dt):
    """at most 6 distinct stored values: +-0, +-inf, NaN and a denormal among them (drawn 6 of 8)"""
    pool = {"f32": [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x00000001, 0x40200000, 0xbf800000],
            "bf16": [0x0000, 0x8000, 0x7f80, 0xff80, 0x7fc0, 0x0001, 0x4020, 0xbf80],
            "f16": [0x0000, 0x8000, 0x7c00, 0xfc00, 0x7e00, 0x0001, 0x4100, 0xbc00]}[dt]
    keep = [0, 1, 4, 5] + list(rng.permutation([2, 3, 6, 7])[:2])
    return np.array([pool[i] for i in keep], np.uint32 if dt == "f32" else np.uint16)


def tie_table(rng, shape, dt):
    """a table drawn from tie_pool: nearly every column of a segment has ties"""
    bits = tie_pool(rng, dt)[rng.integers(0, 6, shape)]
    return bits.view(np.float32) if dt == "f32" else bits


def ragged_ptr(rng, size, max_len=40, lead=3, empty_every=4):
    """seg_ptr [size + 1] with lengths 0..max_len, every empty_every-th segment empty and
    seg_ptr[0] = lead > 0; the caller makes e larger than seg_ptr[-1]"""
    lens = rng.integers(0, max_len + 1, size)
    lens[::empty_every] = 0
    if size > 1:
        lens[1] = max_len
    ptr = np.zeros(size + 1, np.int64)
    ptr[0] = lead
    ptr[1:] = lead + np.cumsum(lens)
    return ptr
