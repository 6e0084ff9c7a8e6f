"""Graph-independent device operators of libeuler_gpu.so on torch tensors:
message passing (MPGather / MPScatterAdd / MPScatterMax), GenPair, the GQL
helper ops (ID_UNIQUE / IDX_GATHER / DATA_GATHER) and the shard split/merge
ops.  All tensors must live on a CUDA (ROCm) device; nothing here has a CPU
path."""
import contextlib
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, lib


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """The current HIP stream of the current device as a pointer (torch.cuda.current_stream()
    builds a Stream object for it: 8 us a call, a quarter of a small op's enqueue cost)."""
    if _RAW_STREAM is not None:
        return C.c_void_p(_RAW_STREAM(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_NULL_CTX = contextlib.nullcontext()


def _on(device):
    """Context of `device`; nothing to switch (5 us less per op) when it is the current one."""
    if device.index is None or torch.cuda.current_device() == device.index:
        return _NULL_CTX
    return torch.cuda.device(device)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _need_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("euler_amd ops need tensors in GPU memory "
                               "(no CPU fallback)")


_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}
_F32 = torch.float32


def _dt(name, t):
    """dtype code of a data tensor; anything but fp32 / bf16 / fp16 is an error, never a
    reinterpretation of its bytes"""
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError("%s: data must be float32, bfloat16 or float16, not %s" % (name, t.dtype))


def _out_dt(name, t, out_dtype):
    """out_dtype None = the input's dtype; else fp32 or the input's dtype"""
    if out_dtype is None or out_dtype == t.dtype:
        return t.dtype
    if out_dtype != _F32:
        raise TypeError("%s: out_dtype is float32 or the input's dtype (%s), not %s"
                        % (name, t.dtype, out_dtype))
    return _F32


def _gather_raw(params, indices, out_dtype=None):
    code = _dt("gather", params)
    od = _out_dt("gather", params, out_dtype)
    params = params.contiguous()
    indices = indices.to(torch.int32).contiguous()
    _need_cuda(params, indices)
    e, d = indices.numel(), params.shape[1]
    out = torch.empty((e, d), dtype=od, device=params.device)
    with _on(params.device):
        check(lib().euler_gpu_gather_t(_stream(), _ptr(params), code, _ptr(indices), e, d,
                                       params.shape[0], _ptr(out), _DT[od]))
    return out


def _scatter_raw(mode, updates, indices, size, out_dtype=None):
    """mode: 0 add, 1 max, 2 mean"""
    code = _dt("scatter", updates)
    od = _out_dt("scatter", updates, out_dtype)
    updates = updates.contiguous()
    indices = indices.to(torch.int32).contiguous()
    _need_cuda(updates, indices)
    e, d = updates.shape
    out = torch.empty((int(size), d), dtype=od, device=updates.device)
    with _on(updates.device):
        check(lib().euler_gpu_scatter_t(_stream(), mode, _ptr(updates), code, _ptr(indices), e, d,
                                        int(size), _ptr(out), _DT[od]))
    return out


_ADD, _MAX, _MEAN = 0, 1, 2


def _count(indices, size, device):
    """scatter_add(ones) + 1e-7, fp32: the denominator of the mean's gradient"""
    ones = torch.ones((indices.numel(), 1), dtype=_F32, device=device)
    return _scatter_raw(_ADD, ones, indices, size) + 1e-7


# An update whose scatter key lies outside [0, size) belongs to no destination: the reduces leave
# it out (mp_segments.h), so its gradient is exactly 0 and no backward pass may read a row of
# grad, out or a count with its key - `gather` trusts its indices.  The keys are made safe and the
# rows of such updates zeroed on the device, without a host wait; in-range updates keep their bits.
def _keys_in_range(si, size):
    """-> (valid [E, 1] bool, the keys as int32 with every key outside [0, size) replaced by 0)"""
    si = si.to(torch.int32)
    valid = (si >= 0) & (si < size)
    return valid.reshape(-1, 1), torch.where(valid, si, torch.zeros_like(si))


def _gather_by_key(t, si, out_dtype=None):
    """rows of t ([size, D]: grad, or grad / count) by scatter key; 0 where the key names no row"""
    size = t.shape[0]
    if size == 0:
        return torch.zeros((si.numel(), t.shape[1]), dtype=_out_dt("gather", t, out_dtype), device=t.device)
    valid, safe = _keys_in_range(si, size)
    return _gather_raw(t, safe, out_dtype).masked_fill_(~valid, 0)


def _max_per_edge(updates32, out, si, size, grad):
    """the per-edge gradient of a max reduce (mp_ops.py:39-62), all fp32"""
    if size == 0:
        return torch.zeros_like(updates32)
    valid, safe = _keys_in_range(si, size)
    indicators = (updates32 == _gather_raw(out, safe, _F32)).to(_F32)
    num_selected = _scatter_raw(_ADD, indicators, si, size)      # (leaves the same updates out)
    per_edge = indicators / _gather_raw(num_selected, safe) * _gather_raw(grad, safe, _F32)
    return per_edge.masked_fill_(~valid, 0)


# Gradients as registered in tf_euler/python/euler_ops/mp_ops.py:39-62.  With 16-bit data the
# formulas are the same and run in fp32: every intermediate of a backward pass is taken with
# out_dtype = fp32 (the widening is exact), and the gradient is rounded once, to the dtype of the
# input it belongs to.  `grad` may arrive as fp32 or in 16 bits.
class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, indices, out_dtype):
        ctx.save_for_backward(indices)
        ctx.n, ctx.dt = params.shape[0], params.dtype
        return _gather_raw(params, indices, out_dtype)

    @staticmethod
    def backward(ctx, grad):
        (indices,) = ctx.saved_tensors
        return _scatter_raw(_ADD, grad, indices, ctx.n, _F32).to(ctx.dt), None, None


class _ScatterAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, updates, indices, size, out_dtype):
        ctx.save_for_backward(indices)
        ctx.dt = updates.dtype
        return _scatter_raw(_ADD, updates, indices, size, out_dtype)

    @staticmethod
    def backward(ctx, grad):
        (indices,) = ctx.saved_tensors
        return _gather_by_key(grad, indices, _F32).to(ctx.dt), None, None, None


class _ScatterMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, updates, indices, size, out_dtype):
        out = _scatter_raw(_MAX, updates, indices, size, out_dtype)
        ctx.save_for_backward(updates, indices, out)
        ctx.size = size
        return out

    @staticmethod
    def backward(ctx, grad):
        updates, indices, out = ctx.saved_tensors
        per_edge = _max_per_edge(updates.to(_F32), out, indices, ctx.size, grad)
        return per_edge.to(updates.dtype), None, None, None


def gather(params, indices, out_dtype=None):
    """MPGather: out[i,:] = params[indices[i],:] (fp32, bf16 or fp16 rows, int32 indices).
    out_dtype: None = the dtype of params, or torch.float32 for 16-bit params (the rows widened,
    which is exact).  params may be an Fp8Rows table: the rows of its dequantize(), out_dtype None
    (fp32), float32, bfloat16 or float16; no gradient."""
    if isinstance(params, Fp8Rows):
        return _fp8_gather(params, indices, out_dtype)
    return _Gather.apply(params, indices, out_dtype)


def scatter_add(updates, indices, size, out_dtype=None):
    """MPScatterAdd: out[indices[i],:] += updates[i,:], zero init, [size,D].  16-bit updates are
    added in fp32, in input order - the bits of the fp32 op on updates.float() - and the sums
    are returned as fp32 (out_dtype=torch.float32) or rounded once to the updates' dtype
    (out_dtype=None).
    An update whose index is < 0 or >= size belongs to no destination: it is left out of `out`
    and its gradient is exactly 0.  The rule holds for every op with a scatter key column -
    scatter_add / scatter_max / scatter_mean and gather_scatter, with or without edge_weight (there
    for grad_edge_weight too) - as it does for edge_softmax; no backward pass reads a row of
    grad with such a key."""
    return _ScatterAdd.apply(updates, indices, int(size), out_dtype)


def scatter_max(updates, indices, size, out_dtype=None):
    """MPScatterMax: element-wise max per destination, -1e9 for empty rows (rounded to the
    output's dtype).  out_dtype as scatter_add."""
    return _ScatterMax.apply(updates, indices, int(size), out_dtype)


class _ScatterMean(torch.autograd.Function):
    """scatter_add(x) / (scatter_add(ones) + 1e-7) in one pass (euler_gpu_scatter_mean);
    the gradient of the composition: grad / (count + 1e-7) gathered back."""

    @staticmethod
    def forward(ctx, updates, indices, size, out_dtype):
        ctx.save_for_backward(indices)
        ctx.size, ctx.dt = size, updates.dtype
        return _scatter_raw(_MEAN, updates, indices, size, out_dtype)

    @staticmethod
    def backward(ctx, grad):
        (indices,) = ctx.saved_tensors
        count = _count(indices, ctx.size, grad.device)
        return _gather_by_key(grad / count, indices).to(ctx.dt), None, None, None


def scatter_mean(updates, indices, size, out_dtype=None):
    """mp_ops.py:65-69.  out_dtype as scatter_add."""
    if updates.shape[0] < (1 << 24):
        return _ScatterMean.apply(updates, indices, int(size), out_dtype)
    od = _out_dt("scatter_mean", updates, out_dtype)
    out = scatter_add(updates, indices, size, out_dtype=_F32)
    ep = 1e-7
    ones = torch.ones((updates.shape[0], 1), dtype=torch.float32,
                      device=updates.device)
    count = scatter_add(ones, indices, size) + ep
    return (out / count).to(od)


_GS_MODE = {"add": 0, "max": 1, "mean": 2}


def _check_rows(name, gi, n_rows):
    """opt-in (a device round trip): the kernels index params with these as they are"""
    if gi.numel() and (int(gi.min()) < 0 or int(gi.max()) >= n_rows):
        raise IndexError("%s: gather index out of range" % name)


def _gather_scatter_raw(mode, params, gather_indices, scatter_indices, size, validate=False,
                        out_dtype=None):
    code = _dt("gather_scatter", params)
    od = _out_dt("gather_scatter", params, out_dtype)
    params = params.contiguous()
    gi = gather_indices.to(torch.int32).contiguous()
    si = scatter_indices.to(torch.int32).contiguous()
    _need_cuda(params, gi)
    _need_cuda(params, si)
    if gi.numel() != si.numel():
        raise ValueError("gather_scatter: one gather index and one scatter index per edge")
    if validate:
        _check_rows("gather_scatter", gi, params.shape[0])
    e, d = gi.numel(), params.shape[1]
    out = torch.empty((int(size), d), dtype=od, device=params.device)
    with _on(params.device):
        check(lib().euler_gpu_gather_scatter_t(_stream(), mode, _ptr(params), code, _ptr(gi), _ptr(si),
                                               e, d, int(size), _ptr(out), _DT[od]))
    return out


def _edge_grad(op, params, gi, si, out, size, grad):
    """fp32 gradient of reduce(op, gather(params, gi), si, size) per edge (mp_ops.py:39-62)"""
    if op == "add":
        return _gather_by_key(grad, si, _F32)
    if op == "mean":
        return _gather_by_key(grad / _count(si, size, grad.device), si)
    return _max_per_edge(_gather_raw(params, gi, _F32), out, si, size, grad)


class _GatherScatter(torch.autograd.Function):
    """scatter_(op, gather(params, gi), si, size) in one pass (euler_gpu_gather_scatter);
    the gradient is the composition's: the scatter's gradient (mp_ops.py:39-62) per edge,
    scatter-added into the rows of params the edges read."""

    @staticmethod
    def forward(ctx, params, gather_indices, scatter_indices, size, op, validate, out_dtype):
        out = _gather_scatter_raw(_GS_MODE[op], params, gather_indices, scatter_indices, size,
                                  validate, out_dtype)
        ctx.save_for_backward(params, gather_indices, scatter_indices, out)
        ctx.size, ctx.op = size, op
        return out

    @staticmethod
    def backward(ctx, grad):
        params, gi, si, out = ctx.saved_tensors
        per_edge = _edge_grad(ctx.op, params, gi, si, out, ctx.size, grad)
        return (_scatter_raw(_ADD, per_edge, gi, params.shape[0]).to(params.dtype),
                None, None, None, None, None, None)


def gather_scatter(op, params, gather_indices, scatter_indices, size, validate=False, out_dtype=None,
                   edge_weight=None):
    """scatter_(op, gather(params, gather_indices), scatter_indices, size) for op in
    "add" / "max" / "mean" - the aggregation of a message-passing step whose message is
    the neighbour's row (SAGE mean / max, GCN after its normalisation) - without
    materialising the gathered [E, D] block: same bits, a third of the HBM traffic.
    Like `gather`, the kernel trusts the gather indices; validate=True checks them first
    (one device round trip).  out_dtype as scatter_add.
    edge_weight ([E], [E, 1] or [E, H] with H dividing D; fp32 or the dtype of params): the
    message is the row times its edge's weight - column c takes weight c // (D // H) - as in
    GCN / APPNP (norm_i * norm_j * x_j) and GAT / AGNN (x_j * alpha): the bits of
    scatter_(op, gather(params, gi) * w_expanded, si, size) with the multiply in fp32, still one
    pass.  Gradients flow to params and to edge_weight (the latter through `edge_dot`)."""
    if op not in _GS_MODE:
        raise ValueError("gather_scatter: op is add, max or mean")
    if edge_weight is not None:
        _edge_weight("gather_scatter", edge_weight, gather_indices.numel(), params)
        if op == "mean" and gather_indices.numel() >= (1 << 24):
            raise ValueError("gather_scatter: a weighted mean needs fewer than 2^24 edges")
        return _GatherScatterW.apply(params, gather_indices, scatter_indices, int(size), op, bool(validate),
                                     out_dtype, edge_weight)
    if op == "mean" and gather_indices.numel() >= (1 << 24):
        return scatter_mean(gather(params, gather_indices), scatter_indices, size, out_dtype=out_dtype)
    return _GatherScatter.apply(params, gather_indices, scatter_indices, int(size), op, bool(validate),
                                out_dtype)


def _segment_dst(seg_ptr, count, size, device):
    """destination of every update of a segmented block (for the gradient)"""
    if seg_ptr is None:
        return torch.arange(size, device=device, dtype=torch.int32).repeat_interleave(int(count))
    lens = (seg_ptr[1:] - seg_ptr[:-1]).to(torch.int64)
    return torch.repeat_interleave(torch.arange(size, device=device, dtype=torch.int32), lens)


def _segment_args(params, gather_indices, seg_ptr, count, size, validate):
    """the tensors of a segmented call -> (params, gi, as_ids, sp), contiguous and checked"""
    params = params.contiguous()
    # int64 ids (what the samplers return) are read in place: index = low word of the id,
    # the int32 a cast would give, without the cast's pass (euler_gpu_gather_segment_reduce_ids_t)
    as_ids = gather_indices.dtype == torch.int64 and not validate
    gi = gather_indices.contiguous() if as_ids else gather_indices.to(torch.int32).contiguous()
    _need_cuda(params, gi)
    sp = None
    if seg_ptr is not None:
        sp = seg_ptr.to(torch.int64).contiguous()
        _need_cuda(params, sp)
        if sp.numel() != size + 1:
            raise ValueError("gather_segment_reduce: seg_ptr has size + 1 entries")
    elif gi.numel() != size * count:
        raise ValueError("gather_segment_reduce: size * count gather indices")
    if validate:
        _check_rows("gather_segment_reduce", gi, params.shape[0])
    return params, gi, as_ids, sp


def _saved_rows(gi, n_rows):
    """int64 ids as the int32 rows the forward kernel read, for the gradient kernels: an id past the
    table - or a negative one, e.g. default_node = -1: unsigned there - reads the table's LAST row
    (euler_gpu.h: min((uint32) low word, rows - 1)), and the gradient must flow to that same row
    (the raw low word would be an out-of-range or negative scatter key)"""
    return torch.clamp(gi & 0xFFFFFFFF, max=n_rows - 1).to(torch.int32)


class _GatherSegmentReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, gather_indices, seg_ptr, count, size, op, validate, out_dtype):
        code = _dt("gather_segment_reduce", params)
        od = _out_dt("gather_segment_reduce", params, out_dtype)
        params, gi, as_ids, sp = _segment_args(params, gather_indices, seg_ptr, count, size, validate)
        rows, d = params.shape
        out = torch.empty((size, d), dtype=od, device=params.device)
        with _on(params.device):
            if as_ids:      # (ids past the table read its last row: euler_gpu.h)
                check(lib().euler_gpu_gather_segment_reduce_ids_t(
                    _stream(), _GS_MODE[op], _ptr(params), code, rows, _ptr(gi), _ptr(sp), count, d, size,
                    _ptr(out), _DT[od]))
            else:
                check(lib().euler_gpu_gather_segment_reduce_t(
                    _stream(), _GS_MODE[op], _ptr(params), code, _ptr(gi), _ptr(sp), count, d, size,
                    _ptr(out), _DT[od]))
        if as_ids and ctx.needs_input_grad[0]:
            gi = _saved_rows(gi, rows)
        ctx.save_for_backward(params, gi, sp if sp is not None else torch.empty(0), out)
        ctx.has_ptr, ctx.count, ctx.size, ctx.op = sp is not None, count, size, op
        return out

    @staticmethod
    def backward(ctx, grad):
        params, gi, sp, out = ctx.saved_tensors
        si = _segment_dst(sp if ctx.has_ptr else None, ctx.count, ctx.size, grad.device)
        per_edge = _edge_grad(ctx.op, params, gi, si, out, ctx.size, grad)
        return (_scatter_raw(_ADD, per_edge, gi, params.shape[0]).to(params.dtype),
                None, None, None, None, None, None, None)


def gather_segment_reduce(op, params, gather_indices, size, seg_ptr=None, count=None, validate=False,
                          out_dtype=None, edge_weight=None):
    """The aggregation of a sampled block: destination r reduces (op = "add" / "max" /
    "mean") the rows params[gather_indices[p]] for p in [seg_ptr[r], seg_ptr[r + 1]) - or
    its `count` consecutive indices when seg_ptr is None (SampleNeighbor's fixed fan-out)
    - in that order.  The bits of scatter_(op, gather(params, gather_indices), dst, size)
    with dst = the destination of every index, in one pass and without the scatter's
    look at its key column (no host wait; validate=True checks the gather indices first,
    which is one).  out_dtype as scatter_add.  edge_weight as gather_scatter - e.g. the weights
    sample_neighbor returns next to the ids.

    params may be an Fp8Rows table (the constant input features of a GNN, a quarter of their fp32
    bytes): the result has the bits of this op on params.dequantize(), out_dtype None (fp32),
    float32, bfloat16 or float16; edge_weight float32, bfloat16 or float16.  No gradient flows to
    an Fp8Rows, and an edge_weight that requires grad raises NotImplementedError there."""
    if isinstance(params, Fp8Rows):
        return _fp8_gather_segment_reduce(op, params, gather_indices, size, seg_ptr, count, validate,
                                          out_dtype, edge_weight)
    if op not in _GS_MODE:
        raise ValueError("gather_segment_reduce: op is add, max or mean")
    if (seg_ptr is None) == (count is None):
        raise ValueError("gather_segment_reduce: pass seg_ptr or count")
    if edge_weight is not None:
        _edge_weight("gather_segment_reduce", edge_weight, gather_indices.numel(), params)
        return _GatherSegmentReduceW.apply(params, gather_indices, seg_ptr, 0 if count is None else int(count),
                                           int(size), op, bool(validate), out_dtype, edge_weight)
    return _GatherSegmentReduce.apply(params, gather_indices, seg_ptr, 0 if count is None else int(count),
                                      int(size), op, bool(validate), out_dtype)


# ---- quantised (fp8) feature row tables --------------------------------------------------------
FP8_MAX = 448.0     # the largest finite e4m3fn value


def _fp8_out_dt(name, out_dtype):
    if out_dtype is None:
        return _F32
    if out_dtype not in _DT:
        raise TypeError("%s: out_dtype of an Fp8Rows op is float32, bfloat16 or float16, not %s"
                        % (name, out_dtype))
    return out_dtype


def column_absmax(x, out=None):
    """absmax[c] = the largest |x[r, c]| over the FINITE values of column c of x [n, d] (fp32, bf16
    or fp16; NaN and +-inf are skipped), as fp32 [d].  Exact.  With `out` (fp32 [d], non-negative):
    out = max(out, absmax(x)) in place, so that a table is scanned in chunks."""
    code = _dt("column_absmax", x)
    if x.dim() != 2:
        raise ValueError("column_absmax: x is [n, d]")
    x = x.contiguous()
    _need_cuda(x)
    n, d = x.shape
    if out is None:
        out = torch.zeros(d, dtype=_F32, device=x.device)
    elif out.dtype != _F32 or out.dim() != 1 or out.numel() != d or not out.is_contiguous() \
            or out.device != x.device:
        raise ValueError("column_absmax: out is a contiguous float32 [d] tensor on the device of x")
    with _on(x.device):
        check(lib().euler_gpu_column_absmax(_stream(), _ptr(x), code, n, d, _ptr(out)))
    return out


class Fp8Rows(object):
    """A quantised row table: q [N, d] uint8 codes of OCP e4m3fn (q.view(torch.float8_e4m3fn) is a
    view of the same bytes) and scale [d] fp32, finite and positive, one per column.  Its value is
    x^[r, c] = float32(q[r, c]) * scale[c] (one fp32 multiply); ops.gather and
    ops.gather_segment_reduce read it in place and return the bits of the fp32 op on
    dequantize().  Forward only: no gradient flows to a table."""

    def __init__(self, q, scale):
        if q.dtype == getattr(torch, "float8_e4m3fn", None):
            q = q.view(torch.uint8)
        if q.dtype != torch.uint8 or q.dim() != 2:
            raise TypeError("Fp8Rows: q is a [N, d] uint8 (or float8_e4m3fn) tensor")
        if scale.dtype != _F32 or scale.dim() != 1 or scale.numel() != q.shape[1]:
            raise TypeError("Fp8Rows: scale is a float32 [d] tensor")
        _need_cuda(q, scale)
        if q.device != scale.device:
            raise ValueError("Fp8Rows: q and scale live on different devices")
        self.q = q.contiguous()
        self.scale = scale.detach().contiguous()

    @property
    def shape(self):
        return self.q.shape

    @property
    def device(self):
        return self.q.device

    @staticmethod
    def scale_of(absmax):
        """the column scales of a column absmax: absmax / 448, and 1 where the column is all zero.
        The d divisions are done on the host (one wait, once per table): IEEE fp32, whatever a
        device library makes of a division by a constant."""
        a = absmax.detach().to(_F32).cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(a > 0, a / np.float32(FP8_MAX), np.float32(1)).astype(np.float32)
        return torch.from_numpy(s).to(absmax.device)

    @staticmethod
    def empty(n, d, scale, device=None):
        """an uninitialised table of n rows with the given column scales (fill it with store())"""
        device = scale.device if device is None else torch.device(device)
        scale = scale.to(device=device, dtype=_F32)
        return Fp8Rows(torch.empty((int(n), int(d)), dtype=torch.uint8, device=device), scale)

    def store(self, first_row, x):
        """quantises x [m, d] (fp32, bf16 or fp16) into rows [first_row, first_row + m) in place,
        with the table's scale: q = Enc(x / scale), an fp32 division, round to nearest even, values
        past the scale saturate at +-448"""
        code = _dt("Fp8Rows.store", x)
        first_row = int(first_row)
        if x.dim() != 2 or x.shape[1] != self.q.shape[1]:
            raise ValueError("Fp8Rows.store: x is [m, %d]" % self.q.shape[1])
        if first_row < 0 or first_row + x.shape[0] > self.q.shape[0]:
            raise IndexError("Fp8Rows.store: rows [%d, %d) are not inside the table's %d"
                             % (first_row, first_row + x.shape[0], self.q.shape[0]))
        x = x.detach().contiguous()
        _need_cuda(x)
        if x.device != self.q.device:
            raise ValueError("Fp8Rows.store: x lives on %s, the table on %s" % (x.device, self.q.device))
        m, d = x.shape
        with _on(self.q.device):
            check(lib().euler_gpu_fp8_quantize_rows(_stream(), _ptr(x), code, m, d, _ptr(self.scale),
                                                    _ptr(self.q[first_row:first_row + m])))
        return self

    @staticmethod
    def quantize(x, scale=None):
        """the table of x [N, d]; scale None: from x's own columns (absmax over the finite values /
        448, 1 for a column of zeros), else the caller's (e.g. one that clips outliers)"""
        if scale is None:
            scale = Fp8Rows.scale_of(column_absmax(x.detach()))
        return Fp8Rows.empty(x.shape[0], x.shape[1], scale, x.device).store(0, x)

    def dequantize(self, out_dtype=_F32):
        """x^ [N, d] in fp32 (exact), or rounded once to bf16 / fp16"""
        n = self.q.shape[0]
        if n >= 1 << 31:
            raise ValueError("Fp8Rows.dequantize: the table has 2^31 rows or more")
        return _fp8_gather(self, torch.arange(n, dtype=torch.int32, device=self.q.device), out_dtype)


def _fp8_gather(table, indices, out_dtype):
    od = _fp8_out_dt("gather", out_dtype)
    indices = indices.to(torch.int32).contiguous()
    _need_cuda(indices)
    e, d = indices.numel(), table.q.shape[1]
    out = torch.empty((e, d), dtype=od, device=table.q.device)
    with _on(table.q.device):
        check(lib().euler_gpu_fp8_gather(_stream(), _ptr(table.q), _ptr(table.scale), _ptr(indices), e, d,
                                         table.q.shape[0], _ptr(out), _DT[od]))
    return out


def _fp8_gather_segment_reduce(op, table, gather_indices, size, seg_ptr, count, validate, out_dtype,
                               edge_weight):
    if op not in _GS_MODE:
        raise ValueError("gather_segment_reduce: op is add, max or mean")
    if (seg_ptr is None) == (count is None):
        raise ValueError("gather_segment_reduce: pass seg_ptr or count")
    od = _fp8_out_dt("gather_segment_reduce", out_dtype)
    size, count = int(size), 0 if count is None else int(count)
    rows, d = table.q.shape
    w2, heads = None, 1
    if edge_weight is not None:
        if edge_weight.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("gather_segment_reduce: no gradient to edge_weight through an Fp8Rows "
                                      "table")
        if edge_weight.dtype not in _DT:
            raise TypeError("gather_segment_reduce: edge_weight is float32, bfloat16 or float16, not %s"
                            % edge_weight.dtype)
        w2, heads = _fp8_edge_weight(edge_weight.detach(), gather_indices.numel(), d)
    _, gi, as_ids, sp = _segment_args(table.q, gather_indices, seg_ptr, count, size, bool(validate))
    out = torch.empty((size, d), dtype=od, device=table.q.device)
    wd = _DT[w2.dtype] if w2 is not None else _lib.F32
    with _on(table.q.device):
        if as_ids:
            check(lib().euler_gpu_fp8_gather_segment_reduce_ids(
                _stream(), _GS_MODE[op], _ptr(table.q), _ptr(table.scale), rows, _ptr(gi), _ptr(sp), count, d,
                size, _ptr(out), _DT[od], _ptr(w2), wd, heads))
        else:
            check(lib().euler_gpu_fp8_gather_segment_reduce(
                _stream(), _GS_MODE[op], _ptr(table.q), _ptr(table.scale), _ptr(gi), _ptr(sp), count, d, size,
                _ptr(out), _DT[od], _ptr(w2), wd, heads))
    return out


def _fp8_edge_weight(w, e, d):
    """the shape rules of _edge_weight for a quantised table -> ([E, H] contiguous, H)"""
    name = "gather_segment_reduce"
    _need_cuda(w)
    if w.dim() not in (1, 2):
        raise ValueError("%s: edge_weight is [E], [E, 1] or [E, H]" % name)
    w2 = w.reshape(-1, 1) if w.dim() == 1 else w
    if w2.shape[0] != e:
        raise ValueError("%s: one weight row per edge (%d), not %d" % (name, e, w2.shape[0]))
    heads = int(w2.shape[1])
    if heads < 1 or d % heads != 0:
        raise ValueError("%s: the %d weights of an edge do not divide the %d columns" % (name, heads, d))
    return w2.contiguous(), heads


# ---- per-column top-k of a sampled block (LGCN: utils/encoders.py:872-922) --------------------
def _segment_topk_raw(params, gi, sp, count, e, size, k, fill, od, want_sel):
    """euler_gpu_gather_segment_topk on prepared tensors -> (out [size, k, d], sel [size, k, d] | None)"""
    d = params.shape[1]
    make = torch.zeros if size == 0 or d == 0 else torch.empty
    out = make((size, k, d), dtype=od, device=params.device)
    sel = make((size, k, d), dtype=torch.int32, device=params.device) if want_sel else None
    if size == 0 or d == 0:
        return out, sel
    with _on(params.device):
        check(lib().euler_gpu_gather_segment_topk(
            _stream(), _ptr(params), _DT[params.dtype], int(params.shape[0]), _ptr(gi),
            int(gi is not None and gi.dtype == torch.int64), _ptr(sp), int(count), e, d, size, k, float(fill),
            _ptr(out), _DT[od], _ptr(sel)))
    return out, sel


def _segment_topk_grad_raw(grad, sel, e):
    """euler_gpu_segment_topk_grad -> the fp32 per-edge block [e, d]: grad at the selected positions,
    +0 elsewhere"""
    size, k, d = sel.shape
    if e == 0 or d == 0:
        return torch.zeros((e, d), dtype=_F32, device=sel.device)
    if grad.dtype not in _DT:
        grad = grad.to(_F32)
    grad = grad.contiguous()
    per_edge = torch.empty((e, d), dtype=_F32, device=sel.device)
    with _on(sel.device):
        check(lib().euler_gpu_segment_topk_grad(_stream(), _ptr(grad), _DT[grad.dtype], _ptr(sel), e, d, size, k,
                                                _ptr(per_edge)))
    return per_edge


class _GatherSegmentTopk(torch.autograd.Function):
    """The fused top-k; the gradient is the composition's: grad lands on the selected positions
    (the helper kernel, one writer per element) and the existing scatter-add carries the per-edge
    block to the rows of params - in input order, indices that name no row left out."""

    @staticmethod
    def forward(ctx, params, gi, sp, count, e, size, k, fill, od, return_indices, need):
        out, sel = _segment_topk_raw(params, gi, sp, count, e, size, k, fill, od, need or return_indices)
        if need:
            ctx.save_for_backward(sel, gi if gi is not None else torch.empty(0))
            ctx.conf = (gi is not None, e, int(params.shape[0]), params.dtype)
        if not return_indices:
            return out, None
        ctx.mark_non_differentiable(sel)
        return out, sel

    @staticmethod
    def backward(ctx, grad, _unused=None):
        sel, gi = ctx.saved_tensors
        has_gi, e, rows, dt = ctx.conf
        if e == 0 or sel.shape[2] == 0:
            return (torch.zeros((rows, sel.shape[2]), dtype=dt, device=sel.device),) + (None,) * 10
        per_edge = _segment_topk_grad_raw(grad, sel, e)
        if not has_gi:      # position p is row p; scatter_add leaves out the positions past the table
            gi = torch.arange(e, device=sel.device, dtype=torch.int32)
        elif gi.dtype == torch.int64:
            gi = torch.where((gi >= 0) & (gi < rows), gi, torch.full_like(gi, -1))
        return (_scatter_raw(_ADD, per_edge, gi, rows).to(dt),) + (None,) * 10


def gather_segment_topk(params, gather_indices, size, k, seg_ptr=None, count=None, fill=0.0, out_dtype=None,
                        return_indices=False, validate=False):
    """The step of the reference's LGCEncoder (LGCN, utils/encoders.py:911-914: get_dense_feature,
    reshape [B, nb, d], transpose, tf.nn.top_k, transpose) in one pass: for destination r and
    EVERY COLUMN c on its own, the k largest values among params[gather_indices[p]][c] over the
    positions p of r's segment - [seg_ptr[r], seg_ptr[r + 1]) or its `count` consecutive positions,
    as gather_segment_reduce - in descending order.  Returns out [size, k, d] in the dtype of
    params (fp32, bf16 or fp16) or fp32 (out_dtype); with return_indices=True also sel
    [size, k, d] int32, the position p each entry came from.
    gather_indices: int32 indices, the int64 ids a sampler returned (read in place, compared in 64
    bits), or None (position p reads row p).  RANGE RULE: an index outside [0, rows) names no row;
    it is never dereferenced, reads as a row of +0 and does take part as a candidate - the zero
    feature row of a default_node fill enters the reference's top_k too - and gets no gradient.
    ORDER: larger first, NaN greatest (as torch.topk); among equals (+0 == -0, NaN == NaN) the
    earlier position first, so the result is the stable descending sort.  An entry j >= the
    segment's length is `fill` (rounded once to the output dtype) with sel = -1.  1 <= k <= 16.
    A pure selection: out carries the bits of the table's elements (a NaN stays a NaN), the same on
    every call, and equals torch.topk(gather(params, gi).view(B, nb, d), k, dim=1) wherever the
    values of a column are distinct - without the [E, d] block or the transposes.
    The gradient of params is the composition's: grad at the selected positions, scatter-added in
    input order and rounded once to the dtype of params.  sel is kept, and asked of the kernel,
    only when params needs a gradient or return_indices is set.  No host wait (validate=True
    checks the gather indices first, which is one)."""
    _dt("gather_segment_topk", params)
    od = _out_dt("gather_segment_topk", params, out_dtype)
    if params.dim() != 2 or params.shape[0] < 1:
        raise ValueError("gather_segment_topk: params is [rows, d], one row at least")
    if (seg_ptr is None) == (count is None):
        raise ValueError("gather_segment_topk: pass seg_ptr or count")
    size, k = int(size), int(k)
    if not 1 <= k <= 16:
        raise ValueError("gather_segment_topk: k is 1..16")
    if size < 0 or size >= 2 ** 31:
        raise ValueError("gather_segment_topk: size is 0 .. 2^31 - 1")
    params = params.contiguous()
    _need_cuda(params)
    gi = gather_indices
    if gi is not None:
        if gi.dtype.is_floating_point or gi.dtype == torch.bool:
            raise ValueError("gather_segment_topk: gather indices are integers, not %s" % gi.dtype)
        gi = gi.reshape(-1)
        gi = gi.contiguous() if gi.dtype == torch.int64 else gi.to(torch.int32).contiguous()
        _need_cuda(params, gi)
        if validate:
            _check_rows("gather_segment_topk", gi, params.shape[0])
    sp = None
    if seg_ptr is not None:
        sp = seg_ptr.to(torch.int64).contiguous()
        _need_cuda(params, sp)
        if sp.numel() != size + 1:
            raise ValueError("gather_segment_topk: seg_ptr has size + 1 entries")
        e = gi.numel() if gi is not None else int(params.shape[0])
        count = 0
    else:
        count = int(count)
        if count < 1:
            raise ValueError("gather_segment_topk: count >= 1")
        e = size * count
        if gi is not None and gi.numel() != e:
            raise ValueError("gather_segment_topk: size * count gather indices")
    if e >= 2 ** 31:
        raise ValueError("gather_segment_topk: fewer than 2^31 positions")
    # (the positions are asked of the kernel only where a backward pass can follow)
    need = params.requires_grad and torch.is_grad_enabled()
    out, sel = _GatherSegmentTopk.apply(params, gi, sp, count, e, size, k, float(fill), od, bool(return_indices), need)
    return (out, sel) if return_indices else out


# ---- edge-weighted aggregation ---------------------------------------------------------------
def _edge_weight(name, w, e, params):
    """checks an edge_weight argument; -> (the weights as a contiguous [E, H] tensor, H)"""
    _dt(name, params)
    if w.dtype != _F32 and (w.dtype != params.dtype or w.dtype not in _DT):
        raise TypeError("%s: edge_weight is float32 or the dtype of params (%s), not %s"
                        % (name, params.dtype, w.dtype))
    _need_cuda(w)
    if w.dim() == 1:
        w2 = w.reshape(-1, 1)
    elif w.dim() == 2:
        w2 = w
    else:
        raise ValueError("%s: edge_weight is [E], [E, 1] or [E, H]" % name)
    if w2.shape[0] != e:
        raise ValueError("%s: one weight row per edge (%d), not %d" % (name, e, w2.shape[0]))
    heads, d = int(w2.shape[1]), int(params.shape[1])
    if heads < 1 or d % heads != 0:
        raise ValueError("%s: the %d weights of an edge do not divide the %d columns" % (name, heads, d))
    return w2.contiguous(), heads


def _gather_scatter_w_raw(mode, params, gi, si, size, w2, heads, out_dtype=None, validate=False):
    """the weighted fused reduce; gi None: update p is row p of params"""
    code = _dt("gather_scatter", params)
    od = _out_dt("gather_scatter", params, out_dtype)
    params = params.contiguous()
    si = si.to(torch.int32).contiguous()
    _need_cuda(params, si, w2)
    if gi is not None:
        gi = gi.to(torch.int32).contiguous()
        _need_cuda(gi)
        if gi.numel() != si.numel():
            raise ValueError("gather_scatter: one gather index and one scatter index per edge")
        if validate:
            _check_rows("gather_scatter", gi, params.shape[0])
    e, d = si.numel(), params.shape[1]
    out = torch.empty((int(size), d), dtype=od, device=params.device)
    with _on(params.device):
        check(lib().euler_gpu_gather_scatter_w_t(_stream(), mode, _ptr(params), code, _ptr(gi), _ptr(si),
                                                 e, d, int(size), _ptr(out), _DT[od], _ptr(w2),
                                                 _DT[w2.dtype], heads))
    return out


def _edge_dot_raw(a, ai, b, bi, heads, od):
    """[E, heads] per-edge dot products (euler_gpu_edge_dot_t); ai / bi None: row p"""
    ca, cb = _dt("edge_dot", a), _dt("edge_dot", b)
    a, b = a.contiguous(), b.contiguous()
    _need_cuda(a, b)
    if ai is not None:
        ai = ai.to(torch.int32).contiguous()
        _need_cuda(ai)
    if bi is not None:
        bi = bi.to(torch.int32).contiguous()
        _need_cuda(bi)
    e = ai.numel() if ai is not None else bi.numel() if bi is not None else a.shape[0]
    d = a.shape[1]
    if d == 0:
        return torch.zeros((e, heads), dtype=od, device=a.device)
    out = torch.empty((e, heads), dtype=od, device=a.device)
    with _on(a.device):
        check(lib().euler_gpu_edge_dot_t(_stream(), _ptr(a), ca, _ptr(ai), _ptr(b), cb, _ptr(bi), e, d,
                                         heads, _ptr(out), _DT[od]))
    return out


def _weighted_backward(op, params, gi, si, w, out, size, grad, refwd):
    """(grad_params, grad_edge_weight) of reduce(op, gather(params, gi) * w, si, size): the
    gradients of the composition under autograd.  add / mean: with G = grad (add) or
    grad / (count + 1e-7) (mean) in fp32, grad_params is the weighted fused op itself with the
    roles swapped - rows of G gathered by si, scattered by gi, the same w: the same operand pairs
    and the same stable grouping as the composition - and grad_edge_weight the per-edge dot
    product of G[si] and params[gi]; neither builds an [E, D] block.  max needs the values of the
    messages for the tie rule of mp_ops.py:53-62 and materialises them."""
    e = si.numel()
    w2 = w.reshape(e, -1)
    heads = w2.shape[1]
    w32 = w2.float().contiguous()
    n = params.shape[0]
    if op == "max":
        if out.dtype != _F32:       # the maxima as fp32: a rounded one equals no message
            out = refwd()
        x = _gather_raw(params, gi, _F32)
        wexp = w32.repeat_interleave(params.shape[1] // heads, dim=1)
        per_edge = _max_per_edge(x * wexp, out, si, size, grad)
        grad_params = _scatter_raw(_ADD, per_edge * wexp, gi, n)
        grad_w = per_edge * x             # (dh = 1: the product itself)
        if params.shape[1] != heads:
            grad_w = grad_w.view(e, heads, -1).sum(-1)
    else:
        g = grad.float() if op == "add" else grad / _count(si, size, grad.device)
        # here the scatter keys are GATHER indices, and the products with G's rows are formed
        # inside the kernels, where nothing can be zeroed afterwards: an update with a key
        # outside [0, size) (_keys_in_range) reads a row of zeros appended to G, with a weight of 0
        valid, key = _keys_in_range(si, size)
        key = torch.where(valid.reshape(-1), key, torch.full_like(key, size))
        g = torch.cat([g, g.new_zeros((1, g.shape[1]))])
        grad_params = _gather_scatter_w_raw(_ADD, g, key, gi, n, w32.masked_fill(~valid, 0), heads)
        grad_w = _edge_dot_raw(g, key, params, gi, heads, _F32).masked_fill_(~valid, 0)
    return grad_params.to(params.dtype), grad_w.to(w.dtype).reshape(w.shape)


class _GatherScatterW(torch.autograd.Function):
    """gather_scatter with edge_weight (euler_gpu_gather_scatter_w)"""

    @staticmethod
    def forward(ctx, params, gather_indices, scatter_indices, size, op, validate, out_dtype, w):
        w2, heads = _edge_weight("gather_scatter", w, gather_indices.numel(), params)
        out = _gather_scatter_w_raw(_GS_MODE[op], params, gather_indices, scatter_indices, size, w2, heads,
                                    out_dtype, validate)
        ctx.save_for_backward(params, gather_indices, scatter_indices, w, out)
        ctx.size, ctx.op = size, op
        return out

    @staticmethod
    def backward(ctx, grad):
        params, gi, si, w, out = ctx.saved_tensors
        w2 = w.reshape(gi.numel(), -1).contiguous()
        refwd = lambda: _gather_scatter_w_raw(_MAX, params, gi, si, ctx.size, w2, w2.shape[1], _F32)
        gp, gw = _weighted_backward(ctx.op, params, gi, si, w, out, ctx.size, grad, refwd)
        return gp, None, None, None, None, None, None, gw


class _GatherSegmentReduceW(torch.autograd.Function):
    """gather_segment_reduce with edge_weight (euler_gpu_gather_segment_reduce_w_t / _ids_w_t)"""

    @staticmethod
    def _raw(mode, params, gi, as_ids, sp, count, size, w2, heads, od):
        rows, d = params.shape
        out = torch.empty((size, d), dtype=od, device=params.device)
        with _on(params.device):
            if as_ids:
                check(lib().euler_gpu_gather_segment_reduce_ids_w_t(
                    _stream(), mode, _ptr(params), _DT[params.dtype], rows, _ptr(gi), _ptr(sp), count, d, size,
                    _ptr(out), _DT[od], _ptr(w2), _DT[w2.dtype], heads))
            else:
                check(lib().euler_gpu_gather_segment_reduce_w_t(
                    _stream(), mode, _ptr(params), _DT[params.dtype], _ptr(gi), _ptr(sp), count, d, size,
                    _ptr(out), _DT[od], _ptr(w2), _DT[w2.dtype], heads))
        return out

    @staticmethod
    def forward(ctx, params, gather_indices, seg_ptr, count, size, op, validate, out_dtype, w):
        _dt("gather_segment_reduce", params)
        od = _out_dt("gather_segment_reduce", params, out_dtype)
        w2, heads = _edge_weight("gather_segment_reduce", w, gather_indices.numel(), params)
        params, gi, as_ids, sp = _segment_args(params, gather_indices, seg_ptr, count, size, validate)
        out = _GatherSegmentReduceW._raw(_GS_MODE[op], params, gi, as_ids, sp, count, size, w2, heads, od)
        if as_ids and (ctx.needs_input_grad[0] or ctx.needs_input_grad[8]):
            gi = _saved_rows(gi, params.shape[0])
        ctx.save_for_backward(params, gi, sp if sp is not None else torch.empty(0), w, out)
        ctx.has_ptr, ctx.count, ctx.size, ctx.op = sp is not None, count, size, op
        return out

    @staticmethod
    def backward(ctx, grad):
        params, gi, sp, w, out = ctx.saved_tensors
        si = _segment_dst(sp if ctx.has_ptr else None, ctx.count, ctx.size, grad.device)
        w2 = w.reshape(gi.numel(), -1).contiguous()
        refwd = lambda: _gather_scatter_w_raw(_MAX, params, gi, si, ctx.size, w2, w2.shape[1], _F32)
        gp, gw = _weighted_backward(ctx.op, params, gi, si, w, out, ctx.size, grad, refwd)
        return gp, None, None, None, None, None, None, None, gw


class _EdgeDot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, a_index, b, b_index, heads, od):
        ctx.save_for_backward(a, b, *[t for t in (a_index, b_index) if t is not None])
        ctx.has = (a_index is not None, b_index is not None)
        ctx.heads = heads
        return _edge_dot_raw(a, a_index, b, b_index, heads, od)

    @staticmethod
    def backward(ctx, grad):
        a, b = ctx.saved_tensors[:2]
        rest = list(ctx.saved_tensors[2:])
        ai = rest.pop(0) if ctx.has[0] else None
        bi = rest.pop(0) if ctx.has[1] else None
        g = grad.float().contiguous()
        e = g.shape[0]
        every = None
        if ai is None or bi is None:
            every = torch.arange(e, device=g.device, dtype=torch.int32)
        ga = gb = None
        if ctx.needs_input_grad[0]:       # d out[p, h] / d a[ai[p]] = grad[p, h] * b[bi[p]]
            ga = _gather_scatter_w_raw(_ADD, b, bi, ai if ai is not None else every, a.shape[0], g,
                                       ctx.heads, _F32).to(a.dtype)
        if ctx.needs_input_grad[2]:
            gb = _gather_scatter_w_raw(_ADD, a, ai, bi if bi is not None else every, b.shape[0], g,
                                       ctx.heads, _F32).to(b.dtype)
        return ga, None, gb, None, None, None


def edge_dot(a, a_index, b, b_index, heads=1, out_dtype=None):
    """out[p, h] = sum_c a[a_index[p], h * dh + c] * b[b_index[p], h * dh + c] with dh = D // heads:
    the dot product of two gathered rows per edge (and per head) - AGNN's attention logit, the
    gradient of an edge-weighted aggregation with respect to its weights - without either [E, D]
    block (euler_gpu_edge_dot).  a and b are [*, D] tables in fp32, bf16 or fp16 (each its own),
    the indices int32 [E] (None: row p).  fp32 products and sums in a fixed order; out_dtype:
    torch.float32, or a 16-bit dtype (rounded once); None = the dtype of a and b when they agree,
    else float32.  Returns [E, heads].
    grad_a = gather_scatter("add", b, b_index, a_index, rows_a, edge_weight=grad_out), grad_b the
    same with the roles swapped."""
    _dt("edge_dot", a)
    _dt("edge_dot", b)
    _need_cuda(a, b)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("edge_dot: a and b are [rows, D] tables of one D")
    heads = int(heads)
    if heads < 1 or a.shape[1] % heads != 0:
        raise ValueError("edge_dot: heads must divide D")
    if out_dtype is None:
        out_dtype = a.dtype if a.dtype == b.dtype else _F32
    if out_dtype not in _DT:
        raise TypeError("edge_dot: out_dtype is float32, bfloat16 or float16, not %s" % out_dtype)
    e = a_index.numel() if a_index is not None else b_index.numel() if b_index is not None else a.shape[0]
    if (b_index is not None and b_index.numel() != e) or (a_index is None and a.shape[0] != e) or \
            (b_index is None and b.shape[0] != e):
        raise ValueError("edge_dot: one row of a and one of b per edge")
    return _EdgeDot.apply(a, a_index, b, b_index, heads, out_dtype)


# ---- GCN-normalised aggregation (norm_i * norm_j * x_j) -----------------------------------------
def _gcn_edges(name, edge_index, size, seg_ptr, count):
    """the edge arguments of gcn_norm / gcn_aggregate -> (dst keys | None, src, seg_ptr | None, count,
    n_dst, n_src): destinations by key (edge_index is [2, E] or a pair (dst, src)) or by segment
    (edge_index is the source column, with seg_ptr or count)"""
    try:
        n_dst, n_src = (int(s) for s in size)
    except (TypeError, ValueError):
        raise ValueError("%s: size is (n_dst, n_src)" % name)
    if n_dst < 0 or n_src < 0:
        raise ValueError("%s: size is (n_dst, n_src), both >= 0" % name)
    if seg_ptr is not None and count is not None:
        raise ValueError("%s: pass seg_ptr or count, not both" % name)
    pair = isinstance(edge_index, (tuple, list)) or edge_index.dim() == 2
    segmented = seg_ptr is not None or count is not None
    if pair and segmented:
        raise ValueError("%s: destinations come as keys (edge_index [2, E]) or as seg_ptr / count with "
                         "the source column alone, not both" % name)
    if not pair and not segmented:
        raise ValueError("%s: a source column alone needs seg_ptr or count" % name)
    if pair:
        if len(edge_index) != 2:
            raise ValueError("%s: edge_index is [2, E] or (dst, src)" % name)
        dst, src = edge_index[0], edge_index[1]
        if dst.dim() != 1 or src.dim() != 1 or dst.numel() != src.numel():
            raise ValueError("%s: one destination and one source per edge" % name)
    else:
        dst, src = None, edge_index
        if src.dim() != 1:
            raise ValueError("%s: the source column is [E]" % name)
    for t in (dst, src):
        if t is not None and (t.dtype.is_floating_point or t.dtype == torch.bool):
            raise ValueError("%s: indices are integers, not %s" % (name, t.dtype))
    if dst is not None:
        dst = dst.to(torch.int32).contiguous()
    src = src.to(torch.int32).contiguous()
    _need_cuda(src)
    if src.numel() >= 2 ** 31:
        raise ValueError("%s: fewer than 2^31 edges" % name)
    sp = None
    if seg_ptr is not None:
        sp = seg_ptr.to(torch.int64).contiguous()
        _need_cuda(sp)
        if sp.numel() != n_dst + 1:
            raise ValueError("%s: seg_ptr has n_dst + 1 entries" % name)
        count = 0
    elif count is not None:
        count = int(count)
        if count < 1:
            raise ValueError("%s: count >= 1" % name)
        if src.numel() != n_dst * count:
            raise ValueError("%s: n_dst * count source indices (%d), not %d" % (name, n_dst * count, src.numel()))
    else:
        _need_cuda(dst)
        count = 0
    return dst, src, sp, count, n_dst, n_src


def _gcn_dst(name, dst, src, sp, count, n_dst):
    """the destination key of every edge; a segmented block's are built (_segment_dst)"""
    if dst is not None:
        return dst
    dst = _segment_dst(sp, count, n_dst, src.device)
    if dst.numel() != src.numel():
        raise ValueError("%s: seg_ptr must span the %d source indices, not %d" % (name, src.numel(), dst.numel()))
    return dst


def _gcn_norm_raw(dst, src, n_dst, n_src):
    norm_dst = torch.empty(n_dst, dtype=_F32, device=src.device)
    norm_src = torch.empty(n_src, dtype=_F32, device=src.device)
    with _on(src.device):
        check(lib().euler_gpu_gcn_norm(_stream(), _ptr(dst), _ptr(src), src.numel(), n_dst, n_src,
                                       _ptr(norm_dst), _ptr(norm_src)))
    return norm_dst, norm_src


def gcn_norm(edge_index, size, seg_ptr=None, count=None):
    """(norm_dst [n_dst], norm_src [n_src]) of a block, fp32: norm = 1 / sqrt(degree), the symmetric
    normalisation of GCN / APPNP / SGCN / TAG / ARMA / DNA (gcn_conv.py:33-51), the degree of a node
    being the number of the block's edges at it on its side.  edge_index is [2, E] or a pair
    (dst, src) - row 0 the destinations, as Block.edge_index - and size = (n_dst, n_src); with
    seg_ptr or count (the forms of gather_segment_reduce) edge_index is the source column alone.
    An edge counts iff both its indices are in range; a node without an edge gets 0, not inf (it
    is never multiplied into anything).  A histogram with integer atomics (euler_gpu_gcn_norm): no
    sort, no host wait, the same bits on every call - those of numpy's
    float32(1) / sqrt(float32(deg)).  No gradient flows through the tables."""
    dst, src, sp, count, n_dst, n_src = _gcn_edges("gcn_norm", edge_index, size, seg_ptr, count)
    dst = _gcn_dst("gcn_norm", dst, src, sp, count, n_dst)
    return _gcn_norm_raw(dst, src, n_dst, n_src)


def _gather_reduce_norm_raw(mode, x, gi, si, sp, count, size, norm_dst, norm_src, root, agg_scale, root_scale,
                            od):
    """euler_gpu_gather_reduce_norm_t on checked, contiguous tensors -> [size, D] of dtype od"""
    rows, d = x.shape
    out = torch.empty((size, d), dtype=od, device=x.device)
    with _on(x.device):
        check(lib().euler_gpu_gather_reduce_norm_t(
            _stream(), mode, _ptr(x), _DT[x.dtype], rows, _ptr(gi), _ptr(si), _ptr(sp), int(count), gi.numel(), d,
            size, _ptr(norm_dst), _ptr(norm_src), _ptr(root), _DT[root.dtype] if root is not None else _lib.F32,
            float(agg_scale), float(root_scale), _ptr(out), _DT[od]))
    return out


class _GcnAggregate(torch.autograd.Function):
    """gcn_aggregate.  grad_x is the same entry with the roles swapped: rows of G (grad * agg_scale;
    for mean divided by count + 1e-7, as _weighted_backward) gathered by dst and scattered by src,
    the two norm tables exchanged - the operand pairs and the stable grouping by src of the
    composition's gradient, so its bits.  A destination key outside the block gathers nothing (the
    entry gives such an update the weight 0)."""

    @staticmethod
    def forward(ctx, x, root, dst, src, sp, count, n_dst, norm_dst, norm_src, op, agg_scale, root_scale, od):
        out = _gather_reduce_norm_raw(_GS_MODE[op], x, src, dst, sp, count, n_dst, norm_dst, norm_src, root,
                                      agg_scale, root_scale, od)
        ctx.save_for_backward(src, norm_dst, norm_src, *[t for t in (dst, sp) if t is not None])
        ctx.has = (dst is not None, sp is not None)
        ctx.args = (count, n_dst, x.shape[0], op, agg_scale, root_scale, x.dtype,
                    root.dtype if root is not None else None)
        return out

    @staticmethod
    def backward(ctx, grad):
        src, norm_dst, norm_src = ctx.saved_tensors[:3]
        rest = list(ctx.saved_tensors[3:])
        dst = rest.pop(0) if ctx.has[0] else None
        sp = rest.pop(0) if ctx.has[1] else None
        count, n_dst, n_src, op, agg_scale, root_scale, x_dtype, root_dtype = ctx.args
        g32 = grad.float().contiguous()
        grad_x = grad_root = None
        if ctx.needs_input_grad[0]:
            g = g32 if agg_scale == 1.0 else g32 * agg_scale
            keys = _gcn_dst("gcn_aggregate", dst, src, sp, count, n_dst)
            if op == "mean":
                if dst is not None:
                    cnt = _count(dst, n_dst, g.device)
                elif sp is not None:
                    cnt = (sp[1:] - sp[:-1]).to(_F32).reshape(-1, 1) + 1e-7
                else:
                    cnt = torch.full((n_dst, 1), float(count), dtype=_F32, device=g.device) + 1e-7
                g = g / cnt
            grad_x = _gather_reduce_norm_raw(_ADD, g.contiguous(), keys, src, None, 0, n_src, norm_src, norm_dst,
                                             None, 1.0, 1.0, _F32).to(x_dtype)
        if root_dtype is not None and ctx.needs_input_grad[1]:
            grad_root = (g32 if root_scale == 1.0 else g32 * root_scale).to(root_dtype)
        return (grad_x, grad_root) + (None,) * 11


def gcn_aggregate(x, edge_index, size, norm=None, op="add", root=None, alpha=None, root_scale=None,
                  seg_ptr=None, count=None, out_dtype=None, validate=False):
    """The aggregation of GCNConv / SGCNConv / TAGConv (op "add"), DNAConv (op "mean"), and with a
    root term a whole APPNPConv / ARMAConv step, in one pass (euler_gpu_gather_reduce_norm_t):
        out[i] = reduce over the edges (i, j) of norm_dst[i] * norm_src[j] * x[j]
    x is the source-side table [n_src, D] (fp32 / bf16 / fp16), size = (n_dst, n_src), edge_index
    [2, E] or a pair (dst, src); with seg_ptr or count edge_index is the source column alone (see
    gcn_norm).  norm is gcn_norm's pair of tables (fp32); None computes them here, once, and keeps
    them for the backward pass.  The weight norm_dst[i] * norm_src[j], the message and the sum are
    separate fp32 roundings in input order: the bits of
    gather_scatter(op, x, src, dst, n_dst, edge_weight=norm_dst[dst] * norm_src[src]) without the
    [E] weight, its two gathers and its multiply.  mean divides by (edges of i + 1e-7).
    root ([n_dst, D], the dtype of x or fp32) adds the destination's own row in the same pass:
    out = agg * a + root * b, three fp32 roundings before the one to out_dtype.  alpha is shorthand
    for (a, b) = (1 - alpha, alpha) (appnp_conv.py:57-60); root without alpha uses (1, 1)
    (arma_conv.py:72-75); root_scale overrides b.
    An edge whose destination is outside [0, n_dst) or whose source is outside [0, n_src) contributes
    nothing, and its gradient is exactly 0; validate=True checks the source indices first (one
    host wait).  out_dtype as gather_scatter.  Gradients flow to x and root (the same fused entry
    with the roles swapped: no [E] or [E, D] tensor in either direction), none through norm."""
    if op not in ("add", "mean"):
        raise ValueError("gcn_aggregate: op is add or mean")
    _dt("gcn_aggregate", x)
    od = _out_dt("gcn_aggregate", x, out_dtype)
    dst, src, sp, count, n_dst, n_src = _gcn_edges("gcn_aggregate", edge_index, size, seg_ptr, count)
    _need_cuda(x)
    if x.dim() != 2 or x.shape[0] != n_src:
        raise ValueError("gcn_aggregate: x is the source-side table [n_src, D]")
    if op == "mean" and src.numel() >= (1 << 24):
        raise ValueError("gcn_aggregate: a mean needs fewer than 2^24 edges")
    if validate:
        _check_rows("gcn_aggregate", src, n_src)
    if norm is None:
        norm = _gcn_norm_raw(_gcn_dst("gcn_aggregate", dst, src, sp, count, n_dst), src, n_dst, n_src)
    norm_dst, norm_src = norm
    for t, n, side in ((norm_dst, n_dst, "norm_dst"), (norm_src, n_src, "norm_src")):
        if t.dtype != _F32:
            raise TypeError("gcn_aggregate: %s is float32, not %s" % (side, t.dtype))
        if t.dim() != 1 or t.numel() != n:
            raise ValueError("gcn_aggregate: %s has %d entries, not %s" % (side, n, tuple(t.shape)))
        _need_cuda(t)
    agg_scale, b = 1.0, 1.0
    if alpha is not None:
        if root is None:
            raise ValueError("gcn_aggregate: alpha needs root")
        agg_scale, b = 1.0 - float(alpha), float(alpha)
    if root_scale is not None:
        if root is None:
            raise ValueError("gcn_aggregate: root_scale needs root")
        b = float(root_scale)
    if root is not None:
        if root.dtype != _F32 and root.dtype != x.dtype:
            raise TypeError("gcn_aggregate: root is float32 or the dtype of x (%s), not %s" % (x.dtype, root.dtype))
        if root.dim() != 2 or tuple(root.shape) != (n_dst, x.shape[1]):
            raise ValueError("gcn_aggregate: root is [n_dst, D] = %s, not %s"
                             % ((n_dst, x.shape[1]), tuple(root.shape)))
        _need_cuda(root)
        root = root.contiguous()
        # the scales as the fp32 numbers the kernel multiplies by
        agg_scale, b = float(np.float32(agg_scale)), float(np.float32(b))
    return _GcnAggregate.apply(x.contiguous(), root, dst, src, sp, count, n_dst, norm_dst.detach().contiguous(),
                               norm_src.detach().contiguous(), op, agg_scale, b, od)


# ---- fused softmax over the updates of a destination ------------------------------------------
def _edge_softmax_raw(x2, grad2, si, sp, count, size, od):
    """euler_gpu_edge_softmax (grad2 None) / euler_gpu_edge_softmax_grad (x2 = the forward's
    output) on contiguous [E, H] tensors; -> [E, H] of dtype od"""
    e, heads = x2.shape
    out = torch.empty((e, heads), dtype=od, device=x2.device)
    if e == 0:
        return out
    if heads == 0:
        raise ValueError("edge_softmax: heads < 1")
    with _on(x2.device):
        if grad2 is None:
            check(lib().euler_gpu_edge_softmax(_stream(), _ptr(x2), _DT[x2.dtype], _ptr(si), _ptr(sp),
                                               int(count), e, heads, int(size), _ptr(out), _DT[od]))
        else:
            check(lib().euler_gpu_edge_softmax_grad(_stream(), _ptr(x2), _DT[x2.dtype], _ptr(grad2),
                                                    _DT[grad2.dtype], _ptr(si), _ptr(sp), int(count), e,
                                                    heads, int(size), _ptr(out), _DT[od]))
    return out


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, si, sp, count, size, od):
        x2 = logits.reshape(logits.shape[0], 1 if logits.dim() == 1 else logits.shape[1]).contiguous()
        # the backward reads the forward's fp32 output; a 16-bit visible one is its rounding
        keep = ctx.needs_input_grad[0] and od != _F32
        y = _edge_softmax_raw(x2, None, si, sp, count, size, _F32 if keep else od)
        ctx.save_for_backward(y, *[t for t in (si, sp) if t is not None])
        ctx.has, ctx.count, ctx.size, ctx.in_dtype = (si is not None, sp is not None), count, size, logits.dtype
        return (y.to(od) if keep else y).reshape(logits.shape)

    @staticmethod
    def backward(ctx, grad):
        y = ctx.saved_tensors[0]
        rest = list(ctx.saved_tensors[1:])
        si = rest.pop(0) if ctx.has[0] else None
        sp = rest.pop(0) if ctx.has[1] else None
        g2 = grad.reshape(y.shape).contiguous()
        if g2.dtype not in _DT:
            g2 = g2.float()
        gx = _edge_softmax_raw(y, g2, si, sp, ctx.count, ctx.size, ctx.in_dtype)
        return gx.reshape(grad.shape), None, None, None, None, None


def edge_softmax(logits, indices=None, size=None, seg_ptr=None, count=None, out_dtype=None):
    """The softmax of the logits over the updates of every destination, in one read and one write
    (euler_gpu_edge_softmax): what GATConv / AGNNConv run between `edge_dot` and an aggregation
    with edge_weight.  logits is [E], [E, 1] or [E, H] (one column per head) in fp32, bf16 or fp16;
    the output has its shape.  The destinations come in exactly one form: `indices` (int32 [E]
    scatter keys in any order, with `size`), `seg_ptr` (int64 [size + 1] offsets) or `count`
    (updates per destination, with `size`) - the forms of gather_scatter and
    gather_segment_reduce.  Arithmetic in fp32 with the library's own exp and a fixed summation
    order: the same segment gives the same bits through every form - not the bits of
    `scatter_softmax`, which stays the reference's composition.  out_dtype: torch.float32 or the
    input's dtype (None), rounded once.  Updates that belong to no destination (a key outside
    [0, size), a position outside [seg_ptr[0], seg_ptr[size])) get 0.
    Differentiable: grad = y * (g - sum_q y_q g_q) per destination (euler_gpu_edge_softmax_grad),
    on the fp32 output."""
    _dt("edge_softmax", logits)
    od = _out_dt("edge_softmax", logits, out_dtype)
    _need_cuda(logits)
    if logits.dim() not in (1, 2):
        raise ValueError("edge_softmax: logits is [E], [E, 1] or [E, H]")
    if logits.dim() == 2 and logits.shape[1] < 1:
        raise ValueError("edge_softmax: logits needs at least one head")
    if (indices is not None) + (seg_ptr is not None) + (count is not None) != 1:
        raise ValueError("edge_softmax: pass exactly one of indices, seg_ptr and count")
    e = int(logits.shape[0])
    si = sp = None
    if indices is not None:
        if size is None:
            raise ValueError("edge_softmax: indices need size")
        si = indices.to(torch.int32).contiguous()
        _need_cuda(si)
        if si.numel() != e:
            raise ValueError("edge_softmax: one index per edge (%d), not %d" % (e, si.numel()))
    elif seg_ptr is not None:
        sp = seg_ptr.to(torch.int64).contiguous()
        _need_cuda(sp)
        if size is None:
            size = sp.numel() - 1
        if sp.numel() != int(size) + 1:
            raise ValueError("edge_softmax: seg_ptr has size + 1 entries")
    else:
        count = int(count)
        if count < 1:
            raise ValueError("edge_softmax: count >= 1")
        if size is None:
            size = e // count
        if int(size) * count != e:
            raise ValueError("edge_softmax: size * count logit rows")
    if int(size) < 0:
        raise ValueError("edge_softmax: size >= 0")
    return _EdgeSoftmax.apply(logits, si, sp, 0 if count is None else count, int(size), od)


# ---- fused segment attention: logits, softmax and weighted sum in one pass ---------------------
_ATT_KIND = {"dot": 0, "additive": 1}


def _att_dst(si, sp, count, size, e, device):
    """the destination of every update as int32 [E]; outside [0, size) where it has none"""
    if si is not None:
        return si
    if sp is None:
        return torch.arange(size, device=device, dtype=torch.int32).repeat_interleave(int(count))
    pos = torch.arange(e, device=device, dtype=torch.int64)
    dst = torch.searchsorted(sp, pos, right=True) - 1          # -1 before seg_ptr[0]
    return torch.where(pos >= sp[-1], torch.full_like(dst, size), dst).to(torch.int32)


def _att_rows(gi, n_rows):
    """the int32 rows the kernels read: the low word as unsigned, clamped to the table's last row"""
    return torch.clamp(gi.to(torch.int64) & 0xFFFFFFFF, max=n_rows - 1).to(torch.int32)


def _att_call(fn, kind, q, qi, k, v, gi, si, sp, count, size, heads, scale, slope, tail):
    d = k.shape[1]
    dv = v.shape[1] if v is not None else d
    with _on(k.device):
        check(fn(_stream(), kind, _ptr(q), _DT[q.dtype] if q is not None else 0, q.shape[0] if q is not None else 0,
                 _ptr(qi), _ptr(k), _DT[k.dtype], k.shape[0], _ptr(v), _DT[v.dtype] if v is not None else 0,
                 v.shape[0] if v is not None else 0, _ptr(gi), int(gi.dtype == torch.int64), _ptr(si), _ptr(sp),
                 int(count), gi.numel(), d, dv, heads, size, float(scale), float(slope), *tail))


class _AttentionAggregate(torch.autograd.Function):
    """euler_gpu_segment_attention, and for the backward euler_gpu_segment_attention_grad at the
    destinations plus the weighted reduces grouped by source row"""

    @staticmethod
    def forward(ctx, q, k, v, kind, qi, gi, si, sp, count, size, heads, scale, slope, od, want_logits):
        e = gi.numel()
        dv = v.shape[1] if v is not None else k.shape[1]
        dev = k.device
        alpha = torch.empty((e, heads), dtype=_F32, device=dev)
        logits = torch.zeros((e, heads), dtype=_F32, device=dev) if want_logits else None
        if e == 0 or size == 0:
            out = torch.zeros((size, dv), dtype=od, device=dev)
            alpha.zero_()
        else:
            out = torch.empty((size, dv), dtype=od, device=dev)
            _att_call(lib().euler_gpu_segment_attention, kind, q, qi, k, v, gi, si, sp, count, size, heads,
                      scale, slope, (_ptr(out), _DT[od], _ptr(alpha), _ptr(logits)))
        ctx.save_for_backward(alpha, *[t for t in (q, k, v, qi, gi, si, sp) if t is not None])
        ctx.has = [t is not None for t in (q, k, v, qi, gi, si, sp)]
        ctx.conf = (kind, count, size, heads, scale, slope)
        if want_logits:
            ctx.mark_non_differentiable(alpha, logits)
            return out, alpha, logits
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    def backward(ctx, grad, *unused):
        saved = list(ctx.saved_tensors)
        alpha = saved.pop(0)
        q, k, v, qi, gi, si, sp = [saved.pop(0) if h else None for h in ctx.has]
        kind, count, size, heads, scale, slope = ctx.conf
        e, d = gi.numel(), k.shape[1]
        need_q = q is not None and ctx.needs_input_grad[0]
        need_k, need_v = ctx.needs_input_grad[1], v is not None and ctx.needs_input_grad[2]
        gq = gk = gv = None
        if e == 0 or size == 0:
            gq = torch.zeros_like(q) if need_q else None
            gk = torch.zeros_like(k) if need_k else None
            gv = torch.zeros_like(v) if need_v else None
            return (gq, gk, gv) + (None,) * 12
        g2 = grad.contiguous()
        if g2.dtype not in _DT:
            g2 = g2.float()
        ds = torch.empty((e, heads), dtype=_F32, device=k.device)
        dq_dst = torch.empty((size, d), dtype=_F32, device=k.device)
        _att_call(lib().euler_gpu_segment_attention_grad, kind, q, qi, k, v, gi, si, sp, count, size, heads,
                  scale, slope, (_ptr(alpha), _ptr(g2), _DT[g2.dtype], _ptr(ds), _ptr(dq_dst)))
        # the source side: an update without a destination has alpha = ds = 0 and reads a row of zeros
        dst = _att_dst(si, sp, count, size, e, k.device)
        if si is not None or sp is not None:
            valid, key = _keys_in_range(dst, size)
            key = torch.where(valid.reshape(-1), key, torch.full_like(key, size))
        else:
            key = dst
        rows_k = _att_rows(gi, k.shape[0])
        if need_v or (v is None and need_k):
            tv = v if v is not None else k
            g32 = g2.float()                               # (fp32 already: no copy)
            if si is not None or sp is not None:           # the zero row of updates without a destination
                g32 = torch.cat([g32, g32.new_zeros((1, g32.shape[1]))])
            gv = _gather_scatter_w_raw(_ADD, g32, key, rows_k if v is None else _att_rows(gi, v.shape[0]),
                                       tv.shape[0], alpha, heads, _F32)
        if need_k:
            if kind == 0:
                q_of_dst = torch.clamp(key, max=size - 1)
                if qi is not None:
                    q_of_dst = qi[q_of_dst.long()]
                gk = _gather_scatter_w_raw(_ADD, q, q_of_dst, rows_k, k.shape[0], ds, heads, _F32)
            else:
                gk = _scatter_raw(_ADD, ds, rows_k, k.shape[0])
            if v is None:
                gk = gv + gk                               # (fp32, grad_v first)
            gk = gk.to(k.dtype)
        if need_q:
            if qi is not None:
                gq = _scatter_raw(_ADD, dq_dst, qi, q.shape[0])
            elif q.shape[0] > size:
                gq = torch.cat([dq_dst, dq_dst.new_zeros((q.shape[0] - size, d))])
            else:
                gq = dq_dst
            gq = gq.to(q.dtype)
        return (gq, gk, gv.to(v.dtype) if need_v else None) + (None,) * 12


def attention_aggregate(kind, q, k, gather_indices, size, v=None, q_index=None, heads=1, scale=1.0,
                        negative_slope=0.2, indices=None, seg_ptr=None, count=None, out_dtype=None,
                        return_attention=False, validate=False, return_logits=False):
    """Attention over the updates of every destination in ONE pass (euler_gpu_segment_attention):
    a logit per (update, head), the softmax over the destination's updates, and the sum of the
    gathered rows weighted by it - what GATConv, AGNNConv, AttentionPool and Set2SetPool compose from
    `edge_dot` (or two gathers), `edge_softmax` and a weighted reduce.  For destination r (qr =
    q_index[r], or r), update p with g = gather_indices[p] and head h:
      kind "dot":       logit = scale * sum_c q[qr, h*dh+c] * k[g, h*dh+c]; q and k are [*, D],
                        dh = D // heads.  AGNN: q = beta * l2norm(x), k = l2norm(x), v = x;
                        Set2Set: q per graph, k = the inputs, v = None; dot-product attention.
      kind "additive":  logit = leaky_relu(q[qr, h] + k[g, h], negative_slope); q and k are score
                        tables [*, heads]; q = None means 0, negative_slope = 1.0 the identity.
                        GAT; AttentionPool is q = None, slope 1, k = the gate.  Needs v.
      alpha = softmax of the logits over the destination's updates (the bits of `edge_softmax`);
      out[r, h*dv+c] = sum_p alpha[p, h] * v[g, h*dv+c], v [*, Dv], dv = Dv // heads (the bits of
      gather_segment_reduce("add", v, gather_indices, size, edge_weight=alpha)).
    v = None (dot only) means v is k: every gathered row is loaded once for the logit and the sum.
    Tables are fp32, bf16 or fp16, each its own; gather_indices int32, or the int64 ids a sampler
    returned (read in place); a row number past a table reads its last row.  The destinations come in
    exactly one form - indices (scatter keys, any order, with size), seg_ptr or count - as for
    `edge_softmax`.  Returns [size, Dv] in out_dtype (None: the dtype of v); an empty destination is
    a zero row; updates that belong to no destination contribute nothing and get alpha = 0 and a
    zero gradient.  return_attention=True also returns the fp32 alpha [E, heads] (not
    differentiable on its own), return_logits=True the fp32 logits after it.
    `scale` is a plain float and is not differentiated: a learnable temperature belongs in q
    (q = beta * x).  Measured on a sampled block: the one-table dot form (v = None) is level
    with or faster than edge_dot + edge_softmax + the weighted reduce, and so are the graph pools' forwards;
    the additive kind and dot with a separate v are slower than those three ops today - prefer them there.
    return_logits is an addition to the op's signature for checks that need the op's own logits.
    Differentiable in q, k and v: the destination side in one pass
    (euler_gpu_segment_attention_grad), the source side by the weighted reduces."""
    if kind not in _ATT_KIND:
        raise ValueError("attention_aggregate: kind is dot or additive")
    if (indices is not None) + (seg_ptr is not None) + (count is not None) != 1:
        raise ValueError("attention_aggregate: pass exactly one of indices, seg_ptr and count")
    heads, size = int(heads), int(size)
    if heads < 1 or size < 0:
        raise ValueError("attention_aggregate: heads >= 1 and size >= 0")
    _dt("attention_aggregate", k)
    if k.dim() != 2 or (q is not None and q.dim() != 2) or (v is not None and v.dim() != 2):
        raise ValueError("attention_aggregate: q, k and v are [rows, columns] tables")
    if kind == "additive":
        if v is None:
            raise ValueError("attention_aggregate: additive attention needs v")
        if k.shape[1] != heads or (q is not None and q.shape[1] != heads):
            raise ValueError("attention_aggregate: additive q and k are [*, heads] score tables")
    else:
        if q is None:
            raise ValueError("attention_aggregate: dot attention needs q")
        if q.shape[1] != k.shape[1] or k.shape[1] % heads != 0:
            raise ValueError("attention_aggregate: q and k are [*, D] with heads dividing D")
    if q is not None:
        _dt("attention_aggregate", q)
    if v is not None:
        _dt("attention_aggregate", v)
        if v.shape[1] % heads != 0:
            raise ValueError("attention_aggregate: heads must divide the columns of v")
    tv = v if v is not None else k
    od = tv.dtype if out_dtype is None else out_dtype
    if od not in _DT:
        raise TypeError("attention_aggregate: out_dtype is float32, bfloat16 or float16, not %s" % od)
    if gather_indices.dtype not in (torch.int32, torch.int64):
        raise TypeError("attention_aggregate: gather_indices are int32 or int64")
    gi = gather_indices.reshape(-1).contiguous()
    e = gi.numel()
    tensors = [t.contiguous() if t is not None else None for t in (q, k, v)]
    q, k, v = tensors
    _need_cuda(k, gi, *[t for t in (q, v) if t is not None])
    if e > 0 and (k.shape[0] < 1 or tv.shape[0] < 1):
        raise ValueError("attention_aggregate: a gathered table has no rows")
    si = sp = qi = None
    if indices is not None:
        si = indices.to(torch.int32).reshape(-1).contiguous()
        _need_cuda(si)
        if si.numel() != e:
            raise ValueError("attention_aggregate: one scatter key per gather index (%d), not %d" % (e, si.numel()))
    elif seg_ptr is not None:
        sp = seg_ptr.to(torch.int64).contiguous()
        _need_cuda(sp)
        if sp.numel() != size + 1:
            raise ValueError("attention_aggregate: seg_ptr has size + 1 entries")
    else:
        count = int(count)
        if count < 1 or size * count != e:
            raise ValueError("attention_aggregate: size * count gather indices, count >= 1")
    if q_index is not None:
        qi = q_index.to(torch.int32).reshape(-1).contiguous()
        _need_cuda(qi)
        if qi.numel() != size:
            raise ValueError("attention_aggregate: one q_index per destination (%d), not %d" % (size, qi.numel()))
    elif q is not None and q.shape[0] < size:
        raise ValueError("attention_aggregate: q has fewer rows than there are destinations")
    if q is not None and size > 0 and q.shape[0] < 1:
        raise ValueError("attention_aggregate: q has no rows")
    if validate:
        _check_rows("attention_aggregate", gi, min(k.shape[0], tv.shape[0]))
        if qi is not None:
            _check_rows("attention_aggregate", qi, q.shape[0])
    res = _AttentionAggregate.apply(q, k, v, _ATT_KIND[kind], qi, gi, si, sp, 0 if count is None else count, size,
                                    heads, float(scale), float(negative_slope), od, bool(return_logits))
    if not (return_attention or return_logits):
        return res[0]
    return tuple([res[0]] + ([res[1]] if return_attention else []) + ([res[2]] if return_logits else []))


# ---- per-relation aggregation (RGCN) ----------------------------------------------------------
_REL_MODE = {"add": 0, "max": 1, "mean": 2, "mean_rel": 3}


def _relation_reduce_raw(mode, params, gi, as_ids, et, num_relations, si, sp, count, size, od, want_counts):
    """euler_gpu_relation_reduce on prepared tensors -> (out [size, R, D], counts [size, R] or None)"""
    e, d = et.numel(), params.shape[1]
    out = torch.empty((size, num_relations, d), dtype=od, device=params.device)
    counts = None
    if want_counts:     # (d == 0: the entry touches nothing)
        counts = (torch.zeros if d == 0 else torch.empty)((size, num_relations), dtype=torch.int32,
                                                          device=params.device)
    with _on(params.device):
        check(lib().euler_gpu_relation_reduce(
            _stream(), mode, _ptr(params), _DT[params.dtype], int(params.shape[0]), _ptr(gi), int(as_ids),
            _ptr(et), num_relations, _ptr(si), _ptr(sp), int(count), e, d, size, _ptr(out), _DT[od],
            _ptr(counts)))
    return out, counts


class _RelationReduce(torch.autograd.Function):
    """out[r, t] = reduce(op) of params[gi[p]] over the valid updates of destination r with
    relation t (euler_gpu_relation_reduce).  The gradient is that of the composition
    gather_scatter(op, params, gi, dst * R + t, size * R), built from the same ops."""

    @staticmethod
    def forward(ctx, params, gi, as_ids, et, num_relations, si, sp, count, size, op, od, want_counts):
        need_grad = ctx.needs_input_grad[0]
        mean = op in ("mean", "mean_rel")
        out, counts = _relation_reduce_raw(_REL_MODE[op], params, gi, as_ids, et, num_relations, si, sp, count,
                                           size, od, want_counts or (mean and need_grad))
        if need_grad:
            if gi is None:
                gi = torch.arange(et.numel(), dtype=torch.int32, device=params.device)
            elif as_ids:
                # the clamp-to-last-row rule of the forward kernel for the saved indices
                # (_GatherSegmentReduce.forward)
                gi = torch.clamp(gi & 0xFFFFFFFF, max=int(params.shape[0]) - 1).to(torch.int32)
            none = torch.empty(0)
            ctx.save_for_backward(params, gi, et, si if si is not None else none, sp if sp is not None else none,
                                  counts if mean else none, out if op == "max" else none)
        ctx.form = "indices" if si is not None else "seg_ptr" if sp is not None else "count"
        ctx.count, ctx.size, ctx.R, ctx.op = count, size, num_relations, op
        if not want_counts:
            return out
        ctx.mark_non_differentiable(counts)
        return out, counts

    @staticmethod
    def backward(ctx, grad, *unused):
        params, gi, et, si, sp, counts, out = ctx.saved_tensors
        size, R, op = ctx.size, ctx.R, ctx.op
        e, d = et.numel(), params.shape[1]
        dev = grad.device
        # 1. the scatter key of the composition: bucket dst * R + t, -1 for an update of no bucket
        if ctx.form == "indices":
            dst = si.to(torch.int64)
        elif ctx.form == "seg_ptr":      # the segment that holds position p; `size` past the last one
            dst = torch.searchsorted(sp, torch.arange(e, dtype=torch.int64, device=dev), right=True) - 1
        else:
            dst = torch.arange(size, dtype=torch.int64, device=dev).repeat_interleave(ctx.count)
        t = et.to(torch.int64)
        valid = (dst >= 0) & (dst < size) & (t >= 0) & (t < R)
        key = torch.where(valid, dst * R + t, torch.full_like(dst, -1)).to(torch.int32)
        # 2. the gradient per edge
        if op == "max":
            per_edge = _max_per_edge(_gather_raw(params, gi, _F32), out.view(size * R, d), key, size * R,
                                     grad.reshape(size * R, d).contiguous())
        elif op == "add":
            per_edge = _gather_by_key(grad.reshape(size * R, d).contiguous(), key, _F32)
        else:
            if op == "mean":
                denom = (counts.sum(1) + 1e-7).view(size, 1, 1)
            else:
                denom = (counts + 1e-7).view(size, R, 1)
            per_edge = _gather_by_key((grad / denom).reshape(size * R, d), key)
        # 3. into the rows the edges read, rounded once
        grad_params = _scatter_raw(_ADD, per_edge, gi, params.shape[0]).to(params.dtype)
        return (grad_params,) + (None,) * 11


def relation_reduce(op, params, gather_indices, edge_type, num_relations, size,
                    indices=None, seg_ptr=None, count=None, out_dtype=None, return_counts=False):
    """The typed aggregation of an RGCN layer: out[r, t] reduces (op = "add", "max", "mean" - over
    the destination - or "mean_rel" - over the bucket) the rows params[gather_indices[p]] of the
    updates p of destination r whose relation edge_type[p] is t, in input order and in one pass
    (euler_gpu_relation_reduce).  Returns [size, num_relations, D] (and the int32 counts
    [size, num_relations] with return_counts=True).
    The destinations come in exactly one form - `indices` (int32 [E] scatter keys in any order),
    `seg_ptr` (int64 [size + 1] offsets) or `count` (updates per destination) - the forms of
    gather_scatter and gather_segment_reduce; seg_ptr and count only enqueue (no host wait).
    gather_indices: int32 [E], the int64 ids a sampler returned (read in place: index = low word,
    clamped to the last row, as gather_segment_reduce) or None (update p is row p).
    An update is valid when its destination is in [0, size) and 0 <= edge_type < num_relations; an
    invalid one - the -1 type the samplers write beside a default_node fill - is left out of every
    sum, maximum and count and its gradient is exactly 0.  "mean" divides a bucket's sum by (the
    destination's valid updates + 1e-7) - RelationConv's scatter_mean, relation_conv.py:59 -,
    "mean_rel" by (the bucket's own count + 1e-7); an empty bucket is 0 (-1e9 for max).
    The bits are those of gather_scatter(op, params, gather_indices, dst * R + edge_type, size * R)
    (add, max, "mean_rel" as its mean; "mean" as its add over the destination's denominator), and
    the gradient with respect to params is that composition's.  out_dtype as scatter_add."""
    if op not in _REL_MODE:
        raise ValueError("relation_reduce: op is add, max, mean or mean_rel")
    _dt("relation_reduce", params)
    od = _out_dt("relation_reduce", params, out_dtype)
    if params.dim() != 2:
        raise ValueError("relation_reduce: params is a [rows, D] table")
    if (indices is not None) + (seg_ptr is not None) + (count is not None) != 1:
        raise ValueError("relation_reduce: pass exactly one of indices, seg_ptr and count")
    num_relations, size = int(num_relations), int(size)
    if num_relations < 1 or size < 0:
        raise ValueError("relation_reduce: num_relations >= 1 and size >= 0")
    params = params.contiguous()
    et = edge_type.reshape(-1).to(torch.int32).contiguous()
    _need_cuda(params, et)
    e = et.numel()
    gi, as_ids = None, False
    if gather_indices is not None:
        as_ids = gather_indices.dtype == torch.int64
        gi = gather_indices.reshape(-1)
        gi = gi.contiguous() if as_ids else gi.to(torch.int32).contiguous()
        _need_cuda(gi)
        if gi.numel() != e:
            raise ValueError("relation_reduce: one gather index and one edge type per update")
    elif params.shape[0] < e:
        raise ValueError("relation_reduce: without gather_indices update p is row p of params")
    si = sp = None
    if indices is not None:
        si = indices.reshape(-1).to(torch.int32).contiguous()
        _need_cuda(si)
        if si.numel() != e:
            raise ValueError("relation_reduce: one scatter index and one edge type per update")
        if e == 0:      # (an empty tensor has no address to name the form with)
            si, sp = None, torch.zeros(size + 1, dtype=torch.int64, device=params.device)
    elif seg_ptr is not None:
        sp = seg_ptr.to(torch.int64).contiguous()
        _need_cuda(sp)
        if sp.numel() != size + 1:
            raise ValueError("relation_reduce: seg_ptr has size + 1 entries")
    else:
        if int(count) < 1 or size * int(count) != e:
            raise ValueError("relation_reduce: count >= 1 and size * count updates")
    return _RelationReduce.apply(params, gi, as_ids, et, num_relations, si, sp, 0 if count is None else int(count),
                                 size, op, od, bool(return_counts))


def relation_conv(x, weight, gather_indices, edge_type, size, indices=None, seg_ptr=None, count=None,
                  aggr="mean"):
    """RelationConv.__call__ (relation_conv.py:53-70) without apply_node's fc(x), which stays the
    caller's own Linear: out[r] = aggr over the updates p of destination r of
    weight[edge_type[p]] @ x[gather_indices[p]].  weight is [R, dim, F] (the reference's `matrix`),
    x is [rows, F]; returns [size, dim].  By linearity the per-edge matrices are never gathered:
    relation_reduce(aggr, ...) gives [size, R, F], and one GEMM with the [R * F, dim] matrix
    finishes (plain autograd for weight; relation_reduce's gradient for x).  aggr is "add", "mean"
    (over the destination, the reference's) or "mean_rel"; the arguments are relation_reduce's."""
    if aggr not in ("add", "mean", "mean_rel"):
        raise ValueError("relation_conv: aggr is add, mean or mean_rel (a max does not commute with the matrices)")
    if weight.dim() != 3 or x.dim() != 2 or weight.shape[2] != x.shape[1]:
        raise ValueError("relation_conv: weight is [R, dim, F] and x is [rows, F]")
    r, dim, f = weight.shape
    h = relation_reduce(aggr, x, gather_indices, edge_type, r, size, indices=indices, seg_ptr=seg_ptr,
                        count=count)
    return h.reshape(int(size), r * f) @ weight.permute(0, 2, 1).reshape(r * f, dim)


_KG_KIND = {"trans_l1": 0, "trans_l2": 1, "distmult": 2}
_KG_CORRUPT = {"front": 0, "tail": 1, "both": 2}


def _kg_ids(name, src, rel_id, dst, neg):
    """the ids of a triple-scoring op -> int64 contiguous src, rel_id, dst [B], neg [B, K] or None, and B"""
    src, rel_id, dst = (t.to(torch.int64).reshape(-1).contiguous() for t in (src, rel_id, dst))
    b = src.numel()
    if rel_id.numel() != b or dst.numel() != b:
        raise ValueError("%s: one src, rel_id and dst per triple" % name)
    if neg is not None:
        neg = neg.to(torch.int64)
        neg = (neg if neg.dim() == 2 else neg.reshape(b, -1)).contiguous()
        if neg.shape[0] != b:
            raise ValueError("%s: neg is [B, K]" % name)
    return src, rel_id, dst, neg, b


def _kg_limits(name, b, neg, *row_counts):
    """the kernels' 32-bit limits: the scores of a batch and the rows of every table given"""
    if b * max(1 if neg is None else neg.shape[1], 1) * 2 >= 2 ** 31 or max(row_counts) >= 2 ** 31:
        raise ValueError("%s: B * max(K, 1) * 2 and the %s rows must stay below 2^31"
                         % (name, "table's" if len(row_counts) == 1 else "tables'"))


def _kg_scores_out(b, k, corrupt, empty, device):
    """-> (pos [B], neg_out [B, K']) for a forward entry to fill; zeros when it has nothing to do"""
    make = torch.zeros if empty else torch.empty
    return (make(b, dtype=_F32, device=device),
            make((b, 2 * k if corrupt == "both" else k), dtype=_F32, device=device))


def _kg_incoming(g_pos, g_neg, k):
    """the incoming gradients as a gradient entry reads them: fp32, contiguous, no g_neg without negatives"""
    return g_pos.to(_F32).contiguous(), g_neg.to(_F32).contiguous() if k else None


def _kg_ent_grad(rows_src, rows_dst, rows_neg, src, dst, neg, table, sparse_grad):
    """the gradient of an entity table from its occurrences' rows, at the keys [src | dst | neg]"""
    rows, ids = [rows_src, rows_dst], [src, dst]
    if neg is not None:
        rows.append(rows_neg.reshape(-1, rows_neg.shape[2]))
        ids.append(neg.reshape(-1))
    return _table_grad(torch.cat(rows), torch.cat(ids), table.shape[0], table.dtype, sparse_grad)


def _triple_head(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize):
    """the arguments the two triple_score entries share, from prepared tensors"""
    b, k = src.numel(), (neg.shape[1] if neg is not None else 0)
    return (_stream(), _KG_KIND[kind], int(bool(normalize)), _KG_CORRUPT[corrupt],
            _ptr(ent), _DT[ent.dtype], ent.shape[0], _ptr(rel), _DT[rel.dtype], rel.shape[0],
            _ptr(src), _ptr(rel_id), _ptr(dst), _ptr(neg), b, k, ent.shape[1])


def _triple_score_raw(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize):
    """euler_gpu_triple_score on prepared tensors -> (pos [B], neg_out [B, K'])"""
    b, k, d = src.numel(), (neg.shape[1] if neg is not None else 0), ent.shape[1]
    pos, out = _kg_scores_out(b, k, corrupt, b == 0 or d == 0, ent.device)
    if b == 0 or d == 0:
        return pos, out
    with _on(ent.device):
        check(lib().euler_gpu_triple_score(*_triple_head(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize),
                                           _ptr(pos), _ptr(out) if k else None))
    return pos, out


def _triple_score_grad_raw(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize, g_pos, g_neg):
    """euler_gpu_triple_score_grad -> the fp32 gradients of the raw rows per occurrence:
    G_src, G_rel, G_dst [B, d] and G_neg [B, K, d]"""
    b, k, d = src.numel(), (neg.shape[1] if neg is not None else 0), ent.shape[1]
    make = torch.zeros if b == 0 or d == 0 else torch.empty
    gs, gr, gd = (make((b, d), dtype=_F32, device=ent.device) for _ in range(3))
    gn = make((b, k, d), dtype=_F32, device=ent.device)
    if b == 0 or d == 0:
        return gs, gr, gd, gn
    g_pos, g_neg = _kg_incoming(g_pos, g_neg, k)
    with _on(ent.device):
        check(lib().euler_gpu_triple_score_grad(
            *_triple_head(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize), _ptr(g_pos), _ptr(g_neg),
            _ptr(gs), _ptr(gr), _ptr(gd), _ptr(gn) if k else None))
    return gs, gr, gd, gn


def _table_grad(rows, ids, n_rows, dt, sparse_grad):
    """The gradient of a [n_rows, d] table from the fp32 gradient rows of its occurrences, added in
    occurrence order (scatter_add) and rounded once to the table's dtype.  An id that names no
    row becomes key -1.  sparse_grad: a sparse_coo_tensor over the distinct rows, built as
    _SparseFeatureEmbedding.backward of graph.py builds it."""
    valid = (ids >= 0) & (ids < n_rows)
    keys = torch.where(valid, ids, torch.full_like(ids, -1))
    if not sparse_grad:
        return scatter_add(rows, keys, n_rows).to(dt)
    rows, keys = rows[valid], keys[valid]
    dim = rows.shape[1]
    if keys.numel() == 0:
        return torch.sparse_coo_tensor(torch.zeros((1, 0), dtype=torch.int64, device=rows.device),
                                       torch.zeros((0, dim), dtype=dt, device=rows.device), (n_rows, dim))
    distinct, inverse = id_unique(keys)
    values = scatter_add(rows, inverse, distinct.numel()).to(dt)
    return torch.sparse_coo_tensor(distinct.reshape(1, -1), values, (n_rows, dim))


class _TripleScore(torch.autograd.Function):
    """The fused scores; the gradients of the two tables are the composition's: the kernel returns
    the gradient of every looked-up row, and scatter_add adds them at the keys
    [src | dst | neg] (ent) and rel_id (rel).  The index tensors get no gradient."""

    @staticmethod
    def forward(ctx, ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize, sparse_grad):
        ctx.save_for_backward(ent, rel, src, rel_id, dst, neg)
        ctx.conf = (kind, corrupt, normalize, sparse_grad)
        return _triple_score_raw(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize)

    @staticmethod
    def backward(ctx, g_pos, g_neg):
        ent, rel, src, rel_id, dst, neg = ctx.saved_tensors
        kind, corrupt, normalize, sparse_grad = ctx.conf
        gs, gr, gd, gn = _triple_score_grad_raw(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize,
                                                g_pos, g_neg)
        g_ent = g_rel = None
        if ctx.needs_input_grad[0]:
            g_ent = _kg_ent_grad(gs, gd, gn, src, dst, neg, ent, sparse_grad)
        if ctx.needs_input_grad[1]:
            g_rel = _table_grad(gr, rel_id, rel.shape[0], rel.dtype, sparse_grad)
        return (g_ent, g_rel) + (None,) * 8


def triple_score(ent, rel, src, rel_id, dst, neg=None, kind="trans_l1", corrupt="both", normalize=True,
                 sparse_grad=False):
    """The energies of knowledge-graph embedding in one pass (calculate_energy of the reference's
    examples/TransX/transX.py:105-133 and examples/distmult/distmult.py:99-126): the rows of src,
    dst and the [B, K] negatives in the entity table `ent` and of rel_id in the relation table
    `rel` (both [rows, d]; fp32, bf16 or fp16, each its own dtype) are looked up, l2-normalised
    (normalize; tf.nn.l2_normalize with its 1e-12 clamp) and scored, without any [B, K, d] block:
        kind "trans_l1"  -sum |a + r - c|      "trans_l2"  -sqrt(sum (a + r - c)^2)
             "distmult"   sum a * r * c
    Returns pos [B] = s(h, r, t) and neg [B, K'] - corrupt "front": s(n_k, r, t); "tail":
    s(h, r, n_k); "both": the K front scores, then the K tail scores of the same negatives
    (transX.py:130) - both fp32; pos alone when neg is None.  Ids are int64; an id outside
    [0, rows) names no row: it reads as a row of zeros and gets no gradient.  All arithmetic is
    fp32 in a fixed order (euler_amd/csrc/kg_score.h); the same call returns the same bits.
    Gradients: the kernel's per-row gradients are added at the keys [src | dst | neg] / rel_id by
    scatter_add and rounded once to the table's dtype; sparse_grad=True returns them as
    torch.sparse_coo_tensor over the distinct rows (for torch.optim.SparseAdam).  trans_l1 uses
    sign(0) = 0; trans_l2 gives a zero gradient where the norm is 0.  No host wait on the forward
    path."""
    if kind not in _KG_KIND:
        raise ValueError("triple_score: kind is trans_l1, trans_l2 or distmult")
    if corrupt not in _KG_CORRUPT:
        raise ValueError("triple_score: corrupt is front, tail or both")
    _dt("triple_score", ent)
    _dt("triple_score", rel)
    if ent.dim() != 2 or rel.dim() != 2 or ent.shape[1] != rel.shape[1] or ent.shape[0] < 1 or rel.shape[0] < 1:
        raise ValueError("triple_score: ent is [rows, d] and rel is [relations, d], one row at least")
    src, rel_id, dst, neg, b = _kg_ids("triple_score", src, rel_id, dst, neg)
    _need_cuda(ent, rel, src, rel_id, dst, *(() if neg is None else (neg,)))
    _kg_limits("triple_score", b, neg, ent.shape[0])
    pos, out = _TripleScore.apply(ent.contiguous(), rel.contiguous(), src, rel_id, dst, neg, kind, corrupt,
                                  bool(normalize), bool(sparse_grad))
    return pos if neg is None else (pos, out)


_KG_PROJ = {"hyperplane": 1, "transfer": 2}


def _triple_proj_head(proj, ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg, kind, corrupt):
    """the arguments the two triple_score_proj entries share, from prepared tensors"""
    b, k = src.numel(), (neg.shape[1] if neg is not None else 0)
    return (_stream(), _KG_PROJ[proj], _KG_KIND[kind], _KG_CORRUPT[corrupt],
            _ptr(ent), _ptr(ent_aux), _DT[ent.dtype], ent.shape[0], _ptr(rel), _ptr(rel_aux), _DT[rel.dtype],
            rel.shape[0], _ptr(src), _ptr(rel_id), _ptr(dst), _ptr(neg), b, k, ent.shape[1])


def _triple_score_proj_raw(proj, ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg, kind, corrupt):
    """euler_gpu_triple_score_proj on prepared tensors -> (pos [B], neg_out [B, K'])"""
    b, k, d = src.numel(), (neg.shape[1] if neg is not None else 0), ent.shape[1]
    pos, out = _kg_scores_out(b, k, corrupt, b == 0 or d == 0, ent.device)
    if b == 0 or d == 0:
        return pos, out
    with _on(ent.device):
        check(lib().euler_gpu_triple_score_proj(
            *_triple_proj_head(proj, ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg, kind, corrupt),
            _ptr(pos), _ptr(out) if k else None))
    return pos, out


def _triple_score_proj_grad_raw(proj, ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg, kind, corrupt, g_pos, g_neg):
    """euler_gpu_triple_score_proj_grad -> the fp32 gradients of the raw rows per occurrence:
    (G_src, G_rel, G_dst [B, d], G_neg [B, K, d], G_rel_aux [B, d], then for "transfer" G_src_aux,
    G_dst_aux [B, d] and G_neg_aux [B, K, d], else three None)"""
    b, k, d = src.numel(), (neg.shape[1] if neg is not None else 0), ent.shape[1]
    make = torch.zeros if b == 0 or d == 0 else torch.empty
    flat = lambda: make((b, d), dtype=_F32, device=ent.device)                          # noqa: E731
    block = lambda: make((b, k, d), dtype=_F32, device=ent.device)                      # noqa: E731
    gs, gr, gd, gn, gra = flat(), flat(), flat(), block(), flat()
    gsa, gda, gna = (flat(), flat(), block()) if proj == "transfer" else (None, None, None)
    if b == 0 or d == 0:
        return gs, gr, gd, gn, gra, gsa, gda, gna
    g_pos, g_neg = _kg_incoming(g_pos, g_neg, k)
    with _on(ent.device):
        check(lib().euler_gpu_triple_score_proj_grad(
            *_triple_proj_head(proj, ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg, kind, corrupt),
            _ptr(g_pos), _ptr(g_neg), _ptr(gs), _ptr(gr), _ptr(gd), _ptr(gn) if k else None, _ptr(gra),
            _ptr(gsa), _ptr(gda), _ptr(gna) if k and gna is not None else None))
    return gs, gr, gd, gn, gra, gsa, gda, gna


class _TripleScoreProj(torch.autograd.Function):
    """The fused scores with a projection; the tables' gradients are the composition's, as
    _TripleScore's: the per-occurrence rows go through _table_grad at [src | dst | neg] (ent,
    ent_transfer) and at rel_id (rel, hyper / rel_transfer).  ent_aux is None for "hyperplane"."""

    @staticmethod
    def forward(ctx, ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg, proj, kind, corrupt, sparse_grad):
        ctx.save_for_backward(ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg)
        ctx.conf = (proj, kind, corrupt, sparse_grad)
        return _triple_score_proj_raw(proj, ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg, kind, corrupt)

    @staticmethod
    def backward(ctx, g_pos, g_neg):
        ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg = ctx.saved_tensors
        proj, kind, corrupt, sparse_grad = ctx.conf
        gs, gr, gd, gn, gra, gsa, gda, gna = _triple_score_proj_grad_raw(
            proj, ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg, kind, corrupt, g_pos, g_neg)
        g_ent = _kg_ent_grad(gs, gd, gn, src, dst, neg, ent, sparse_grad) if ctx.needs_input_grad[0] else None
        g_ent_aux = _kg_ent_grad(gsa, gda, gna, src, dst, neg, ent_aux, sparse_grad) \
            if ent_aux is not None and ctx.needs_input_grad[1] else None
        g_rel = _table_grad(gr, rel_id, rel.shape[0], rel.dtype, sparse_grad) if ctx.needs_input_grad[2] else None
        g_rel_aux = _table_grad(gra, rel_id, rel_aux.shape[0], rel_aux.dtype, sparse_grad) \
            if ctx.needs_input_grad[3] else None
        return (g_ent, g_ent_aux, g_rel, g_rel_aux) + (None,) * 8


def triple_score_proj(ent, rel, src, rel_id, dst, neg=None, proj="hyperplane", hyper=None, ent_transfer=None,
                      rel_transfer=None, kind="trans_l1", corrupt="both", sparse_grad=False):
    """triple_score with the projection of TransH or TransD fused in (generate_embedding of the
    reference's examples/TransX/transH.py:43-66 and transD.py:46-73): the lookups of the extra
    tables, the projection of every entity row, the normalisations and the scores in one pass,
    without any [B, K, d] block.  N is tf.nn.l2_normalize with its 1e-12 clamp.
        proj "hyperplane" (TransH)  hyper [relations, d]: w = N(hyper[rel_id]); an entity row x is
             not normalised and becomes x - (x . w) w
        proj "transfer" (TransD)    ent_transfer [rows, d], rel_transfer [relations, d]: with
             rho = rel_transfer[rel_id] and a = ent_transfer[id] an entity row x = ent[id] becomes
             N(x + (x . a) rho)
    r = N(rel[rel_id]) in both.  kind is "trans_l1" or "trans_l2" ("distmult" takes no projection);
    corrupt, the returned pos [B] and neg [B, K'] (pos alone when neg is None) and the rule for
    ids that name no row are triple_score's.  ent_transfer has ent's dtype and rows, hyper /
    rel_transfer have rel's; each pair is fp32, bf16 or fp16.  All arithmetic is fp32 in a fixed
    order (euler_amd/csrc/kg_proj.h); the same call returns the same bits.  Gradients reach every
    table passed, as triple_score's: the kernel's per-row gradients are added at the keys
    [src | dst | neg] (ent, ent_transfer) / rel_id (rel, hyper, rel_transfer) by scatter_add and
    rounded once to the table's dtype; sparse_grad=True returns sparse_coo tensors over the
    distinct rows.  No host wait on the forward path."""
    name = "triple_score_proj"
    if proj not in _KG_PROJ:
        raise ValueError("%s: proj is hyperplane or transfer" % name)
    if kind not in ("trans_l1", "trans_l2"):
        raise ValueError("%s: kind is trans_l1 or trans_l2 (distmult takes no projection)" % name)
    if corrupt not in _KG_CORRUPT:
        raise ValueError("%s: corrupt is front, tail or both" % name)
    if proj == "hyperplane":
        if hyper is None or ent_transfer is not None or rel_transfer is not None:
            raise ValueError("%s: proj hyperplane takes hyper and neither ent_transfer nor rel_transfer" % name)
        ent_aux, rel_aux = None, hyper
    else:
        if hyper is not None or ent_transfer is None or rel_transfer is None:
            raise ValueError("%s: proj transfer takes ent_transfer and rel_transfer and no hyper" % name)
        ent_aux, rel_aux = ent_transfer, rel_transfer
    for t in (ent, rel, rel_aux) + (() if ent_aux is None else (ent_aux,)):
        _dt(name, t)
    if ent.dim() != 2 or rel.dim() != 2 or ent.shape[1] != rel.shape[1] or ent.shape[0] < 1 or rel.shape[0] < 1:
        raise ValueError("%s: ent is [rows, d] and rel is [relations, d], one row at least" % name)
    if rel_aux.shape != rel.shape or (ent_aux is not None and ent_aux.shape != ent.shape):
        raise ValueError("%s: ent_transfer has ent's shape, hyper / rel_transfer have rel's" % name)
    if rel_aux.dtype != rel.dtype or (ent_aux is not None and ent_aux.dtype != ent.dtype):
        raise TypeError("%s: ent_transfer has ent's dtype, hyper / rel_transfer have rel's" % name)
    src, rel_id, dst, neg, b = _kg_ids(name, src, rel_id, dst, neg)
    _need_cuda(ent, rel, rel_aux, src, rel_id, dst, *(() if neg is None else (neg,)),
               *(() if ent_aux is None else (ent_aux,)))
    _kg_limits(name, b, neg, ent.shape[0])
    pos, out = _TripleScoreProj.apply(ent.contiguous(), None if ent_aux is None else ent_aux.contiguous(),
                                      rel.contiguous(), rel_aux.contiguous(), src, rel_id, dst, neg, proj, kind,
                                      corrupt, bool(sparse_grad))
    return pos if neg is None else (pos, out)


KG_MATRIX_MAX_DIM = 512


def _matrix_grouping(rel_id, n_rel):
    """The grouping of euler_gpu_triple_score_matrix, with torch and without a host wait:
    -> (order [B]: the stable sort of the keys - rel_id, or n_rel where it names no relation -,
    sorted_keys [B])"""
    valid = (rel_id >= 0) & (rel_id < n_rel)
    key = torch.where(valid, rel_id, torch.full_like(rel_id, n_rel))
    sorted_keys, order = torch.sort(key, stable=True)
    return order.contiguous(), sorted_keys


def _matrix_segments(sorted_keys, n_rel, compact):
    """-> (seg_ptr [nseg + 1], seg_rel [nseg]) over the sorted keys.  Not compact: one segment a
    relation, any length may be 0 - fixed size, no host wait.  compact: the distinct relations
    used (their segments are adjacent in the order); this one waits for the host."""
    dev = sorted_keys.device
    if compact:
        seg_rel = torch.unique_consecutive(sorted_keys)
        seg_rel = seg_rel[seg_rel < n_rel].contiguous()
        edges = torch.cat([seg_rel, torch.full((1,), n_rel, dtype=torch.int64, device=dev)])
    else:
        seg_rel = torch.arange(n_rel, dtype=torch.int64, device=dev)
        edges = torch.arange(n_rel + 1, dtype=torch.int64, device=dev)
    return torch.searchsorted(sorted_keys, edges).contiguous(), seg_rel


def _triple_matrix_head(ent, rel, matrix, src, rel_id, dst, neg, kind, corrupt, order):
    """the arguments the two triple_score_matrix entries share, from prepared tensors"""
    b, k = src.numel(), (neg.shape[1] if neg is not None else 0)
    return (_stream(), _KG_KIND[kind], _KG_CORRUPT[corrupt], _ptr(ent), _DT[ent.dtype], ent.shape[0], ent.shape[1],
            _ptr(rel), _DT[rel.dtype], rel.shape[0], rel.shape[1], _ptr(matrix), _DT[matrix.dtype],
            _ptr(src), _ptr(rel_id), _ptr(dst), _ptr(neg), b, k, _ptr(order))


def _triple_score_matrix_raw(ent, rel, matrix, src, rel_id, dst, neg, kind, corrupt, order):
    """euler_gpu_triple_score_matrix on prepared tensors -> (pos [B], neg_out [B, K'])"""
    b, k = src.numel(), (neg.shape[1] if neg is not None else 0)
    empty = b == 0 or ent.shape[1] == 0 or rel.shape[1] == 0
    pos, out = _kg_scores_out(b, k, corrupt, empty, ent.device)
    if empty:
        return pos, out
    with _on(ent.device):
        check(lib().euler_gpu_triple_score_matrix(
            *_triple_matrix_head(ent, rel, matrix, src, rel_id, dst, neg, kind, corrupt, order),
            _ptr(pos), _ptr(out) if k else None))
    return pos, out


def _triple_score_matrix_grad_raw(ent, rel, matrix, src, rel_id, dst, neg, kind, corrupt, order, seg_ptr, seg_rel,
                                  g_pos, g_neg):
    """euler_gpu_triple_score_matrix_grad -> the fp32 gradients of the raw rows per occurrence
    (G_src [B, de], G_rel [B, dr], G_dst [B, de], G_neg [B, K, de]), the gz rows (gz_src, gz_dst
    [B, dr], gz_neg [B, K, dr]) and G_M [nseg, de * dr] in the matrix's dtype (None without
    segments)"""
    b, k, de, dr = src.numel(), (neg.shape[1] if neg is not None else 0), ent.shape[1], rel.shape[1]
    nseg = 0 if seg_rel is None else seg_rel.numel()
    empty = b == 0 or de == 0 or dr == 0
    make = torch.zeros if empty else torch.empty
    f = lambda *shape: make(shape, dtype=_F32, device=ent.device)                        # noqa: E731
    gs, gr, gd, gn = f(b, de), f(b, dr), f(b, de), f(b, k, de)
    zs, zd, zn = f(b, dr), f(b, dr), f(b, k, dr)
    gm = None if seg_rel is None else make((nseg, de * dr), dtype=matrix.dtype, device=ent.device)
    if empty:
        return gs, gr, gd, gn, zs, zd, zn, gm
    g_pos, g_neg = _kg_incoming(g_pos, g_neg, k)
    with _on(ent.device):
        check(lib().euler_gpu_triple_score_matrix_grad(
            *_triple_matrix_head(ent, rel, matrix, src, rel_id, dst, neg, kind, corrupt, order),
            _ptr(seg_ptr) if nseg else None, _ptr(seg_rel) if nseg else None, nseg, _ptr(g_pos), _ptr(g_neg),
            _ptr(gs), _ptr(gr), _ptr(gd), _ptr(gn) if k else None, _ptr(zs), _ptr(zd), _ptr(zn) if k else None,
            _ptr(gm) if nseg else None))
    return gs, gr, gd, gn, zs, zd, zn, gm


class _TripleScoreMatrix(torch.autograd.Function):
    """The fused scores with TransR's projection.  ent and rel take their gradients as
    _TripleScore's do: the per-occurrence rows go through _table_grad at [src | dst | neg] and at
    rel_id.  The gradient of `matrix` is the third kernel's ordered sum per relation: dense
    [R, de * dr], or with sparse_grad a sparse_coo_tensor over the distinct relations used (that
    compaction waits for the host, as _table_grad's does)."""

    @staticmethod
    def forward(ctx, ent, rel, matrix, src, rel_id, dst, neg, kind, corrupt, sparse_grad):
        order, sorted_keys = _matrix_grouping(rel_id, rel.shape[0])
        ctx.save_for_backward(ent, rel, matrix, src, rel_id, dst, neg, order, sorted_keys)
        ctx.conf = (kind, corrupt, sparse_grad)
        return _triple_score_matrix_raw(ent, rel, matrix, src, rel_id, dst, neg, kind, corrupt, order)

    @staticmethod
    def backward(ctx, g_pos, g_neg):
        ent, rel, matrix, src, rel_id, dst, neg, order, sorted_keys = ctx.saved_tensors
        kind, corrupt, sparse_grad = ctx.conf
        seg_ptr = seg_rel = None
        if ctx.needs_input_grad[2]:
            seg_ptr, seg_rel = _matrix_segments(sorted_keys, rel.shape[0], sparse_grad)
        gs, gr, gd, gn, _, _, _, gm = _triple_score_matrix_grad_raw(
            ent, rel, matrix, src, rel_id, dst, neg, kind, corrupt, order, seg_ptr, seg_rel, g_pos, g_neg)
        g_ent = g_rel = g_matrix = None
        if ctx.needs_input_grad[0]:
            g_ent = _kg_ent_grad(gs, gd, gn, src, dst, neg, ent, sparse_grad)
        if ctx.needs_input_grad[1]:
            g_rel = _table_grad(gr, rel_id, rel.shape[0], rel.dtype, sparse_grad)
        if ctx.needs_input_grad[2]:
            g_matrix = torch.sparse_coo_tensor(seg_rel.reshape(1, -1), gm, matrix.shape) if sparse_grad else gm
        return (g_ent, g_rel, g_matrix) + (None,) * 7


def triple_score_matrix(ent, rel, matrix, src, rel_id, dst, neg=None, kind="trans_l1", corrupt="both",
                        sparse_grad=False):
    """triple_score with TransR's per-relation matrix projection fused in (generate_embedding of
    the reference's examples/TransX/transR.py:41-68): ent [rows, de], rel [relations, dr] and
    matrix [relations, de * dr] (or [relations, de, dr]; row-major M_rho [de, dr]).  With
    rho = rel_id an entity row x is not normalised and becomes N(x . M_rho), r = N(rel[rho]); N is
    tf.nn.l2_normalize with its 1e-12 clamp.  The reference looks up one matrix per triple, tiles
    it over the negatives and runs a batched product: a [B, K, de * dr] block forward and backward.
    Here the triples are worked on grouped by relation (a stable sort of rel_id, built with torch,
    no host wait), a matrix is staged once per group of triples and no triple owns a matrix.
    kind is "trans_l1" or "trans_l2" ("distmult" takes no projection); corrupt, the returned
    pos [B] and neg [B, K'] (pos alone when neg is None) and the rule for ids that name no row
    are triple_score's; a rel_id that names no relation removes its rel row and its matrix.  The
    three tables are fp32, bf16 or fp16, each its own dtype; de and dr are at most 512.  All
    arithmetic is fp32 in a fixed order (euler_amd/csrc/kg_matrix.h) that does not depend on the
    batch or its grouping; the same call returns the same bits.  Gradients: ent and rel as
    triple_score's (scatter_add of the kernel's per-occurrence rows, rounded once); the matrix's
    gradient is summed per relation over its occurrences in triple order, without atomics, and
    rounded once to the matrix's dtype.  sparse_grad=True returns sparse_coo tensors over the
    distinct rows / relations for all three tables (torch.optim.SparseAdam)."""
    name = "triple_score_matrix"
    if kind not in ("trans_l1", "trans_l2"):
        raise ValueError("%s: kind is trans_l1 or trans_l2 (distmult takes no projection)" % name)
    if corrupt not in _KG_CORRUPT:
        raise ValueError("%s: corrupt is front, tail or both" % name)
    for t in (ent, rel, matrix):
        _dt(name, t)
    if ent.dim() != 2 or rel.dim() != 2 or ent.shape[0] < 1 or rel.shape[0] < 1:
        raise ValueError("%s: ent is [rows, de] and rel is [relations, dr], one row at least" % name)
    de, dr = ent.shape[1], rel.shape[1]
    if matrix.dim() not in (2, 3) or matrix.shape[0] != rel.shape[0] or \
            (tuple(matrix.shape[1:]) != (de, dr) if matrix.dim() == 3 else matrix.shape[1] != de * dr):
        raise ValueError("%s: matrix is [relations, de * dr] or [relations, de, dr]" % name)
    if de > KG_MATRIX_MAX_DIM or dr > KG_MATRIX_MAX_DIM:
        raise ValueError("%s: de and dr are at most %d" % (name, KG_MATRIX_MAX_DIM))
    if sparse_grad and matrix.dim() == 3:
        raise ValueError("%s: sparse_grad takes the matrix as [relations, de * dr]" % name)
    src, rel_id, dst, neg, b = _kg_ids(name, src, rel_id, dst, neg)
    _need_cuda(ent, rel, matrix, src, rel_id, dst, *(() if neg is None else (neg,)))
    _kg_limits(name, b, neg, ent.shape[0], rel.shape[0])
    flat = matrix.contiguous()
    if flat.dim() == 3:
        flat = flat.reshape(rel.shape[0], de * dr)
    pos, out = _TripleScoreMatrix.apply(ent.contiguous(), rel.contiguous(), flat, src, rel_id, dst, neg, kind,
                                        corrupt, bool(sparse_grad))
    return pos if neg is None else (pos, out)


# ---- the skip-gram loss head (tf_euler/python/solution/base_unsupervise.py) --------------------

def _skipgram_head(target, context, src, pos, neg):
    """the arguments the two skipgram_loss entries share, from prepared tensors"""
    return (_stream(), _ptr(target), _DT[target.dtype], target.shape[0], _ptr(context), _DT[context.dtype],
            context.shape[0], _ptr(src), _ptr(pos), _ptr(neg), src.numel(), pos.shape[1],
            neg.shape[1] if neg is not None else 0, target.shape[1])


def _skipgram_loss_raw(target, context, src, pos, neg):
    """euler_gpu_skipgram_loss on prepared tensors -> (loss [1], rank [B] int32, logits [B, P + K],
    row_loss [B])"""
    b, n, dev = src.numel(), pos.shape[1] + (neg.shape[1] if neg is not None else 0), target.device
    if b == 0:
        return (torch.zeros(1, dtype=_F32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros((0, n), dtype=_F32, device=dev), torch.zeros(0, dtype=_F32, device=dev))
    loss, row_loss = torch.empty(1, dtype=_F32, device=dev), torch.empty(b, dtype=_F32, device=dev)
    rank = torch.empty(b, dtype=torch.int32, device=dev)
    logits = torch.empty((b, n), dtype=_F32, device=dev)
    with _on(dev):
        check(lib().euler_gpu_skipgram_loss(*_skipgram_head(target, context, src, pos, neg), _ptr(logits), _ptr(rank),
                                            _ptr(row_loss), _ptr(loss)))
    return loss, rank, logits, row_loss


def _skipgram_loss_grad_raw(target, context, src, pos, neg, logits, g):
    """euler_gpu_skipgram_loss_grad -> the fp32 gradients of the raw rows per occurrence:
    G_src [B, d], G_pos [B, P, d] and G_neg [B, K, d]; g is the gradient of the loss (one element)"""
    b, p, k, d = src.numel(), pos.shape[1], (neg.shape[1] if neg is not None else 0), target.shape[1]
    make = torch.zeros if b == 0 else torch.empty
    gs = make((b, d), dtype=_F32, device=target.device)
    gp = make((b, p, d), dtype=_F32, device=target.device)
    gn = make((b, k, d), dtype=_F32, device=target.device)
    if b == 0:
        return gs, gp, gn
    g = g.to(_F32).reshape(1).contiguous()
    logits = logits.contiguous()
    with _on(target.device):
        check(lib().euler_gpu_skipgram_loss_grad(*_skipgram_head(target, context, src, pos, neg), _ptr(logits),
                                                 _ptr(g), _ptr(gs), _ptr(gp), _ptr(gn) if k else None))
    return gs, gp, gn


class _SkipgramLoss(torch.autograd.Function):
    """The fused loss head, in the shape of _TripleScore: the forward saves its logits, the kernel
    of the backward returns the gradient of every looked-up row from them, and scatter_add adds
    those rows at the keys src (target) and [pos | neg] (context).  rank and logits carry no
    gradient; the index tensors get none."""

    @staticmethod
    def forward(ctx, target, context, src, pos, neg, sparse_grad):
        loss, rank, logits, _ = _skipgram_loss_raw(target, context, src, pos, neg)
        ctx.save_for_backward(target, context, src, pos, neg, logits)
        ctx.sparse_grad = sparse_grad
        ctx.mark_non_differentiable(rank, logits)
        return loss.reshape(()), rank, logits

    @staticmethod
    def backward(ctx, g_loss, _g_rank, _g_logits):
        target, context, src, pos, neg, logits = ctx.saved_tensors
        gs, gp, gn = _skipgram_loss_grad_raw(target, context, src, pos, neg, logits, g_loss)
        d = target.shape[1]
        g_target = g_context = None
        if ctx.needs_input_grad[0]:
            g_target = _table_grad(gs, src, target.shape[0], target.dtype, ctx.sparse_grad)
        if ctx.needs_input_grad[1]:
            rows, ids = [gp.reshape(-1, d)], [pos.reshape(-1)]
            if neg is not None:
                rows.append(gn.reshape(-1, d))
                ids.append(neg.reshape(-1))
            g_context = _table_grad(torch.cat(rows), torch.cat(ids), context.shape[0], context.dtype,
                                    ctx.sparse_grad)
        return g_target, g_context, None, None, None, None


def skipgram_loss(target, context, src, pos, neg=None, sparse_grad=False, return_logits=False):
    """The loss head of the walk-based models in one pass (DeepWalk, node2vec, LINE, unsupervised
    GraphSAGE: the reference's solution/base_unsupervise.py with PosNegLogits of
    solution/logits.py:30-34, xent_loss of solution/losses.py:27-33 and the rank behind mrr_score /
    hitk_score / mr_score of utils/metrics.py:51-83).  target [Nt, d] and context [Nc, d] are the
    two embedding tables (fp32, bf16 or fp16, each its own dtype; pass the same tensor twice to
    share one table, LINE's first order); src [B], pos [B, P] (P >= 1) and neg [B, K] (or None)
    are int64 ids.  With t = target[src] the logits are x_j = t . context[pos_j] and
    t . context[neg_j]; the loss is the mean over all B * (P + K) logits of softplus(-x) of a
    positive and softplus(x) of a negative; rank [B] (int32) counts the negatives and the first
    P - 1 positives whose logit is >= the last positive's (tf.nn.top_k's tie rule on
    concat([neg, pos]): a tie goes against the positive) - rank_metric turns it into mrr, mr
    and hit@k.  Returns (loss, rank), loss a 0-d fp32 tensor, or (loss, rank, logits [B, P + K])
    with return_logits; rank and logits carry no gradient.  No [B, 1 + K, d] block, no matmul
    and no sort is built; an id outside [0, rows) names no row: it reads as a row of zeros (its
    term, ln 2, still counts) and gets no gradient.  All arithmetic is fp32 in a fixed order,
    exp and log1p included (euler_amd/csrc/skipgram.h); the same call returns the same bits.
    Gradients: the kernel's per-row gradients are added at the keys src (target) and [pos | neg]
    (context) by scatter_add and rounded once to the table's dtype; sparse_grad=True returns them
    as torch.sparse_coo_tensor over the distinct rows (for torch.optim.SparseAdam); for a shared
    table autograd adds the two.  NaN logits are outside the contract.  No host wait on the
    forward path."""
    name = "skipgram_loss"
    _dt(name, target)
    _dt(name, context)
    if target.dim() != 2 or context.dim() != 2 or target.shape[1] != context.shape[1] or target.shape[1] < 1 \
            or target.shape[0] < 1 or context.shape[0] < 1:
        raise ValueError("%s: target is [rows, d] and context is [rows, d], one row and one column at least" % name)
    src = src.to(torch.int64).reshape(-1).contiguous()
    b = src.numel()
    pos = pos.to(torch.int64)
    pos = (pos if pos.dim() == 2 else pos.reshape(b, -1)).contiguous()
    if pos.shape[0] != b or pos.shape[1] < 1:
        raise ValueError("%s: pos is [B, P], P >= 1" % name)
    if neg is not None:
        neg = neg.to(torch.int64)
        neg = (neg if neg.dim() == 2 else neg.reshape(b, -1)).contiguous()
        if neg.shape[0] != b:
            raise ValueError("%s: neg is [B, K]" % name)
        if neg.shape[1] == 0:
            neg = None
    _need_cuda(target, context, src, pos, *(() if neg is None else (neg,)))
    if b * (pos.shape[1] + (0 if neg is None else neg.shape[1])) >= 2 ** 31 or target.shape[0] >= 2 ** 31 \
            or context.shape[0] >= 2 ** 31:
        raise ValueError("%s: B * (P + K) and the tables' rows must stay below 2^31" % name)
    tc = target.contiguous()
    cc = tc if context is target else context.contiguous()
    loss, rank, logits = _SkipgramLoss.apply(tc, cc, src, pos, neg, bool(sparse_grad))
    return (loss, rank, logits) if return_logits else (loss, rank)


_RANK_METRICS = ("mrr", "mr", "hit1", "hit3", "hit10")


def rank_metric(name, rank):
    """The reference's ranking metrics from skipgram_loss's integer ranks (utils/metrics.py:51-83):
    "mrr" = mean 1 / (rank + 1), "mr" = mean rank + 1, "hit1" / "hit3" / "hit10" = the share of
    rows with rank < k.  Plain torch in float64, for logging: a 0-d tensor, no bit contract."""
    if name not in _RANK_METRICS:
        raise ValueError("rank_metric: name is one of %s" % ", ".join(_RANK_METRICS))
    r = rank.to(torch.float64)
    if name == "mrr":
        return (1.0 / (r + 1.0)).mean()
    if name == "mr":
        return (r + 1.0).mean()
    return (r < float(name[3:])).to(torch.float64).mean()


# ---- exact search over a whole table (knn/knn.py:35-77; utils/metrics.py:51-83 over every row) --

_TS_METRIC = {"ip": 0, "cos": 1, "l2": 2, "l1": 3}
_TS_MAX_K = 64


def _table_search_args(name, table, queries, metric, exclude, target=None):
    """checks and prepares what table_topk and table_rank share -> (table, queries, metric code,
    exclude | None, target | None), contiguous"""
    if metric not in _TS_METRIC:
        raise ValueError("%s: metric is one of %s" % (name, ", ".join(_TS_METRIC)))
    _dt(name, table)
    _dt(name, queries)
    if table.dim() != 2 or queries.dim() != 2 or table.shape[1] != queries.shape[1] or table.shape[1] < 1:
        raise ValueError("%s: table is [N, d] and queries is [Q, d], one column at least" % name)
    q = queries.shape[0]
    if table.shape[0] >= 2 ** 31 or q >= 2 ** 31:
        raise ValueError("%s: N and Q must stay below 2^31" % name)
    ids = []
    for what, t in (("exclude", exclude), ("target", target)):
        if t is not None:
            if t.dtype != torch.int64 or t.dim() != 1 or t.shape[0] != q:
                raise ValueError("%s: %s is [Q] int64" % (name, what))
            t = t.contiguous()
        ids.append(t)
    _need_cuda(table, queries, *[t for t in ids if t is not None])
    for t in [queries] + [t for t in ids if t is not None]:
        if t.device != table.device:
            raise ValueError("%s: every tensor must be on the table's device" % name)
    return table.detach().contiguous(), queries.detach().contiguous(), _TS_METRIC[metric], ids[0], ids[1]


def table_topk(table, queries, k, metric="ip", exclude=None, ids=None):
    """The k best rows of a whole embedding table for each query, exactly and in one pass (the
    step of the reference's knn/knn.py:35-77, which returns (distance, idx) through a faiss
    index).  table [N, d] and queries [Q, d] are fp32, bf16 or fp16, each its own dtype, widened
    exactly.  metric: "ip" = sum q_c x_c and "cos" = (ip * inv_q) * inv_x with
    inv = 1 / sqrt(max(sum x_c^2, 1e-12)) - larger is better; "l2" = sum (q_c - x_c)^2 (the
    squared distance, as faiss METRIC_L2 returns it) and "l1" = sum |q_c - x_c| (TransE's energy
    with q = h + r) - smaller is better.  Row a precedes row b iff its score is better, or b's is
    NaN and a's is not, or the two compare equal and a < b: a total order, so equal scores come out
    in row order on every run.  exclude [Q] int64 (optional) is a row the query must not return -
    its own row when the queries come from the table; a value outside [0, N) excludes nothing.
    Returns (scores [Q, k] fp32, rows [Q, k] int64), best first; past the number of candidates
    rows = -1 and scores = -inf (ip, cos) or +inf (l2, l1).  With ids ([N] int64, the node id of
    every row, as knn.py maps I through its id file) the second output is ids[rows], -1 kept.
    1 <= k <= 64.  No [Q, N] block is built: scratch is O(Q * k * slabs).  All arithmetic is fp32
    in a fixed order (euler_amd/csrc/table_search.h): a score depends on the two rows, their dtypes
    and the rows' alignment alone, never on Q, N, k or the grid, and the same call returns the same
    bits.  Forward only: the outputs carry no gradient.  No host wait."""
    name = "table_topk"
    if not isinstance(k, int) or isinstance(k, bool) or k < 1 or k > _TS_MAX_K:
        raise ValueError("%s: k is an int in 1..%d" % (name, _TS_MAX_K))
    table, queries, code, exclude, _ = _table_search_args(name, table, queries, metric, exclude)
    n, d, q, dev = table.shape[0], table.shape[1], queries.shape[0], table.device
    if ids is not None:
        if ids.dtype != torch.int64 or ids.dim() != 1 or ids.shape[0] != n or ids.device != dev:
            raise ValueError("%s: ids is [N] int64 on the table's device" % name)
    scores = torch.empty((q, k), dtype=_F32, device=dev)
    rows = torch.empty((q, k), dtype=torch.int64, device=dev)
    if q > 0:
        with _on(dev):
            check(lib().euler_gpu_table_topk(_stream(), code, _ptr(table) if n else None, _DT[table.dtype], n, d,
                                             _ptr(queries), _DT[queries.dtype], q, k, _ptr(exclude), _ptr(scores),
                                             _ptr(rows)))
    if ids is not None and n > 0:
        rows = torch.where(rows >= 0, ids[rows.clamp(min=0)], rows)
    return scores, rows


def table_rank(table, queries, target, metric="ip", exclude=None):
    """The rank of row target[q] among ALL rows of the table for each query - the evaluation
    TransE / DistMult / DeepWalk results are reported with, where skipgram_loss's rank (the
    reference's utils/metrics.py:51-83) counts sampled negatives only.  table, queries, metric
    and exclude as in table_topk; target [Q] int64.  rank[q] (int32) is the number of rows r,
    r != target[q] and r != exclude[q], whose score is better than or EQUAL to that of row
    target[q]: a tie goes against the target, as in skipgram_loss, so rank_metric applies
    unchanged (mrr, mr, hit@k).  A NaN score is never counted; a target outside [0, N) gives -1.
    The target's score comes from the same lane arithmetic as every other row's (bit-equal to the
    score table_topk returns for it).  No [Q, N] block, integer partial counts per slab of rows;
    forward only; no host wait."""
    name = "table_rank"
    if target is None:
        raise ValueError("%s: target is [Q] int64" % name)
    table, queries, code, exclude, target = _table_search_args(name, table, queries, metric, exclude, target)
    n, d, q = table.shape[0], table.shape[1], queries.shape[0]
    rank = torch.empty(q, dtype=torch.int32, device=table.device)
    if q > 0:
        with _on(table.device):
            check(lib().euler_gpu_table_rank(_stream(), code, _ptr(table) if n else None, _DT[table.dtype], n, d,
                                             _ptr(queries), _DT[queries.dtype], q, _ptr(target), _ptr(exclude),
                                             _ptr(rank)))
    return rank


# ---- the supervised loss head (tf_euler/python/mp_utils/base.py:24-47) -------------------------

_SV_SCRATCH = {}


def _supervise_scratch(device):
    """counters of a call without a metric: added to and never read, one block per device"""
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _SV_SCRATCH:
        _SV_SCRATCH[key] = torch.zeros(5, dtype=torch.int64, device=device)
    return _SV_SCRATCH[key]


def _supervise_loss_raw(logits, labels, graph, nodes, fid, counts, hist, thresholds, want_prob, want_diff):
    """euler_gpu_supervise_loss on prepared tensors -> (loss [1], prob [B, C] | None, diff [B, C] |
    None, row_loss [B]); counts [5] and hist [2, T + 1] | None (int64) are added to"""
    b, c, dev = logits.shape[0], logits.shape[1], logits.device
    loss, row_loss = torch.empty(1, dtype=_F32, device=dev), torch.empty(b, dtype=_F32, device=dev)
    prob = torch.empty((b, c), dtype=_F32, device=dev) if want_prob else None
    diff = torch.empty((b, c), dtype=_F32, device=dev) if want_diff else None
    with _on(dev):
        check(lib().euler_gpu_supervise_loss(
            _stream(), _ptr(logits), _DT[logits.dtype], b, c, _ptr(labels), _DT[labels.dtype] if labels is not None else 0,
            graph._h if graph is not None else None, _ptr(nodes), int(fid), int(thresholds), _ptr(prob), _ptr(diff),
            _ptr(row_loss), _ptr(loss), _ptr(counts), _ptr(hist)))
    return loss, prob, diff, row_loss


def _supervise_loss_grad_raw(diff, g, dtype):
    """euler_gpu_supervise_loss_grad -> the gradient of the logits [B, C] in `dtype`"""
    b, c = diff.shape
    out = torch.empty((b, c), dtype=dtype, device=diff.device)
    g = g.to(_F32).reshape(1).contiguous()
    with _on(diff.device):
        check(lib().euler_gpu_supervise_loss_grad(_stream(), _ptr(diff), _ptr(g), b, c, _ptr(out), _DT[dtype]))
    return out


class _SuperviseLoss(torch.autograd.Function):
    """The fused head: the forward keeps diff = p - z only when the logits need a gradient, and the
    backward is one kernel on it.  prob carries no gradient; the labels get none."""

    @staticmethod
    def forward(ctx, logits, labels, graph, nodes, fid, metric, return_prob):
        need = ctx.needs_input_grad[0]
        if metric is not None:
            counts, hist, t = metric._buffers(logits.device)
        else:
            counts, hist, t = _supervise_scratch(logits.device), None, 0
        loss, prob, diff, _ = _supervise_loss_raw(logits, labels, graph, nodes, fid, counts, hist, t, return_prob, need)
        if need:
            ctx.save_for_backward(diff)
        ctx.dtype = logits.dtype
        if prob is not None:
            ctx.mark_non_differentiable(prob)
        return loss.reshape(()), prob

    @staticmethod
    def backward(ctx, g_loss, _g_prob):
        diff, = ctx.saved_tensors
        return _supervise_loss_grad_raw(diff, g_loss, ctx.dtype), None, None, None, None, None, None


def _supervise_call(name, logits, labels, graph, nodes, fid, metric, return_prob):
    _dt(name, logits)
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError("%s: logits is [B, C], C >= 1" % name)
    _need_cuda(logits)
    if logits.numel() >= 2 ** 31:
        raise ValueError("%s: B * C must stay below 2^31" % name)
    if metric is not None and not hasattr(metric, "_buffers"):
        raise TypeError("%s: metric is a metrics.Streaming object (f1, acc or auc)" % name)
    loss, prob = _SuperviseLoss.apply(logits.contiguous(), labels, graph, nodes, fid, metric, bool(return_prob))
    return (loss, prob) if return_prob else loss


def supervise_loss(logits, labels, metric=None, return_prob=False):
    """The loss head of the supervised models in one pass (the reference's SuperviseModel.__call__
    after out_fc, mp_utils/base.py:24-47; SuperviseSolution; GraphModel): logits [B, C] and labels
    [B, C] (fp32, bf16 or fp16 each; soft labels allowed) -> the mean over all B * C elements of
    tf.nn.sigmoid_cross_entropy_with_logits, a 0-d fp32 tensor, or (loss, prob [B, C] fp32 =
    sigmoid(logits)) with return_prob.  metric: a metrics.Streaming object ("f1", "acc" or "auc")
    whose device counters the same kernel adds to - the prediction is floor(p + 0.5) in fp32, the
    AUC buckets are those of tf.metrics.auc's threshold table; no host wait, and metric.value() is a
    device tensor.  All arithmetic is fp32 in a fixed order (euler_amd/csrc/supervise.h): the same
    call returns the same bits.  The logits receive the gradient g / (B C) * (p - labels), rounded
    once to their dtype, from one kernel on p - labels, which the forward keeps only when the
    logits require a gradient; the labels receive none.  NaN logits are outside the contract.
    Graph.supervise_loss reads the labels straight from a graph's feature table instead."""
    name = "supervise_loss"
    _dt(name, labels)
    if labels.shape != logits.shape:
        raise ValueError("%s: labels has the shape of logits, [B, C]" % name)
    _need_cuda(labels)
    return _supervise_call(name, logits, labels.detach().contiguous(), None, None, 0, metric, return_prob)


# ---- in-place embedding stores (tf_euler/python/utils/embedding.py:24-68) ---------------------
# The stores of ScalableSageEncoder / ScalableGCNEncoder (utils/encoders.py:629-748, 294-409): a
# non-trainable [max_id + 1, d] table per layer that lives in HBM across steps and is changed IN
# PLACE - no [rows, d] temporary, no [E, d] block of per-occurrence rows.  The contract is stated
# in euler_amd/csrc/embed_store.h.  The reference sizes its stores [max_id + 2, d] and spends the
# last row as a dump for the default_node = max_id + 1 fills of the samplers; here an id outside
# [0, rows) names no row, so a store of [max_id + 1, d] drops those fills by the range rule.

def _store_table(name, table, ids):
    """checks of the table and the ids -> (ids as flat int64, E, d)"""
    if not torch.is_tensor(table) or table.dtype not in _DT:
        raise ValueError("%s: table must be float32, bfloat16 or float16" % name)
    if table.dim() != 2 or table.shape[0] < 1 or not table.is_contiguous():
        raise ValueError("%s: table is a contiguous [rows, d] tensor, one row at least (it is modified in place)"
                         % name)
    if table.requires_grad:
        raise RuntimeError("%s: table requires grad, but a store is changed in place and is not differentiable"
                           % name)
    if ids.dtype.is_floating_point or ids.dtype == torch.bool:
        raise ValueError("%s: ids are integers, not %s" % (name, ids.dtype))
    flat = ids.to(torch.int64).reshape(-1).contiguous()
    _need_cuda(table, flat)
    if flat.numel() >= 2 ** 31 or table.shape[1] >= 2 ** 31:
        raise ValueError("%s: the number of ids and d must stay below 2^31" % name)
    return flat, flat.numel(), table.shape[1]


def _store_write(name, table, ids, values, row_index, count):
    flat, e, d = _store_table(name, table, ids)
    if not torch.is_tensor(values) or values.dim() != 2 or values.shape[1] != d:
        raise ValueError("%s: values is [M, d] with the table's d" % name)
    if values.dtype != _F32 and values.dtype != table.dtype:
        raise ValueError("%s: values are float32 or of the table's dtype (%s), not %s"
                         % (name, table.dtype, values.dtype))
    if row_index is not None and count is not None:
        raise ValueError("%s: pass row_index or count, not both" % name)
    m = values.shape[0]
    if row_index is not None:
        if row_index.dtype.is_floating_point or row_index.numel() != e:
            raise ValueError("%s: row_index holds one integer per id" % name)
        row_index = row_index.to(torch.int32).reshape(-1).contiguous()
    elif count is not None:
        count = int(count)
        if count <= 0 or e % count != 0 or m != e // count:
            raise ValueError("%s: count > 0 divides the number of ids and values is [ids / count, d]" % name)
    elif m != e:
        raise ValueError("%s: values holds one row per id (or pass row_index / count)" % name)
    values = values.contiguous()
    _need_cuda(values, *(() if row_index is None else (row_index,)))
    fn = getattr(lib(), "euler_gpu_store_" + name.split("_")[1])
    with torch.no_grad(), _on(table.device):
        check(fn(_stream(), _ptr(table), _DT[table.dtype], table.shape[0], d, _ptr(flat), e, _ptr(values),
                 _DT[values.dtype], m, _ptr(row_index), count or 0))
        torch.autograd.graph.increment_version(table)
    return table


def embedding_update(table, ids, values, row_index=None, count=None):
    """embedding_update of the reference's utils/embedding.py (tf.scatter_update), IN PLACE on
    `table` ([rows, d], contiguous; fp32, bf16 or fp16): table[id] = the source row of the LAST
    occurrence of id in `ids` (any shape, flattened; the sequential loop of the CPU op).  The source
    row of occurrence p is values[p], values[row_index[p]] (one int per id; an entry outside
    [0, M) removes the occurrence) or values[p // count] (values is [E / count, d]: one row
    broadcast over the `count` sampled neighbours of a node - the [E, d] block is never built).
    values is fp32 or of the table's dtype: the same dtype copies bits, fp32 into a 16-bit table
    rounds once to nearest even.  An id outside [0, rows) names no row and is left out - a store
    sized [max_id + 1, d] so drops the default_node = max_id + 1 fills for which the reference
    keeps a dump row ([max_id + 2, d]).  Not differentiable; returns `table` (the same tensor, its
    version counter advanced).  The same call gives the same bits; no host wait."""
    return _store_write("embedding_update", table, ids, values, row_index, count)


def embedding_add(table, ids, values, row_index=None, count=None):
    """embedding_add of the reference's utils/embedding.py (tf.scatter_add), IN PLACE on `table`:
    for every distinct in-range id, acc = table[id] widened to fp32, then one correctly rounded
    fp32 add per occurrence of the id IN INPUT ORDER, then one rounding to the table's dtype - the
    bits of the reference's sequential loop, without float atomics, the same on every call.
    Arguments as embedding_update; count=fanout adds the gradient row of a node's mean / sum to
    each of its `fanout` sampled neighbours without materialising the [B * fanout, d] block.
    Not differentiable; returns `table`.  No host wait."""
    return _store_write("embedding_add", table, ids, values, row_index, count)


def embedding_take(table, ids, clear=False, out_dtype=None):
    """embedding_lookup of the reference's utils/embedding.py on a store: out[p] = table[ids[p]]
    as it was BEFORE the call, for every occurrence (duplicates included), shaped
    ids.shape + (d,), in the table's dtype or fp32 (out_dtype).  An id outside [0, rows) reads
    as a row of +0.  clear=True also sets every row an in-range id names to +0 in the same call -
    the embedding_update(gradient_store, node, zeros) under a control dependency of
    utils/encoders.py:738-743.  Not differentiable.  No host wait."""
    flat, e, d = _store_table("embedding_take", table, ids)
    od = _out_dt("embedding_take", table, out_dtype)
    shape = tuple(ids.shape) + (d,)
    if e == 0 or d == 0:
        return torch.zeros(shape, dtype=od, device=table.device)
    out = torch.empty((e, d), dtype=od, device=table.device)
    with torch.no_grad(), _on(table.device):
        check(lib().euler_gpu_store_take(_stream(), _ptr(table), _DT[table.dtype], table.shape[0], d, _ptr(flat), e,
                                         int(bool(clear)), _ptr(out), _DT[od]))
        if clear:
            torch.autograd.graph.increment_version(table)
    return out.reshape(shape)


# ---- fused sparse-row optimiser steps ------------------------------------------------------------
# One call applies one optimiser step to the table rows a list of ids names, from the gradient
# rows of the OCCURRENCES: duplicates are summed in input order inside the kernel, the table and
# its state rows change in place.  The contract is stated in euler_amd/csrc/sparse_optim.h;
# euler_amd/optim.py wraps this in torch.optim.Optimizer classes.

_ROW_STEP_KINDS = {"sgd": 0, "momentum": 1, "adagrad": 2, "adam": 3}
_ROW_STEP_STATES = {"sgd": 0, "momentum": 1, "adagrad": 1, "adam": 2}


def _storage_overlap(a, b):
    """do two contiguous tensors share bytes?"""
    if a.numel() == 0 or b.numel() == 0 or a.device != b.device:
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def sparse_row_step(kind, table, ids, grad, state=(), lr=None, momentum=0.0, eps=None, betas=(0.9, 0.999), step=1,
                    row_index=None, count=None):
    """One optimiser step - kind "sgd", "momentum", "adagrad" or "adam", the four of the
    reference's utils/optimizers.py - IN PLACE on the rows of `table` ([rows, d], contiguous; fp32,
    bf16 or fp16; a leaf that requires grad is accepted: a parameter is one) that `ids` names.
    `grad` holds the gradient rows of the occurrences, in the three forms of embedding_add: grad[p],
    grad[row_index[p]] or grad[p // count]; fp32 or of the table's dtype.  Per distinct in-range id
    the rows of its occurrences are summed IN INPUT ORDER in fp32 (no coalesce, no float atomics),
    then the step runs in correctly rounded fp32 operations and the row is rounded once:
      sgd       p -= lr * g                                     state ()
      momentum  a = momentum * a + g;  p -= lr * a              state (a,)      touched rows only
      adagrad   s += g * g;  p -= lr * g / (sqrt(s) + eps)      state (s,)      eps default 1e-10
      adam      m += (g - m) * (1 - beta1);  v += (g * g - v) * (1 - beta2);
                p -= lr * sqrt(1 - beta2^step) / (1 - beta1^step) * m / (sqrt(v) + eps)
                                                                state (m, v)    eps default 1e-8
    (adam is lazy: torch.optim.SparseAdam's formula).  `state` tensors are fp32, contiguous, of the
    table's shape, modified in place, and share no storage with the table or grad.  The scalars
    are computed here in double and rounded once to fp32; `step` (>= 1) is the caller's count.
    Rows no live id names keep their bits.  Returns `table`; the version counters of the table and
    of every state tensor advance.  The same call gives the same bits; no host wait."""
    name = "sparse_row_step"
    if kind not in _ROW_STEP_KINDS:
        raise ValueError("%s: kind is one of %s, not %r" % (name, ", ".join(_ROW_STEP_KINDS), kind))
    if not torch.is_tensor(table) or table.dtype not in _DT:
        raise ValueError("%s: table must be float32, bfloat16 or float16" % name)
    if table.dim() != 2 or table.shape[0] < 1 or not table.is_contiguous():
        raise ValueError("%s: table is a contiguous [rows, d] tensor, one row at least (it is modified in place)" % name)
    if table.requires_grad and not table.is_leaf:
        raise RuntimeError("%s: table is not a leaf: only a parameter (or a tensor without grad) is stepped in place"
                           % name)
    if ids.dtype.is_floating_point or ids.dtype == torch.bool:
        raise ValueError("%s: ids are integers, not %s" % (name, ids.dtype))
    flat = ids.to(torch.int64).reshape(-1).contiguous()
    e, d = flat.numel(), table.shape[1]
    if e >= 2 ** 31 or d >= 2 ** 31:
        raise ValueError("%s: the number of ids and d must stay below 2^31" % name)
    if not torch.is_tensor(grad) or grad.dim() != 2 or grad.shape[1] != d:
        raise ValueError("%s: grad is [M, d] with the table's d" % name)
    if grad.dtype != _F32 and grad.dtype != table.dtype:
        raise ValueError("%s: grad is float32 or of the table's dtype (%s), not %s" % (name, table.dtype, grad.dtype))
    if row_index is not None and count is not None:
        raise ValueError("%s: pass row_index or count, not both" % name)
    m = grad.shape[0]
    if row_index is not None:
        if row_index.dtype.is_floating_point or row_index.numel() != e:
            raise ValueError("%s: row_index holds one integer per id" % name)
        row_index = row_index.to(torch.int32).reshape(-1).contiguous()
    elif count is not None:
        count = int(count)
        if count <= 0 or e % count != 0 or m != e // count:
            raise ValueError("%s: count > 0 divides the number of ids and grad is [ids / count, d]" % name)
    elif m != e:
        raise ValueError("%s: grad holds one row per id (or pass row_index / count)" % name)
    grad = grad.detach().contiguous()
    state = tuple(state)
    if len(state) != _ROW_STEP_STATES[kind]:
        raise ValueError("%s: %s takes %d state tensor(s), not %d" % (name, kind, _ROW_STEP_STATES[kind], len(state)))
    for n, s in enumerate(state):
        if not torch.is_tensor(s) or s.dtype != _F32 or s.shape != table.shape:
            raise ValueError("%s: state[%d] is a float32 tensor of the table's shape" % (name, n))
        if not s.is_contiguous():
            raise ValueError("%s: state[%d] is not contiguous (it is modified in place)" % (name, n))
        if s.requires_grad:
            raise RuntimeError("%s: state[%d] requires grad" % (name, n))
        if _storage_overlap(s, table) or _storage_overlap(s, grad) or any(_storage_overlap(s, o) for o in state[:n]):
            raise ValueError("%s: state[%d] shares storage with the table, grad or another state tensor" % (name, n))
    _need_cuda(table, flat, grad, *state, *(() if row_index is None else (row_index,)))
    if lr is None:
        raise ValueError("%s: lr is required" % name)
    if eps is None:
        eps = {"adagrad": 1e-10, "adam": 1e-8}.get(kind, 0.0)
    beta1, beta2 = betas
    step = int(step)
    if step < 1 or not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
        raise ValueError("%s: step >= 1 and betas in [0, 1)" % name)
    scalars = (float(lr), float(momentum), float(eps), 1.0 - beta1, 1.0 - beta2,
               float(lr) * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step))
    if not all(np.isfinite(x) and x >= 0 for x in scalars):
        raise ValueError("%s: lr, momentum and eps are finite and not negative" % name)
    with torch.no_grad(), _on(table.device):
        check(lib().euler_gpu_sparse_optim_step(
            _stream(), _ROW_STEP_KINDS[kind], _ptr(table), _DT[table.dtype], table.shape[0], d,
            _ptr(state[0]) if len(state) > 0 else None, _ptr(state[1]) if len(state) > 1 else None, _ptr(flat), e,
            _ptr(grad), _DT[grad.dtype], m, _ptr(row_index), count or 0, *scalars))
        torch.autograd.graph.increment_version(table)
        for s in state:
            torch.autograd.graph.increment_version(s)
    return table


def scatter_softmax(updates, indices, size, out_dtype=None):
    """mp_ops.py:76-79.  16-bit updates: the fp32 softmax of updates.float(), rounded once at the end
    unless out_dtype is torch.float32 (and its gradient once on the way back)."""
    if updates.dtype == _F32:
        _out_dt("scatter_softmax", updates, out_dtype)
        updates = updates - gather(scatter_max(updates, indices, size), indices)
        updates = torch.exp(updates)
        return updates / gather(scatter_add(updates, indices, size), indices)
    _dt("scatter_softmax", updates)
    od = _out_dt("scatter_softmax", updates, out_dtype)
    return scatter_softmax(updates.float(), indices, size).to(od)


def scatter_(op, updates, indices, size, out_dtype=None):
    """mp_ops.py:72-73."""
    return {"add": scatter_add, "max": scatter_max, "mean": scatter_mean,
            "softmax": scatter_softmax}[op](updates, indices, size, out_dtype=out_dtype)


def gen_pair(paths, left_win_size, right_win_size):
    """GenPair (tf_euler/kernels/gen_pair_op.cc): [batch, path_len] int64 ->
    [batch, pair_count, 2]."""
    paths = paths.to(torch.int64).contiguous()
    _need_cuda(paths)
    b, l = paths.shape
    pc = lib().euler_gpu_gen_pair_count(l, left_win_size, right_win_size)
    out = torch.empty((b, pc, 2), dtype=torch.int64, device=paths.device)
    with _on(paths.device):
        check(lib().euler_gpu_gen_pair(_stream(), _ptr(paths), b, l, left_win_size,
                                       right_win_size, _ptr(out)))
    return out


def node2vec_step(seed, call_id, c_row, c_idx, c_ids, c_w, p_row, p_idx, p_ids, parent_ids,
                  p, q, default_node=-1):
    """One node2vec step over explicit neighbour lists (euler_gpu_node2vec_step;
    tf_euler/kernels/random_walk_op.cc:83-168): walker i's child list is row c_row[i] of
    (c_idx [rows, 2], c_ids, c_w), its parent's list row p_row[i] of (p_idx, p_ids) -
    p_row None on the first step.  Returns the next nodes [n] int64."""
    c_row = c_row.to(torch.int32).contiguous()
    c_idx = c_idx.to(torch.int32).contiguous()
    c_ids = c_ids.to(torch.int64).contiguous()
    c_w = c_w.to(torch.float32).contiguous()
    parent_ids = parent_ids.to(torch.int64).contiguous()
    _need_cuda(c_row, c_idx, c_ids, c_w, parent_ids)
    if p_row is not None:
        p_row = p_row.to(torch.int32).contiguous()
        p_idx = p_idx.to(torch.int32).contiguous()
        p_ids = p_ids.to(torch.int64).contiguous()
        _need_cuda(p_row, p_idx, p_ids)
    n = c_row.numel()
    out = torch.empty(n, dtype=torch.int64, device=c_row.device)
    null = C.c_void_p(0)
    with _on(c_row.device):
        check(lib().euler_gpu_node2vec_step(
            _stream(), int(seed), int(call_id), n, _ptr(c_row), _ptr(c_idx), _ptr(c_ids), _ptr(c_w),
            int(c_w.numel()),
            _ptr(p_row) if p_row is not None else null,
            _ptr(p_idx) if p_row is not None else null,
            _ptr(p_ids) if p_row is not None else null,
            _ptr(parent_ids), float(p), float(q), int(default_node), _ptr(out)))
    return out


def id_unique(ids):
    """ID_UNIQUE: (unique ids in first-occurrence order, gather_idx int32)."""
    ids = ids.to(torch.int64).contiguous().reshape(-1)
    _need_cuda(ids)
    n = ids.numel()
    uq = torch.empty(n, dtype=torch.int64, device=ids.device)
    gi = torch.empty(n, dtype=torch.int32, device=ids.device)
    nu = C.c_int64(0)
    with _on(ids.device):
        check(lib().euler_gpu_id_unique(_stream(), _ptr(ids), n, _ptr(uq), _ptr(gi),
                                        C.byref(nu)))
    return uq[:nu.value], gi


def idx_gather(idx, gather_idx):
    """IDX_GATHER: re-based [n,2] offsets of the gathered segments."""
    idx = idx.to(torch.int32).contiguous()
    gi = gather_idx.to(torch.int32).contiguous()
    _need_cuda(idx, gi)
    n = gi.numel()
    out = torch.empty((n, 2), dtype=torch.int32, device=idx.device)
    total = C.c_int64(0)
    with _on(idx.device):
        check(lib().euler_gpu_idx_gather(_stream(), _ptr(idx), _ptr(gi), n,
                                         _ptr(out), C.byref(total)))
    return out, int(total.value)


def data_gather(data, idx, gather_idx):
    """DATA_GATHER: concatenated segments data[idx[g]] for g in gather_idx."""
    data = data.contiguous()
    idx = idx.to(torch.int32).contiguous()
    gi = gather_idx.to(torch.int32).contiguous()
    _need_cuda(data, idx, gi)
    out_idx, total = idx_gather(idx, gi)
    out = torch.empty(total, dtype=data.dtype, device=data.device)
    with _on(data.device):
        check(lib().euler_gpu_data_gather(_stream(), _ptr(data), data.element_size(),
                                          _ptr(idx), _ptr(gi), _ptr(out_idx),
                                          gi.numel(), _ptr(out)))
    return out


def sparse_gather(gather_idx, indices, values, dense_shape):
    """tf_euler sparse_gather (tf_euler/kernels/sparse_gather_op.cc:32-240, op
    tf_euler/ops/util_ops.cc:37-55): `gather` on a SparseTensor whose entries are sorted by row.
    Row g of the result = row gather_idx[g] of the input: its entries in order, first index
    column rewritten to g, the other columns and the values copied; dense_shape[0] = len(
    gather_idx).  Returns (out_indices [nnz', cols] int64, out_values, out_dense_shape).  The
    rows' extents come from a binary search of the first index column (the reference's
    GatherWithBinarySearch; its GatherWithIndex branch answers the same on inputs where every
    gathered row has an entry - what get_sparse_feature produces: it inserts a default entry
    for empty rows), the copies are the DATA_GATHER kernel's.  A row without entries gathers
    nothing; an index >= dense_shape[0] raises IndexError as the reference's InvalidArgument."""
    gi = gather_idx.reshape(-1).to(torch.int64)
    indices = indices.to(torch.int64).contiguous()
    _need_cuda(indices, values)
    if indices.dim() != 2 or values.dim() != 1 or values.numel() != indices.shape[0]:
        raise ValueError("sparse_gather: indices [nnz, cols] and values [nnz]")
    shape = [int(x) for x in (dense_shape.tolist() if hasattr(dense_shape, "tolist") else dense_shape)]
    if len(shape) != indices.shape[1]:
        raise ValueError("sparse_gather: dense_shape and indices shape mismatch")
    rows = shape[0]
    if gi.numel() and (int(gi.max()) >= rows or int(gi.min()) < 0):
        raise IndexError("sparse_gather: gather idx out of range")
    dev = indices.device
    col0 = indices[:, 0].contiguous()
    bounds = torch.searchsorted(col0, torch.arange(rows + 1, device=dev, dtype=torch.int64))
    idx = torch.stack([bounds[:-1], bounds[1:]], dim=1).to(torch.int32)
    g32 = gi.to(torch.int32).to(dev)
    out_values = data_gather(values, idx, g32)
    lens = (idx[:, 1] - idx[:, 0]).to(torch.int64)[gi.to(dev)]
    cols = [torch.repeat_interleave(torch.arange(gi.numel(), device=dev, dtype=torch.int64), lens)]
    for k in range(1, indices.shape[1]):
        cols.append(data_gather(indices[:, k].contiguous(), idx, g32))
    out_indices = torch.stack(cols, dim=1) if out_values.numel() else \
        torch.empty((0, indices.shape[1]), dtype=torch.int64, device=dev)
    out_shape = torch.tensor([gi.numel()] + shape[1:], dtype=torch.int64)
    return out_indices, out_values, out_shape


def inflate_idx(idx):
    """tf_euler inflate_idx (tf_euler/kernels/inflate_idx_op.cc:34-66, op tf_euler/ops/util_ops.cc):
    idx is a 1-D int32 vector whose values are exactly 0 .. U-1; out[i] = the place of entry i
    after a stable sort by value.  A value outside [0, number of distinct values) raises
    ValueError (the reference's InvalidArgument), a non-vector too."""
    if idx.dim() != 1:
        raise ValueError("InflateIdx expects a 1-D vector.")
    if idx.dtype != torch.int32 and idx.numel():
        # before the narrowing: a value such as 2^32 + 1 would wrap into range and be answered.
        # The number of distinct values is at most numel(), so this refuses nothing valid.
        lo, hi = torch.aminmax(idx)
        if int(lo) < 0 or int(hi) >= idx.numel():
            raise ValueError("InflateIdx: expect input idx in [0,unique_cnt).")
    idx = idx.to(torch.int32).contiguous()
    _need_cuda(idx)
    out = torch.empty_like(idx)
    with _on(idx.device):
        rc = lib().euler_gpu_inflate_idx(_stream(), _ptr(idx), idx.numel(), _ptr(out))
    if rc == -1:
        raise ValueError("InflateIdx: expect input idx in [0,unique_cnt).")
    check(rc)
    return out


def id_split(ids, partitions, shards):
    """ID_SPLIT: stable bucket by owner(id) = (id % partitions) % shards.
    Returns (shard_off list[shards+1], shard_ids int64 [n], merge_idx int32 [n])."""
    ids = ids.to(torch.int64).contiguous().reshape(-1)
    _need_cuda(ids)
    n = ids.numel()
    off = (C.c_int64 * (shards + 1))()
    sid = torch.empty(n, dtype=torch.int64, device=ids.device)
    mi = torch.empty(n, dtype=torch.int32, device=ids.device)
    with _on(ids.device):
        check(lib().euler_gpu_id_split(_stream(), _ptr(ids), n, partitions, shards,
                                       off, _ptr(sid), _ptr(mi)))
    return list(off), sid, mi


def _root_mask_arg(name, root_mask, n, root_group):
    """root_mask as contiguous uint8, with a byte for every group of n positions: the kernels
    index it by position // group and do not know its length"""
    if root_mask is None:
        return None
    root_mask = root_mask.to(torch.uint8).contiguous()
    _need_cuda(root_mask)
    group = max(int(root_group), 1)
    need = (n + group - 1) // group
    if root_mask.numel() < need:
        raise ValueError("%s: root_mask has %d elements, %d positions in groups of %d need %d"
                         % (name, root_mask.numel(), n, group, need))
    return root_mask


def dedup_split(ids, partitions, shards, root_mask=None, root_group=1, dense_table=None):
    """Distinct ids bucketed by owner + the bucketed index of every position
    (ID_UNIQUE + ID_SPLIT in one call, one host sync).  Returns (shard_off
    list[shards+1], shard_ids int64 [m], pos int32 [n]) with m = shard_off[-1] <= n.
    root_mask ([ceil(n / root_group)] uint8): marked groups count as id 0.
    dense_table (optional int32 [limit + 1] scratch kept by the caller, contents
    irrelevant): every id of the graph is < limit, so duplicates are found in a
    table indexed by the id itself instead of by hashing."""
    ids = ids.to(torch.int64).contiguous().reshape(-1)
    _need_cuda(ids)
    n = ids.numel()
    root_mask = _root_mask_arg("dedup_split", root_mask, n, root_group)
    limit = 0
    if dense_table is not None:
        _need_cuda(dense_table)
        assert dense_table.dtype == torch.int32 and dense_table.is_contiguous()
        limit = dense_table.numel() - 1
    off = (C.c_int64 * (shards + 1))()
    sid = torch.empty(n, dtype=torch.int64, device=ids.device)
    pos = torch.empty(n, dtype=torch.int32, device=ids.device)
    with _on(ids.device):
        check(lib().euler_gpu_dedup_split(_stream(), _ptr(ids), n, _ptr(root_mask),
                                          int(root_group), partitions, shards,
                                          _ptr(dense_table), limit, off, _ptr(sid),
                                          _ptr(pos)))
    off = list(off)
    return off, sid[:off[-1]], pos


class FrontHandle(object):
    """One dedup_split call in flight (euler_gpu_front): begin() enqueues the
    front end and returns, end() waits for the bucket sizes only."""

    def __init__(self):
        h = C.c_void_p()
        check(lib().euler_gpu_front_create(C.byref(h)))
        self._h = h
        self._token = None

    def begin(self, ids, partitions, shards, root_mask=None, root_group=1, dense_table=None):
        ids = ids.to(torch.int64).contiguous().reshape(-1)
        _need_cuda(ids)
        n = ids.numel()
        root_mask = _root_mask_arg("FrontHandle.begin", root_mask, n, root_group)
        limit = dense_table.numel() - 1 if dense_table is not None else 0
        sid = torch.empty(n, dtype=torch.int64, device=ids.device)
        pos = torch.empty(n, dtype=torch.int32, device=ids.device)
        with _on(ids.device):
            check(lib().euler_gpu_dedup_split_begin(
                self._h, _stream(), _ptr(ids), n, _ptr(root_mask), int(root_group), partitions,
                shards, _ptr(dense_table), limit, _ptr(sid), _ptr(pos)))
        # the inputs must outlive the enqueued kernels: keep them with the token
        self._token = (shards, sid, pos, ids, root_mask)
        return self

    def end(self):
        shards, sid, pos, _ids, _mask = self._token
        self._token = None
        off = (C.c_int64 * (shards + 1))()
        check(lib().euler_gpu_dedup_split_end(self._h, off))
        off = list(off)
        return off, sid[:off[-1]], pos

    def __del__(self):
        try:
            if self._h is not None and self._h.value:
                lib().euler_gpu_front_destroy(self._h)
                self._h = None
        except Exception:
            pass


def expand_rows(pos, ids, w, t, mask, count):
    """Row pos[i] of the sampled rows of the distinct roots -> position i:
    (ids [n,count] int64, w f32, t int32, mask [n] uint8)."""
    pos = pos.to(torch.int32).contiguous()
    ids = ids.contiguous(); w = w.contiguous(); t = t.contiguous()
    mask = mask.to(torch.uint8).contiguous()
    _need_cuda(pos, ids, w, t, mask)
    n = pos.numel()
    dev = pos.device
    o_id = torch.empty((n, count), dtype=torch.int64, device=dev)
    o_w = torch.empty((n, count), dtype=torch.float32, device=dev)
    o_t = torch.empty((n, count), dtype=torch.int32, device=dev)
    o_m = torch.empty(n, dtype=torch.uint8, device=dev)
    with _on(dev):
        check(lib().euler_gpu_expand_rows(_stream(), _ptr(pos), n, int(count), _ptr(ids),
                                          _ptr(w), _ptr(t), _ptr(mask), _ptr(o_id),
                                          _ptr(o_w), _ptr(o_t), _ptr(o_m)))
    return o_id, o_w, o_t, o_m


def packed_words(count, single_type=None):
    """int32 words per wire row: ids (2 each) | weights | [types] | mask, pad."""
    return ((3 if single_type is not None else 4) * int(count) + 2 + 1) & ~1     # even: 8-byte rows


def pack_rows(ids, w, t, mask, count, single_type=None):
    """Sampler outputs [m, count] (+ mask [m]) -> wire rows [m, packed_words] int32.
    single_type (the one listed edge type of the call): the type column is left
    off the wire."""
    ids = ids.contiguous(); w = w.contiguous(); t = t.contiguous()
    mask = mask.to(torch.uint8).contiguous()
    _need_cuda(ids, w, t, mask)
    m = mask.numel()
    out = torch.empty((m, packed_words(count, single_type)), dtype=torch.int32,
                      device=ids.device)
    with _on(ids.device):
        check(lib().euler_gpu_pack_rows(_stream(), _ptr(ids), _ptr(w), _ptr(t),
                                        _ptr(mask), m, int(count),
                                        -1 if single_type is None else int(single_type),
                                        _ptr(out)))
    return out


def expand_packed(pos, packed, count, single_type=None):
    """Wire rows -> (ids [n,count] int64, w f32, t int32, mask [n] uint8) per
    position: row pos[i] of `packed` is position i's row."""
    pos = pos.to(torch.int32).contiguous()
    packed = packed.contiguous()
    _need_cuda(pos, packed)
    assert packed.shape[-1] == packed_words(count, single_type), "wire row width"
    n = pos.numel()
    dev = pos.device
    o_id = torch.empty((n, count), dtype=torch.int64, device=dev)
    o_w = torch.empty((n, count), dtype=torch.float32, device=dev)
    o_t = torch.empty((n, count), dtype=torch.int32, device=dev)
    o_m = torch.empty(n, dtype=torch.uint8, device=dev)
    with _on(dev):
        check(lib().euler_gpu_expand_packed(_stream(), _ptr(pos), n, int(count),
                                            -1 if single_type is None else int(single_type),
                                            _ptr(packed), _ptr(o_id), _ptr(o_w),
                                            _ptr(o_t), _ptr(o_m)))
    return o_id, o_w, o_t, o_m


def merge_rows(rows, merge_idx, n_rows=None):
    """IDX_MERGE / DATA_MERGE for fixed-size rows: out[merge_idx[j]] = rows[j]."""
    rows = rows.contiguous()
    mi = merge_idx.to(torch.int32).contiguous()
    _need_cuda(rows, mi)
    n = mi.numel()
    out = torch.empty_like(rows) if n_rows is None else torch.empty(
        (n_rows,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    row_bytes = rows.element_size() * (rows.numel() // max(n, 1)) if n else 4
    with _on(rows.device):
        check(lib().euler_gpu_merge_rows(_stream(), _ptr(rows), _ptr(mi), n,
                                         row_bytes, _ptr(out)))
    return out


def sample_node_split(seed, call_id, count, shard_weight):
    """SAMPLE_NODE_SPLIT (host): per-shard counts proportional to the shards'
    type weight sums; shard_weight has shards+1 entries (last = total)."""
    sw = np.ascontiguousarray(shard_weight, dtype=np.float32)
    shards = len(sw) - 1
    out = np.zeros(shards, np.int32)
    check(lib().euler_gpu_sample_node_split(
        seed, call_id, count, sw.ctypes.data_as(_lib.f32p), shards,
        out.ctypes.data_as(_lib.i32p)))
    return out
