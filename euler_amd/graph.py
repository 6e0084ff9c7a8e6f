"""Device-resident Euler graph + the sampling / message-passing operators on it.

Host-side mirror of what the reference reaches through
`QueryProxy::RunAsyncGremlin` for the hot path (tf_euler/kernels/*.cc): every
method enqueues hand-written HIP kernels of libeuler_gpu.so on the current
torch stream and returns torch tensors living in HBM.  torch is plumbing here
(device memory, streams); the computation is in euler_amd/csrc.
"""
import contextlib
import ctypes as C
import math
import threading

import numpy as np
import torch

from . import _lib
from ._lib import check, lib

_I32 = C.POINTER(C.c_int32)


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """The current HIP stream of the current device as a pointer (torch.cuda.current_stream()
    builds a Stream object for it: 8 us a call, a quarter of a small op's enqueue cost)."""
    if _RAW_STREAM is not None:
        return C.c_void_p(_RAW_STREAM(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


_NULL_CTX = contextlib.nullcontext()


_I32_CACHE = {}
_FANOUT_PLANS = {}
_WS_BYTES = {}


def _fanout_plan(edge_types, counts):
    """(edge types [layers, k] as int32 array, its pointer, k, counts array, its pointer) of a
    fanout call; cached for list arguments (a training loop passes the same ones every step)."""
    key = None
    try:
        key = (tuple(tuple(int(t) for t in row) for row in edge_types), tuple(int(c) for c in counts))
        hit = _FANOUT_PLANS.get(key)
        if hit is not None:
            return hit
    except TypeError:
        key = None
    layers = len(counts)
    et = np.ascontiguousarray(np.asarray(edge_types, dtype=np.int32).reshape(layers, -1)) if layers \
        else np.zeros((0, 0), np.int32)
    cnt = np.ascontiguousarray(np.asarray(counts, dtype=np.int32).reshape(-1))
    res = (et, et.ctypes.data_as(_I32), int(et.size // layers) if layers else 0, cnt, cnt.ctypes.data_as(_I32))
    if key is not None and len(_FANOUT_PLANS) < 1024:
        et.flags.writeable = False      # shared by every later call with these arguments
        cnt.flags.writeable = False
        _FANOUT_PLANS[key] = res
    return res


def _i32_array(values):
    """(array, int32*, size) of a list of small ints (edge types, counts); flat lists are
    cached - the same few lists come back every minibatch."""
    key = None
    if type(values) in (list, tuple) and len(values) <= 32 and all(type(v) is int for v in values):
        key = tuple(values)
        hit = _I32_CACHE.get(key)
        if hit is not None:
            return hit
    a = np.ascontiguousarray(np.asarray(values, dtype=np.int32).reshape(-1))
    res = (a, a.ctypes.data_as(_I32), int(a.size))
    if key is not None and len(_I32_CACHE) < 1024:
        a.flags.writeable = False       # shared by every later call with this list
        _I32_CACHE[key] = res
    return res


def _read_counts(counts):
    """A few device-side counts as Python ints.  Tensor.cpu() is the cheapest way measured
    (profiles/r4_ab_count_read.txt: a pinned buffer + stream / event synchronize costs the
    same or more; what the read costs is the drain of the stream, ~55 us, not the copy)."""
    return [int(c) for c in counts.cpu().tolist()]


def _as_i64_cuda(x, device):
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x).astype(np.int64, copy=False))
    if x.dtype != torch.int64:
        x = x.to(torch.int64)
    return x.to(device).contiguous()


def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def synth_params(seed, n_nodes, n_edges, n_types=1, weighted=True, scale=None, hashed_ids=False):
    """Parameters of the deterministic synthetic power-law graph (RMAT
    marginals a,b,c,d = .57,.19,.19,.05, minimum degree 1).
    deg_table[z] = expected extra out-degree of a node whose (id-1) has z one
    bits, normalised so the edge total is n_edges."""
    if scale is None:
        scale = max(1, int(math.ceil(math.log2(max(n_nodes, 2)))))
    # number of x in [0, n_nodes) with popcount(x & mask) == z, by digit DP
    cnt = [0] * 65
    mask_bits = scale
    hi = n_nodes >> mask_bits           # full cycles of the low `scale` bits
    lo = n_nodes & ((1 << mask_bits) - 1)
    if hi:
        for z in range(mask_bits + 1):
            cnt[z] += hi * math.comb(mask_bits, z)
    ones = 0
    for b in range(mask_bits - 1, -1, -1):
        if (lo >> b) & 1:
            for z in range(b + 1):
                cnt[ones + z] += math.comb(b, z)
            ones += 1
    p = _lib.SynthParams()
    p.seed = seed
    p.n_nodes = n_nodes
    p.n_edges_target = n_edges
    p.scale = scale
    p.n_types = n_types
    p.weighted = 1 if weighted else 0
    # hashed_ids: node x is known outside by mix64(x) (arbitrary u64 ids, hash id map) - what a
    # dataset converted by euler/tools looks like - instead of x itself (identity id map)
    p.hashed_ids = 1 if hashed_ids else 0
    wz = [(0.76 ** (scale - z)) * (0.24 ** z) for z in range(scale + 1)]
    norm = sum(c * w for c, w in zip(cnt, wz))
    extra = max(0.0, float(n_edges - n_nodes))
    for z in range(64):
        p.deg_table[z] = extra * wz[z] / norm if (z <= scale and norm > 0) else 0.0
    return p


def _edge_feature_tables(e, n, dense, sparse, binary):
    """Fill the feature tables of a HostEdges; returns the arrays it points into (keep them alive
    for the call)."""
    keep = []

    def table(slots, vtype, vptr):
        if all(isinstance(c, np.ndarray) and c.ndim == 2 and len(c) == n for c in slots):
            # every record has the same slot layout: the library stores one row of ends
            lens = np.array([c.shape[1] for c in slots], np.int64)
            ends = np.tile(np.cumsum(lens).astype(np.int32), n)
            ptr = np.arange(n + 1, dtype=np.int64) * int(lens.sum())
            if len(slots) == 1:
                val = np.ascontiguousarray(slots[0], vtype).reshape(-1)
            else:
                val = np.ascontiguousarray(np.concatenate([c.astype(vtype) for c in slots], 1)).reshape(-1)
        else:
            if vtype == np.uint8:
                slots = [[np.frombuffer(bytes(b), np.uint8) for b in c] for c in slots]
            lens = np.stack([np.array([len(x) for x in c], np.int64) for c in slots], 1)
            ends = np.cumsum(lens, 1).astype(np.int32).reshape(-1)
            ptr = np.zeros(n + 1, np.int64)
            ptr[1:] = np.cumsum(lens.sum(1))
            vals = [np.asarray(c[r], vtype).reshape(-1) for r in range(n) for c in slots]
            val = np.concatenate(vals) if vals else np.zeros(0, vtype)
        if len(val) == 0:
            val = np.zeros(1, vtype)
        keep.extend([ptr, ends, val])
        return (ptr.ctypes.data_as(_lib.i64p), ends.ctypes.data_as(_lib.i32p),
                val.ctypes.data_as(vptr))

    if dense:
        e.n_float_features = len(dense)
        e.feat_ptr, e.feat_idx, e.feat_val = table(list(dense), np.float32, _lib.f32p)
    if sparse:
        e.n_u64_features = len(sparse)
        e.ufeat_ptr, e.ufeat_idx, e.ufeat_val = table(list(sparse), np.uint64, _lib.u64p)
    if binary:
        e.n_binary_features = len(binary)
        e.bfeat_ptr, e.bfeat_idx, e.bfeat_val = table(list(binary), np.uint8, _lib.u8p)
    return keep



def dat_feature_info(data_path, name, edge=False):
    """euler.meta's (type, slot, dim) for the feature `name` exactly as written there."""
    t, slot, dim = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    check(lib().euler_gpu_dat_feature_info(str(data_path).encode(), 1 if edge else 0,
                                           str(name).encode(), C.byref(t), C.byref(slot),
                                           C.byref(dim)))
    return int(t.value), int(slot.value), int(dim.value)


def _label_triple(idx, ids):
    """SparseTensorBuilder's triple of a get_graph_by_label result
    (tf_euler/kernels/get_graph_by_label_op.cc): a label with no nodes emits (i, 0) = 0."""
    dev = ids.device
    b = idx.shape[0]
    if b == 0:
        return (torch.zeros((0, 2), dtype=torch.int64, device=dev),
                torch.zeros(0, dtype=torch.int64, device=dev), [0, 0])
    lens = (idx[:, 1] - idx[:, 0]).to(torch.int64)
    slots = torch.clamp(lens, min=1)
    nnz = int(slots.sum().item())
    row = torch.repeat_interleave(torch.arange(b, device=dev), slots, output_size=nnz)
    first = torch.cumsum(slots, 0) - slots
    col = torch.arange(nnz, device=dev) - first[row]
    # values: the nodes where a label has them, 0 at the fill entry
    src = idx[:, 0].to(torch.int64)[row] + col
    has = lens[row] > 0
    vals = torch.zeros(nnz, dtype=torch.int64, device=dev)
    if ids.numel():
        vals[has] = ids[src[has]]
    width = max(int(lens.max().item()), 1)
    return torch.stack([row, col], 1), vals, [b, width]


_SE_COMBINER = {"sum": 0, "mean": 1, "sqrtn": 2}


def _sparse_embedding_raw(graph, nodes, fid, default_value, table, combiner, od):
    """euler_gpu_sparse_feature_embedding: (out [n, dim] of dtype od, counts [n] int32 - the
    entries each node's combiner counted).  Enqueue only."""
    n, (n_rows, dim) = nodes.numel(), table.shape
    out = torch.empty((n, dim), dtype=od, device=graph.device)
    counts = torch.empty(n, dtype=torch.int32, device=graph.device)
    with graph._on_device():
        check(lib().euler_gpu_sparse_feature_embedding(
            graph._h, _stream(), _ptr(nodes), n, int(fid), int(default_value is not None),
            int(default_value or 0), _ptr(table), Graph._FEAT_DT[table.dtype], int(n_rows), int(dim),
            _SE_COMBINER[combiner], _ptr(out), Graph._FEAT_DT[od], _ptr(counts)))
    return out, counts


def _sparse_embedding_pairs(graph, nodes, fid, default_value, n_rows):
    """(row of the batch, table row) of every entry, in batch order then stored order, from
    get_sparse_feature (one host wait).  An id that names no row is -1: the mask is taken on the
    int64 values, unsigned - before any cast to int32, which would wrap 2^32 + 5 into row 5."""
    # without a default the one entry of an empty node must name no row: -1 does
    (ind, val, _), = graph.get_sparse_feature(nodes, [fid], [-1 if default_value is None else default_value])
    ids = torch.where((val < 0) | (val >= n_rows), torch.full_like(val, -1), val)
    return ind[:, 0].contiguous(), ids


class _SparseFeatureEmbedding(torch.autograd.Function):
    """The fused lookup; the gradient of the table is the composition's:
    scatter_add(gather(s, row_of_entry), id_of_entry, V) with s = grad / (what the combiner
    divided by), through the fused gather_scatter (no [nnz, dim] intermediate), rounded once to
    the table's dtype.  Entries that name no row get exactly 0; nodes get no gradient."""

    @staticmethod
    def forward(ctx, table, graph, nodes, fid, default_value, combiner, od, sparse_grad):
        out, counts = _sparse_embedding_raw(graph, nodes, fid, default_value, table, combiner, od)
        ctx.save_for_backward(nodes, counts)
        ctx.graph, ctx.fid, ctx.default_value, ctx.combiner = graph, fid, default_value, combiner
        ctx.shape, ctx.dt, ctx.sparse_grad = tuple(table.shape), table.dtype, sparse_grad
        return out

    @staticmethod
    def backward(ctx, grad):
        from . import ops
        nodes, counts = ctx.saved_tensors
        n_rows, dim = ctx.shape
        s = grad.float()
        if ctx.combiner != "sum":
            denom = counts.to(torch.float32)
            if ctx.combiner == "sqrtn":
                denom = denom.sqrt()
            s = s / denom.reshape(-1, 1)
        s = s.masked_fill((counts == 0).reshape(-1, 1), 0).contiguous()
        rows, ids = _sparse_embedding_pairs(ctx.graph, nodes, ctx.fid, ctx.default_value, n_rows)
        none = (None,) * 7
        if not ctx.sparse_grad:
            return (ops.gather_scatter("add", s, rows, ids, n_rows).to(ctx.dt),) + none
        keep = ids >= 0
        rows, ids = rows[keep], ids[keep]
        if ids.numel() == 0:
            return (torch.sparse_coo_tensor(torch.zeros((1, 0), dtype=torch.int64, device=grad.device),
                                            torch.zeros((0, dim), dtype=ctx.dt, device=grad.device),
                                            (n_rows, dim)),) + none
        distinct, inverse = ops.id_unique(ids)
        values = ops.gather_scatter("add", s, rows, inverse, distinct.numel()).to(ctx.dt)
        return (torch.sparse_coo_tensor(distinct.reshape(1, -1), values, (n_rows, dim)),) + none


_NB_MODE = {"add": 0, "max": 1, "mean": 2}
_NB_KIND = {None: 0, "edge": 1, "norm": 2}


class _NeighborAggregate(torch.autograd.Function):
    """Graph.neighbor_aggregate: the fused forward (euler_gpu_neighbor_reduce).  The backward
    pass rebuilds the neighbour list and differentiates the composition of the existing ops
    (Graph.neighbor_aggregate_composed), so the gradients of table and root have its bits."""

    @staticmethod
    def forward(ctx, table, root, graph, nodes, edge_types, op, kind, self_loop, norm, a, b, od):
        from . import ops
        n, d = nodes.numel(), table.shape[1]
        out = torch.empty((n, d), dtype=od, device=table.device)
        et, et_p, k = _i32_array(edge_types)
        nd, ns = norm if norm is not None else (None, None)
        with graph._on_device():
            check(lib().euler_gpu_neighbor_reduce(
                graph._h, _stream(), _NB_MODE[op], _ptr(nodes), n, et_p, k, _NB_KIND[kind], 1 if self_loop else 0,
                _ptr(table), ops._DT[table.dtype], table.shape[0], d, _ptr(nd), _ptr(ns), _ptr(root),
                ops._DT[root.dtype] if root is not None else _lib.F32, a, b, _ptr(out), ops._DT[od]))
        ctx.save_for_backward(table, nodes, *[t for t in (root, nd, ns) if t is not None])
        ctx.has_root, ctx.has_norm = root is not None, norm is not None
        ctx.args = (graph, edge_types, op, kind, self_loop, a, b, od)
        return out

    @staticmethod
    def backward(ctx, grad):
        table, nodes = ctx.saved_tensors[:2]
        rest = list(ctx.saved_tensors[2:])
        root = rest.pop(0) if ctx.has_root else None
        norm = (rest[0], rest[1]) if ctx.has_norm else None
        graph, edge_types, op, kind, self_loop, a, b, od = ctx.args
        need_t, need_r = ctx.needs_input_grad[0], root is not None and ctx.needs_input_grad[1]
        with torch.enable_grad():
            t = table.detach().requires_grad_(need_t)
            r = root.detach().requires_grad_(need_r) if root is not None else None
            out = graph._aggregate_composed(op, t, nodes, edge_types, kind, norm, self_loop, r, a, b, od)
            wanted = [x for x, need in ((t, need_t), (r, need_r)) if need]
            got = list(torch.autograd.grad(out, wanted, grad)) if wanted else []
        grad_t = got.pop(0) if need_t else None
        grad_r = got.pop(0) if need_r else None
        return (grad_t, grad_r) + (None,) * 10


class Graph:
    """Immutable graph in HBM (CSR + row metadata + alias tables)."""

    def __init__(self, handle, device, meta=None):
        self._h = handle
        self.device = torch.device("cuda", device)
        self._dev_index = self.device.index
        self.device_index = device
        self.seed = 0
        self._call_id = 0
        self._lock = threading.Lock()
        self._nb_method = "exact"   # what method=None of sample_neighbor / sample_fanout resolves to
        self.data_path = None       # the directory of a loaded graph (feature names)
        self.node_type_names = (meta or {}).get("node_types", {})
        self.edge_type_names = (meta or {}).get("edge_types", {})

    # ------------------------------------------------------------ creation
    @classmethod
    def from_csr(cls, row_id, row_ptr, type_end, nbr, prefix_w, type_prefix,
                 n_edge_types, node_type=None, node_weight=None,
                 sampler_order=None, device=0, partitions=1, shard_index=0,
                 shards=1, features=None, sparse_features=None):
        """features = (n_float, feat_ptr [n+1], feat_idx [n*F], feat_val): the
        reference's per-node float_features_idx_ / float_features_
        (core/graph/node.h) concatenated over rows; sparse_features = the same
        four for uint64_features_idx_ / uint64_features_."""
        row_id = _np(row_id, np.uint64)
        row_ptr = _np(row_ptr, np.int64)
        type_end = _np(type_end, np.int32).reshape(-1)
        nbr = _np(nbr, np.uint64)
        prefix_w = _np(prefix_w, np.float32)
        type_prefix = _np(type_prefix, np.float32).reshape(-1)
        c = _lib.HostCSR()
        c.n_rows = len(row_id)
        c.n_edge_types = int(n_edge_types)
        keep = [row_id, row_ptr, type_end, nbr, prefix_w, type_prefix]
        c.row_id = row_id.ctypes.data_as(_lib.u64p)
        c.row_ptr = row_ptr.ctypes.data_as(_lib.i64p)
        c.type_end = type_end.ctypes.data_as(_lib.i32p)
        c.nbr = nbr.ctypes.data_as(_lib.u64p)
        c.prefix_w = prefix_w.ctypes.data_as(_lib.f32p)
        c.type_prefix = type_prefix.ctypes.data_as(_lib.f32p)
        n_node_types = 1
        if node_type is not None:
            node_type = _np(node_type, np.int32)
            keep.append(node_type)
            c.node_type = node_type.ctypes.data_as(_lib.i32p)
            n_node_types = int(node_type.max()) + 1 if len(node_type) else 1
        if node_weight is not None:
            node_weight = _np(node_weight, np.float32)
            keep.append(node_weight)
            c.node_weight = node_weight.ctypes.data_as(_lib.f32p)
        if sampler_order is not None:
            sampler_order = _np(sampler_order, np.uint64)
            keep.append(sampler_order)
            c.sampler_order = sampler_order.ctypes.data_as(_lib.u64p)
        c.n_node_types = n_node_types
        if features is not None:
            nf, fptr, fidx, fval = features
            fptr = _np(fptr, np.int64)
            fidx = _np(fidx, np.int32).reshape(-1)
            fval = _np(fval, np.float32)
            keep += [fptr, fidx, fval]
            c.n_float_features = int(nf)
            c.feat_ptr = fptr.ctypes.data_as(_lib.i64p)
            c.feat_idx = fidx.ctypes.data_as(_lib.i32p)
            c.feat_val = fval.ctypes.data_as(_lib.f32p)
        if sparse_features is not None:
            nu, uptr, uidx, uval = sparse_features
            uptr = _np(uptr, np.int64)
            uidx = _np(uidx, np.int32).reshape(-1)
            uval = _np(uval, np.uint64)
            keep += [uptr, uidx, uval]
            c.n_u64_features = int(nu)
            c.ufeat_ptr = uptr.ctypes.data_as(_lib.i64p)
            c.ufeat_idx = uidx.ctypes.data_as(_lib.i32p)
            c.ufeat_val = uval.ctypes.data_as(_lib.u64p)
        h = C.c_void_p()
        check(lib().euler_gpu_graph_create_shard(C.byref(c), device, partitions,
                                                 shard_index, shards, C.byref(h)))
        return cls(h, device)

    @classmethod
    def synthetic(cls, params, device=0, partitions=1, shard_index=0, shards=1):
        h = C.c_void_p()
        check(lib().euler_gpu_graph_create_synthetic(
            C.byref(params), device, partitions, shard_index, shards, C.byref(h)))
        return cls(h, device)

    @classmethod
    def from_edges(cls, src, dst=None, edge_type=None, weight=None, n_edge_types=None, nodes=None,
                   node_type=None, node_weight=None, n_node_types=None, features=None,
                   undirected=False, node_sampler=True, device=None):
        """The graph of an edge list that lives on the device, built there (csrc/edge_build.h): the
        same graph `from_csr` makes from these edges laid out by the reference's rules.

        src, dst: [E] int64 device tensors (the bits of the u64 ids); a [2, E] edge_index is taken as
        src with dst=None.  edge_type [E] (None: all 0), weight [E] (None: all 1.0).  n_edge_types None
        = max(edge_type) + 1.  nodes [N]: the rows, in this order (None: the distinct ids of src and
        dst, ascending as unsigned numbers).  node_type / node_weight [N] and features - a list of
        [N, d] fp32 tensors, one per dense feature slot - need nodes.  undirected: the list is the
        edges followed by all of them reversed.  node_sampler=False leaves the global node sampler to
        a later set_node_sampler.  Nothing given is written to; the work runs on the current stream
        and the graph is complete on return."""
        def dev_tensor(x, dtype):
            if x is None:
                return None
            if not torch.is_tensor(x):
                x = torch.as_tensor(np.asarray(x))
            return x.to(device=dev, dtype=dtype).contiguous()

        if dst is None:
            if not torch.is_tensor(src) or src.dim() != 2 or src.shape[0] != 2:
                raise ValueError("from_edges: dst=None needs a [2, E] edge_index as src")
            src, dst = src[0], src[1]
        if device is None:
            device = src.device.index if torch.is_tensor(src) and src.is_cuda else torch.cuda.current_device()
        dev = torch.device("cuda", device)
        src = dev_tensor(src, torch.int64).reshape(-1)
        dst = dev_tensor(dst, torch.int64).reshape(-1)
        n_e = src.numel()
        if dst.numel() != n_e:
            raise ValueError("from_edges: src and dst differ in length")
        edge_type = dev_tensor(edge_type, torch.int32)
        weight = dev_tensor(weight, torch.float32)
        for t, what in ((edge_type, "edge_type"), (weight, "weight")):
            if t is not None and t.numel() != n_e:
                raise ValueError("from_edges: %s has %d entries for %d edges" % (what, t.numel(), n_e))
        if n_edge_types is None:
            n_edge_types = int(edge_type.max()) + 1 if edge_type is not None and n_e else 1
        nodes = dev_tensor(nodes, torch.int64)
        n_n = nodes.numel() if nodes is not None else 0
        if nodes is not None and n_n == 0:
            nodes = torch.empty(1, dtype=torch.int64, device=dev)      # no rows, but a pointer: "given"
        node_type = dev_tensor(node_type, torch.int32)
        node_weight = dev_tensor(node_weight, torch.float32)
        for t, what in ((node_type, "node_type"), (node_weight, "node_weight")):
            if t is not None and nodes is not None and t.numel() != n_n:
                raise ValueError("from_edges: %s has %d entries for %d nodes" % (what, t.numel(), n_n))
        if n_node_types is None:
            n_node_types = int(node_type.max()) + 1 if node_type is not None and node_type.numel() else 1
        feats = [dev_tensor(f, torch.float32) for f in (features or [])]
        for f in feats:
            if nodes is not None and (f.dim() != 2 or f.shape[0] != n_n):
                raise ValueError("from_edges: a feature slot is [N, d], N = len(nodes)")
        e = _lib.DevEdges()
        e.n_edges, e.n_nodes = n_e, n_n
        e.n_edge_types, e.undirected = int(n_edge_types), 1 if undirected else 0
        e.src, e.dst, e.type, e.weight = _ptr(src), _ptr(dst), _ptr(edge_type), _ptr(weight)
        e.nodes, e.node_type, e.node_weight = _ptr(nodes), _ptr(node_type), _ptr(node_weight)
        e.n_node_types, e.node_sampler = int(n_node_types), 1 if node_sampler else 0
        e.n_features = len(feats)
        if feats:
            ptrs = (C.c_void_p * len(feats))(*[f.data_ptr() for f in feats])
            dims = (C.c_int32 * len(feats))(*[int(f.shape[1]) if f.dim() == 2 else 0 for f in feats])
            e.features = C.cast(ptrs, C.POINTER(C.c_void_p))
            e.feature_dims = C.cast(dims, _lib.i32p)
        h = C.c_void_p()
        with torch.cuda.device(dev):
            check(lib().euler_gpu_graph_create_from_edges(C.byref(e), device, _stream(), C.byref(h)))
        return cls(h, device)

    def from_edges_pass_ms(self):
        """{pass: milliseconds} of the build of a graph made by from_edges (the stream drained after
        each pass); {} for any other graph."""
        names = ("rows", "id_map", "keys", "sort", "segments", "gather", "prefix_short_rows",
                 "prefix_long_rows", "features", "search_index", "node_sampler")
        ms = np.zeros(len(names), np.float32)
        n = C.c_int32(0)
        check(lib().euler_gpu_graph_from_edges_pass_ms(self._h, ms.ctypes.data_as(_lib.f32p), len(names),
                                                       C.byref(n)))
        return {k: float(x) for k, x in zip(names[:n.value], ms)}

    @classmethod
    def load(cls, data_path, device=0, shard_index=0, shards=1, edges=False):
        """Graph::Init over a data directory; edges=True also loads the Edge records the shard
        keeps (edge sampling and edge features)."""
        h = C.c_void_p()
        check(lib().euler_gpu_graph_load(str(data_path).encode(), device,
                                         shard_index, shards, C.byref(h)))
        g = cls(h, device)
        g.data_path = str(data_path)
        if edges:
            check(lib().euler_gpu_graph_load_edges(h, g.data_path.encode(), shard_index, shards))
        return g

    def close(self):
        if self._h is not None and self._h.value:
            lib().euler_gpu_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -------------------------------------------------------------- facts
    @property
    def num_nodes(self):
        return lib().euler_gpu_graph_num_nodes(self._h)

    @property
    def num_edges(self):
        return lib().euler_gpu_graph_num_edges(self._h)

    @property
    def num_edge_types(self):
        return lib().euler_gpu_graph_num_edge_types(self._h)

    @property
    def num_node_types(self):
        return lib().euler_gpu_graph_num_node_types(self._h)

    @property
    def partitions(self):
        """euler.meta's partitions_num for a graph loaded from a data directory (0
        otherwise): the `partitions` a sharded sampler must route ids with."""
        return int(lib().euler_gpu_graph_partitions(self._h))

    @property
    def device_bytes(self):
        return lib().euler_gpu_graph_bytes(self._h)

    def node_weight_sums(self):
        out = np.zeros(max(self.num_node_types, 1), np.float32)
        check(lib().euler_gpu_graph_node_weight_sums(
            self._h, out.ctypes.data_as(_lib.f32p)))
        return out

    def export_rows(self, ids):
        """Rows of the device CSR for `ids` as host numpy arrays."""
        ids = _np(ids, np.uint64)
        n = len(ids)
        T = self.num_edge_types
        row_ptr = np.zeros(n + 1, np.int64)
        check(lib().euler_gpu_graph_export_rows(
            self._h, ids.ctypes.data_as(_lib.u64p), n,
            row_ptr.ctypes.data_as(_lib.i64p), None, None, None, None))
        tot = int(row_ptr[-1])
        type_end = np.zeros(n * T, np.int32)
        nbr = np.zeros(max(tot, 1), np.uint64)
        pw = np.zeros(max(tot, 1), np.float32)
        tp = np.zeros(n * T, np.float32)
        check(lib().euler_gpu_graph_export_rows(
            self._h, ids.ctypes.data_as(_lib.u64p), n,
            row_ptr.ctypes.data_as(_lib.i64p), type_end.ctypes.data_as(_lib.i32p),
            nbr.ctypes.data_as(_lib.u64p), pw.ctypes.data_as(_lib.f32p),
            tp.ctypes.data_as(_lib.f32p)))
        return row_ptr, type_end, nbr[:tot], pw[:tot], tp

    def side_index(self):
        """(bytes, lines, overflowing lines) of the header + window side index that hop 2 of the
        2-hop fanout draws through on plain weighted graphs (csrc/wb_hw.h, csrc/wb_hw2.h); bytes 0 = the graph
        has none (not that kind of graph, over the index budget, too many overflows).  Builds
        the indexes if needed; the bytes are part of `device_bytes`."""
        b, n, o = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().euler_gpu_graph_side_index(self._h, C.byref(b), C.byref(n), C.byref(o)))
        return b.value, n.value, o.value

    def side_index_format(self):
        """0 = no side index, 1 = the lines of csrc/wb_hw.h, 2 = those of csrc/wb_hw2.h (tuning key
        76 when the index was built).  Builds the indexes if needed."""
        f = C.c_int32(0)
        check(lib().euler_gpu_graph_side_index_format(self._h, C.byref(f)))
        return f.value

    def index_overflow_rows(self, cap=4096):
        """Node ids (identity id maps only) of rows in which a bucket of the weight-bucket index
        overflows its block, as found while the index was built (at most 4 096): draws that land
        there take the fallback search.  Tests draw roots from them on purpose."""
        out = np.zeros(max(int(cap), 1), np.uint64)
        n = C.c_int64(0)
        check(lib().euler_gpu_graph_index_overflow_rows(self._h, out.ctypes.data_as(_lib.u64p), int(cap),
                                                        C.byref(n)))
        return out[:n.value]

    # ------------------------------------------------- alias neighbour mode
    NEIGHBOR_METHODS = ("exact", "alias")

    def build_neighbor_alias(self):
        """Builds the neighbour alias tables (csrc/nb_alias.h: one 32-byte entry per edge) on the
        current stream and waits for them; idempotent.  `method="alias"` calls build them on
        first use.  Graphs with negative or NaN weights are refused (EulerGpuError)."""
        with self._on_device():
            check(lib().euler_gpu_graph_build_neighbor_alias(self._h, _stream()))

    def neighbor_alias(self):
        """(bytes, entries) of the neighbour alias tables, (0, 0) when they are not built; the
        bytes are part of `device_bytes`."""
        b, n = C.c_int64(0), C.c_int64(0)
        check(lib().euler_gpu_graph_neighbor_alias_info(self._h, C.byref(b), C.byref(n)))
        return b.value, n.value

    def neighbor_alias_rows(self, ids):
        """The alias entries of the rows of `ids`, in the row order of `export_rows`, as host
        arrays: (row_ptr, id_self, id_alias, prob, w_self, w_alias).  The tables must be built."""
        ids = _np(ids, np.uint64)
        n = len(ids)
        row_ptr = np.zeros(n + 1, np.int64)
        args = (self._h, ids.ctypes.data_as(_lib.u64p), n, row_ptr.ctypes.data_as(_lib.i64p))
        check(lib().euler_gpu_graph_export_neighbor_alias(*args, None, None, None, None, None))
        tot = int(row_ptr[-1])
        id_self, id_alias = np.zeros(max(tot, 1), np.uint64), np.zeros(max(tot, 1), np.uint64)
        prob, w_self, w_alias = (np.zeros(max(tot, 1), np.float32) for _ in range(3))
        check(lib().euler_gpu_graph_export_neighbor_alias(
            *args, id_self.ctypes.data_as(_lib.u64p), id_alias.ctypes.data_as(_lib.u64p),
            prob.ctypes.data_as(_lib.f32p), w_self.ctypes.data_as(_lib.f32p),
            w_alias.ctypes.data_as(_lib.f32p)))
        return row_ptr, id_self[:tot], id_alias[:tot], prob[:tot], w_self[:tot], w_alias[:tot]

    def set_neighbor_method(self, name):
        """The neighbour draw that `method=None` of `sample_neighbor` / `sample_fanout` resolves
        to: "exact" (the default: the reference's CDF inversion, its neighbours bit for bit) or
        "alias" (one alias-table entry per draw: the same distribution, other neighbours)."""
        self._nb_method = self._neighbor_method(name)

    def _neighbor_method(self, method):
        if method is None:
            return self._nb_method
        if method not in self.NEIGHBOR_METHODS:
            raise ValueError("method must be one of %s, not %r" % (" / ".join(self.NEIGHBOR_METHODS), method))
        return method

    # ---------------------------------------------------------------- RNG

    def _on_device(self):
        """Context of the graph's device; nothing to switch (and 5 us less per op) when the
        caller already runs on it."""
        if torch.cuda.current_device() == self._dev_index:
            return _NULL_CTX
        return torch.cuda.device(self.device)

    def set_seed(self, seed, call_id=0):
        """Fix the sampling stream: ids are a pure function of (seed, call_id,
        node id / sample index, draw index)."""
        with self._lock:
            self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            self._call_id = int(call_id)

    def _take_call_ids(self, n, call_id=None):
        if call_id is not None:
            return int(call_id) & 0xFFFFFFFF
        with self._lock:
            c = self._call_id
            self._call_id = (self._call_id + n) & 0xFFFFFFFF
        return c

    # ------------------------------------------------------------ sampling
    def sample_neighbor(self, nodes, edge_types, count, default_node=-1,
                        layout="tf", call_id=None, return_mask=False, dedup=True, method=None,
                        root_mask=None, root_group=1):
        """tf_euler SampleNeighbor (tf_euler/kernels/sample_neighbor_op.cc):
        nodes [n] int64 -> (neighbors [n,count] int64, weights f32, types
        int32).  layout='core' gives the API_SAMPLE_NB fill (0, 0.0, 0).
        method: "exact" (the reference's draw), "alias" (the alias tables: same distribution,
        other neighbours; `dedup` is accepted and ignored) or None = `set_neighbor_method`'s.
        root_mask: optional uint8 [ceil(n / root_group)]; the roots of a non-zero byte sample as
        node id 0 (how a fanout chains its hops)."""
        method = self._neighbor_method(method)
        nodes = _as_i64_cuda(nodes, self.device)
        shape = tuple(nodes.shape) + (int(count),)
        flat = nodes.reshape(-1)
        n = flat.numel()
        out_n = torch.empty(shape, dtype=torch.int64, device=self.device)
        out_w = torch.empty(shape, dtype=torch.float32, device=self.device)
        out_t = torch.empty(shape, dtype=torch.int32, device=self.device)
        mask = (torch.empty(n, dtype=torch.uint8, device=self.device)
                if return_mask else None)
        et, et_p, k = _i32_array(edge_types)
        lay = _lib.LAYOUT_TF if layout == "tf" else _lib.LAYOUT_CORE
        if root_mask is not None:
            if method == "exact" and not dedup:
                raise ValueError("root_mask: not with dedup=False")
            root_mask = root_mask.to(device=self.device, dtype=torch.uint8).contiguous()
            if root_group < 1 or root_mask.numel() * int(root_group) < n:
                raise ValueError("root_mask: needs ceil(n / root_group) bytes")
        with self._on_device():
            if method == "alias" or dedup:
                fn = lib().euler_gpu_sample_neighbor_alias if method == "alias" else lib().euler_gpu_sample_neighbor
                check(fn(
                    self._h, _stream(), self.seed, self._take_call_ids(1, call_id),
                    _ptr(flat), n, _ptr(root_mask), int(root_group), et_p, k, int(count), lay,
                    int(default_node), _ptr(out_n), _ptr(out_w), _ptr(out_t),
                    _ptr(mask)))
            else:       # roots known to be distinct (sharded sampler)
                check(lib().euler_gpu_sample_neighbor_distinct(
                    self._h, _stream(), self.seed, self._take_call_ids(1, call_id),
                    _ptr(flat), n, et_p, k, int(count), lay, int(default_node),
                    _ptr(out_n), _ptr(out_w), _ptr(out_t), _ptr(mask)))
        res = (out_n, out_w, out_t)
        return res + (mask,) if return_mask else res

    def sample_neighbor_sets(self, nodes, type_sets, count, default_node=-1, call_id=None,
                             feat=None, aggr="mean"):
        """S SampleNeighbor ops over the same nodes - one per edge-type set, as a heterogeneous
        (RGCN-style) model issues them - in ONE launch (euler_gpu_sample_neighbor_sets): returns
        (neighbors [S, n, count] int64, weights f32, types int32); set s draws with the call id
        of the s-th of S consecutive sample_neighbor calls, and the result equals theirs bit
        for bit.  With `feat` ([rows, d] f32 indexed by node id) the sampled neighbours'
        rows are aggregated per (set, root) in the same enqueue
        (euler_gpu_sample_aggregate_sets): a fourth result [S, n, d] = add / max / mean over
        the `count` rows, the bits of scatter_(aggr, gather(feat, neighbors))."""
        flat = _as_i64_cuda(nodes, self.device).reshape(-1)
        n, S = flat.numel(), len(type_sets)
        ks = [len(ts) for ts in type_sets]
        ks_a, ks_p, _ = _i32_array(ks)
        et_a, et_p, _ = _i32_array([int(t) for ts in type_sets for t in ts])
        out_n = torch.empty((S, n, int(count)), dtype=torch.int64, device=self.device)
        out_w = torch.empty((S, n, int(count)), dtype=torch.float32, device=self.device)
        out_t = torch.empty((S, n, int(count)), dtype=torch.int32, device=self.device)
        cid = self._take_call_ids(S, call_id)
        with self._on_device():
            if feat is None:
                check(lib().euler_gpu_sample_neighbor_sets(
                    self._h, _stream(), self.seed, cid, _ptr(flat), n, et_p, ks_p, S, int(count),
                    int(default_node), _ptr(out_n), _ptr(out_w), _ptr(out_t)))
                return out_n, out_w, out_t
            assert feat.dtype == torch.float32 and feat.dim() == 2 and feat.is_contiguous()
            if not 0 <= int(default_node) < feat.shape[0]:
                raise ValueError("sample_neighbor_sets(feat=...): default_node must name a row of the "
                                 "feature table (the row the default fill aggregates, e.g. max_id + 1); "
                                 "got %d for %d rows" % (int(default_node), feat.shape[0]))
            mode = {"add": 0, "max": 1, "mean": 2}[aggr]
            agg = torch.empty((S, n, feat.shape[1]), dtype=torch.float32, device=self.device)
            check(lib().euler_gpu_sample_aggregate_sets(
                self._h, _stream(), self.seed, cid, _ptr(flat), n, et_p, ks_p, S, int(count),
                int(default_node), mode, _ptr(feat), int(feat.shape[0]), int(feat.shape[1]),
                _ptr(out_n), _ptr(out_w), _ptr(out_t), _ptr(agg)))
        return out_n, out_w, out_t, agg

    def sample_neighbor_packed(self, nodes, edge_types, count, default_node=-1,
                               call_id=None):
        """The shard side of a multi-GPU hop: TF-layout SampleNeighbor of the
        (distinct) ids this shard owns, returned as wire rows for ops.expand_packed:
        [n, 4 * count + 2] int32 (ids | weights | types | mask, pad), or
        [n, 3 * count + 2 (padded to even)] without the types when one edge type is listed."""
        flat = _as_i64_cuda(nodes, self.device).reshape(-1)
        n = flat.numel()
        et, et_p, k = _i32_array(edge_types)
        # one listed type: the type column stays off the wire
        words = ((3 if k == 1 else 4) * int(count) + 2 + 1) & ~1
        rows = torch.empty((n, words), dtype=torch.int32, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_sample_neighbor_packed(
                self._h, _stream(), self.seed, self._take_call_ids(1, call_id),
                _ptr(flat), n, et_p, k, int(count), int(default_node), _ptr(rows)))
        return rows

    def sample_neighbor_sets_packed(self, nodes, type_sets, count, default_node=-1, call_id=None):
        """sample_neighbor_packed for several edge-type sets over the same (distinct) ids in ONE
        launch (euler_gpu_sample_neighbor_sets_packed): a list of wire-row tensors, one per set -
        the rows of len(type_sets) sample_neighbor_packed calls with consecutive call ids (views
        of one allocation)."""
        flat = _as_i64_cuda(nodes, self.device).reshape(-1)
        n, S = flat.numel(), len(type_sets)
        ks = [len(ts) for ts in type_sets]
        ks_a, ks_p, _ = _i32_array(ks)
        et_a, et_p, _ = _i32_array([int(t) for ts in type_sets for t in ts])
        words = [((3 if k == 1 else 4) * int(count) + 2 + 1) & ~1 for k in ks]
        buf = torch.empty((n * sum(words),), dtype=torch.int32, device=self.device)
        cid = self._take_call_ids(S, call_id)
        with self._on_device():
            check(lib().euler_gpu_sample_neighbor_sets_packed(
                self._h, _stream(), self.seed, cid, _ptr(flat), n, et_p, ks_p, S, int(count),
                int(default_node), _ptr(buf)))
        out, off = [], 0
        for w in words:
            out.append(buf[off:off + n * w].view(n, w))
            off += n * w
        return out

    def sample_fanout(self, nodes, edge_types, counts, default_node=-1,
                      call_id=None, method=None):
        """tf_euler sample_fanout (euler_ops/neighbor_ops.py:122-158 over
        tf_euler/kernels/sample_fanout_op.cc): returns (neighbors_list,
        weights_list, types_list) with flattened per-hop tensors.  method: as `sample_neighbor`."""
        method = self._neighbor_method(method)
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        layers = len(counts)
        et, et_p, k, cnt, cnt_p = _fanout_plan(edge_types, counts)
        n = nodes.numel()
        outs_n, outs_w, outs_t = [], [], []
        m = n
        for c in counts:
            m *= int(c)
            outs_n.append(torch.empty(m, dtype=torch.int64, device=self.device))
            outs_w.append(torch.empty(m, dtype=torch.float32, device=self.device))
            outs_t.append(torch.empty(m, dtype=torch.int32, device=self.device))
        ws_key = (n,) + tuple(int(c) for c in counts)
        ws_bytes = _WS_BYTES.get(ws_key)
        if ws_bytes is None:
            ws_bytes = int(lib().euler_gpu_sample_fanout_workspace(n, cnt_p, layers))
            if len(_WS_BYTES) < 4096:
                _WS_BYTES[ws_key] = ws_bytes
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=self.device)
        pn = (C.c_void_p * layers)(*[t.data_ptr() for t in outs_n])
        pw = (C.c_void_p * layers)(*[t.data_ptr() for t in outs_w])
        pt = (C.c_void_p * layers)(*[t.data_ptr() for t in outs_t])
        # (the alias mode's workspace has the exact mode's size: euler_gpu_sample_fanout_alias_workspace)
        fn = lib().euler_gpu_sample_fanout_alias if method == "alias" else lib().euler_gpu_sample_fanout
        with self._on_device():
            check(fn(
                self._h, _stream(), self.seed,
                self._take_call_ids(layers, call_id), _ptr(nodes), n, et_p, k,
                cnt_p, layers, int(default_node), pn, pw, pt, _ptr(ws)))
        return [nodes] + outs_n, outs_w, outs_t

    def sample_fanout_multi(self, batches, edge_types, counts, default_node=-1, call_id=None,
                            call_ids=None):
        """M minibatches of sample_fanout in ONE enqueue (euler_gpu_sample_fanout_multi):
        `batches` is an [M, B] tensor or a list of M equally long root tensors; minibatch b
        draws with call id call_id + b * len(counts) - what M consecutive sample_fanout calls
        take from the graph's counter - or call_ids[b] (a device uint32 / int32 tensor).
        Returns a list of M (neighbors_list, weights_list, types_list), each what
        sample_fanout returns for that minibatch (views of one allocation per hop), bit for
        bit."""
        if isinstance(batches, (list, tuple)):
            batches = torch.stack([_as_i64_cuda(b, self.device).reshape(-1) for b in batches], 0)
        roots = _as_i64_cuda(batches, self.device)
        assert roots.dim() == 2, "batches: [M, B]"
        roots = roots.contiguous()
        m, n = int(roots.shape[0]), int(roots.shape[1])
        layers = len(counts)
        et, et_p, k, cnt, cnt_p = _fanout_plan(edge_types, counts)
        outs_n, outs_w, outs_t, rows = [], [], [], n
        for c in counts:
            rows *= int(c)
            outs_n.append(torch.empty((m, rows), dtype=torch.int64, device=self.device))
            outs_w.append(torch.empty((m, rows), dtype=torch.float32, device=self.device))
            outs_t.append(torch.empty((m, rows), dtype=torch.int32, device=self.device))
        ws_key = (m * n,) + tuple(int(c) for c in counts)
        ws_bytes = _WS_BYTES.get(ws_key)
        if ws_bytes is None:
            ws_bytes = int(lib().euler_gpu_sample_fanout_workspace(m * n, cnt_p, layers))
            if len(_WS_BYTES) < 4096:
                _WS_BYTES[ws_key] = ws_bytes
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=self.device)
        pn = (C.c_void_p * layers)(*[t.data_ptr() for t in outs_n])
        pw = (C.c_void_p * layers)(*[t.data_ptr() for t in outs_w])
        pt = (C.c_void_p * layers)(*[t.data_ptr() for t in outs_t])
        ids_p = None
        if call_ids is not None:
            call_ids = call_ids.to(device=self.device, dtype=torch.int32).contiguous()
            assert call_ids.numel() == m
            ids_p = _ptr(call_ids)
        with self._on_device():
            check(lib().euler_gpu_sample_fanout_multi(
                self._h, _stream(), self.seed, self._take_call_ids(layers * m, call_id), layers,
                ids_p, m, _ptr(roots), n, et_p, k, cnt_p, layers, int(default_node), pn, pw, pt,
                _ptr(ws)))
        return [([roots[b]] + [t[b] for t in outs_n], [t[b] for t in outs_w], [t[b] for t in outs_t])
                for b in range(m)]

    def sample_fanout_unique(self, nodes, edge_types, counts, default_node=-1, call_id=None):
        """The 2-hop fanout in the (unique rows, index) form (euler_gpu_sample_fanout_unique):
        returns (hop-1 ids [n, c1], weights, types, row_index [n * c1] int64, rows_id
        [n * c1, c2], rows_w, rows_t) with hop-2 tensor = rows[row_index]; only the rows
        row_index names are written.  Raises EulerGpuError(EINVAL) for graphs / fanouts the
        one-kernel path does not serve."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        assert len(counts) == 2
        et = np.asarray(edge_types, dtype=np.int32).reshape(2, -1)
        assert et.shape[1] == 1, "one listed edge type per hop"
        et, et_p, _ = _i32_array(et)
        cnt, cnt_p, _ = _i32_array(counts)
        n, c1, c2 = nodes.numel(), int(counts[0]), int(counts[1])
        dev = self.device
        id1 = torch.empty((n, c1), dtype=torch.int64, device=dev)
        w1 = torch.empty((n, c1), dtype=torch.float32, device=dev)
        t1 = torch.empty((n, c1), dtype=torch.int32, device=dev)
        idx = torch.empty(n * c1, dtype=torch.int32, device=dev)
        rid = torch.empty((n * c1, c2), dtype=torch.int64, device=dev)
        rw = torch.empty((n * c1, c2), dtype=torch.float32, device=dev)
        rt = torch.empty((n * c1, c2), dtype=torch.int32, device=dev)
        ws_bytes = lib().euler_gpu_sample_fanout_workspace(n, cnt_p, 2)
        ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=dev)
        with self._on_device():
            check(lib().euler_gpu_sample_fanout_unique(
                self._h, _stream(), self.seed, self._take_call_ids(2, call_id), _ptr(nodes), n,
                et_p, cnt_p, int(default_node), _ptr(id1), _ptr(w1), _ptr(t1), _ptr(idx),
                _ptr(rid), _ptr(rw), _ptr(rt), _ptr(ws)))
        # uint32 row numbers read as int64 for indexing
        return id1, w1, t1, idx.to(torch.int64) & 0xFFFFFFFF, rid, rw, rt

    def sample_fanout_with_feature(self, nodes, edge_types, counts, default_node,
                                   feature_ids, dimensions, call_id=None, out_dtype=None):
        """tf_euler sample_fanout_with_feature, dense part (euler_ops/neighbor_ops.py:49-70
        over tf_euler/kernels/sample_fanout_with_feature_op.cc:135-233) as ONE enqueue
        (euler_gpu_sample_fanout_with_feature): returns (neighbors_list, weights_list,
        types_list, dense_features) with dense_features[layer * len(feature_ids) + j] =
        [m_layer, dimensions[j]], layer 0 = the roots.  out_dtype as get_dense_feature (16-bit
        rows are fetched per layer after the fanout's enqueue)."""
        od = self._feature_out_dtype(out_dtype)
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        layers = len(counts)
        et = np.asarray(edge_types, dtype=np.int32).reshape(layers, -1)
        et, et_p, _ = _i32_array(et)
        k = et.size // layers if layers else 0
        cnt, cnt_p, _ = _i32_array(counts)
        fid, fid_p, _ = _i32_array(feature_ids)
        dim, dim_p, _ = _i32_array(dimensions)
        nd = len(feature_ids)
        n = nodes.numel()
        outs_n, outs_w, outs_t, dense = [], [], [], []
        m = n
        sizes = [n]
        for c in counts:
            m *= int(c)
            sizes.append(m)
            outs_n.append(torch.empty(m, dtype=torch.int64, device=self.device))
            outs_w.append(torch.empty(m, dtype=torch.float32, device=self.device))
            outs_t.append(torch.empty(m, dtype=torch.int32, device=self.device))
        if od != torch.float32:
            nd = 0              # the entry writes fp32 rows: the typed fetch follows the fanout
        for ml in sizes:
            for d in (dimensions if nd else ()):
                dense.append(torch.empty((ml, int(d)), dtype=torch.float32, device=self.device))
        ws_bytes = lib().euler_gpu_sample_fanout_workspace(n, cnt_p, layers)
        ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=self.device)
        pn = (C.c_void_p * max(layers, 1))(*[t.data_ptr() for t in outs_n])
        pw = (C.c_void_p * max(layers, 1))(*[t.data_ptr() for t in outs_w])
        pt = (C.c_void_p * max(layers, 1))(*[t.data_ptr() for t in outs_t])
        pd = (C.c_void_p * max(len(dense), 1))(*[t.data_ptr() for t in dense])
        with self._on_device():
            check(lib().euler_gpu_sample_fanout_with_feature(
                self._h, _stream(), self.seed, self._take_call_ids(layers, call_id),
                _ptr(nodes), n, et_p, k, cnt_p, layers, int(default_node), pn, pw, pt, _ptr(ws),
                fid_p, dim_p, nd, pd))
        if od != torch.float32:
            for layer_nodes in [nodes] + outs_n:
                dense.extend(self.get_dense_feature(layer_nodes, feature_ids, dimensions, out_dtype=od))
        return [nodes] + outs_n, outs_w, outs_t, dense

    def sage_blocks(self, nodes, edge_types, fanouts, default_node=-1, add_self_loops=True,
                    call_id=None, sync=True):
        """The whole SageDataFlow (tf_euler/python/dataflow/sage_dataflow.py +
        UniqueDataFlow.produce_subgraph) as ONE enqueue, no host round trip between
        the hops (euler_gpu_sage_blocks).  Returns (blocks, counts): blocks[h] =
        (n_id, res_n_id, edge_src, edge_dst, edge_index) - FIVE entries since round 4: edge_index
        is the [:, :e] view of the [2, cap] tensor whose rows are edge_src / edge_dst (rows
        contiguous, the tensor as a whole not: .contiguous() before .view(-1) / data_ptr() /
        torch.save, which would otherwise serialise the cap-sized storage) - and
        counts = the layer sizes - sliced to
        their true sizes after one read of the counts when sync is True, else padded
        to the worst case with `counts` left on the device (uint32 [layers + 1])."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        layers = len(fanouts)
        et = np.asarray(edge_types, dtype=np.int32).reshape(layers, -1)
        et, et_p, _ = _i32_array(et)
        k = et.size // layers if layers else 0
        fan, fan_p, _ = _i32_array(fanouts)
        n = nodes.numel()
        caps = [n]
        for c in fanouts:
            caps.append(caps[-1] * (int(c) + 1))
        dev = self.device
        n_ids = [torch.empty(max(caps[h + 1], 1), dtype=torch.int64, device=dev) for h in range(layers)]
        res = [torch.empty(max(caps[h], 1), dtype=torch.int64, device=dev) for h in range(layers)]
        # edge_src / edge_dst of a hop are the two rows of ONE [2, cap] tensor: the block's
        # edge_index is then a view of it ([:, :e]) instead of a stacked copy
        eidx = [torch.empty((2, max(caps[h + 1], 1)), dtype=torch.int64, device=dev) for h in range(layers)]
        esrc = [t[0] for t in eidx]
        edst = [t[1] for t in eidx]
        counts = torch.zeros(layers + 1, dtype=torch.int32, device=dev)
        ws = torch.empty(max(int(lib().euler_gpu_sage_blocks_workspace(n, fan_p, layers)), 16),
                         dtype=torch.uint8, device=dev)
        arr = lambda ts: (C.c_void_p * layers)(*[t.data_ptr() for t in ts])
        with self._on_device():
            check(lib().euler_gpu_sage_blocks(
                self._h, _stream(), self.seed, self._take_call_ids(layers, call_id), _ptr(nodes), n,
                et_p, k, fan_p, layers, int(default_node), 1 if add_self_loops else 0, _ptr(ws),
                arr(n_ids), arr(res), arr(esrc), arr(edst), _ptr(counts)))
        if not sync:
            return list(zip(n_ids, res, esrc, edst, eidx)), counts
        cnt = _read_counts(counts)                             # the one host read
        blocks = []
        for h in range(layers):
            e = cnt[h] * int(fanouts[h]) + (cnt[h] if add_self_loops else 0)
            blocks.append((n_ids[h][:cnt[h + 1]], res[h][:cnt[h]], esrc[h][:e], edst[h][:e], eidx[h][:, :e]))
        return blocks, cnt

    def sage_blocks_multi(self, nodes, edge_types, fanouts, default_node=-1, add_self_loops=True,
                          call_id=None, sync=True):
        """M minibatches' SageDataFlows as ONE enqueue (euler_gpu_sage_blocks_multi): nodes
        [M, n] int64 -> a list of M (blocks, counts) pairs, each what sage_blocks returns for
        that minibatch - minibatch b draws with the call ids of the b-th of M consecutive
        sage_blocks calls, and the result equals theirs bit for bit.  sync=False: (padded
        tensors per hop - n_id [M, cap], res_n_id [M, cap], edge_src / edge_dst [M, cap] - and the
        device-side counts [M, layers + 1]), no host read."""
        nodes = _as_i64_cuda(nodes, self.device)
        assert nodes.dim() == 2, "sage_blocks_multi: nodes must be [M, n]"
        M, n = int(nodes.shape[0]), int(nodes.shape[1])
        nodes = nodes.contiguous()
        layers = len(fanouts)
        et = np.asarray(edge_types, dtype=np.int32).reshape(layers, -1)
        et, et_p, _ = _i32_array(et)
        k = et.size // layers if layers else 0
        fan, fan_p, _ = _i32_array(fanouts)
        caps = [n]
        for c in fanouts:
            caps.append(caps[-1] * (int(c) + 1))
        dev = self.device
        n_ids = [torch.empty((M, max(caps[h + 1], 1)), dtype=torch.int64, device=dev) for h in range(layers)]
        res = [torch.empty((M, max(caps[h], 1)), dtype=torch.int64, device=dev) for h in range(layers)]
        esrc = [torch.empty((M, max(caps[h + 1], 1)), dtype=torch.int64, device=dev) for h in range(layers)]
        edst = [torch.empty((M, max(caps[h + 1], 1)), dtype=torch.int64, device=dev) for h in range(layers)]
        counts = torch.zeros((M, layers + 1), dtype=torch.int32, device=dev)
        ws = torch.empty(max(int(lib().euler_gpu_sage_blocks_multi_workspace(M, n, fan_p, layers)), 16),
                         dtype=torch.uint8, device=dev)
        arr = lambda ts: (C.c_void_p * layers)(*[t.data_ptr() for t in ts])
        with self._on_device():
            check(lib().euler_gpu_sage_blocks_multi(
                self._h, _stream(), self.seed, self._take_call_ids(layers * M, call_id), layers, M,
                _ptr(nodes), n, et_p, k, fan_p, layers, int(default_node), 1 if add_self_loops else 0,
                _ptr(ws), arr(n_ids), arr(res), arr(esrc), arr(edst), _ptr(counts)))
        if not sync:
            return list(zip(n_ids, res, esrc, edst)), counts
        cnt_all = counts.cpu().numpy().astype(np.int64)          # the one host read
        out = []
        for b in range(M):
            cnt = [int(x) for x in cnt_all[b]]
            blocks = []
            for h in range(layers):
                e = cnt[h] * int(fanouts[h]) + (cnt[h] if add_self_loops else 0)
                s_, d_ = esrc[h][b, :e], edst[h][b, :e]
                blocks.append((n_ids[h][b, :cnt[h + 1]], res[h][b, :cnt[h]], s_, d_, torch.stack([s_, d_], 0)))
            out.append((blocks, cnt))
        return out

    def full_blocks(self, nodes, edge_types, edge_caps, add_self_loops=True, with_types=False):
        """GCNDataFlow / RelationDataFlow block construction as ONE enqueue
        (euler_gpu_full_blocks): every hop = full neighbours of the listed types of the
        nodes so far + first-occurrence unique + res_n_id + edge_index.  edge_caps[h] =
        capacity of hop h's edge list.  Returns (blocks, counts) with blocks[h] = (n_id,
        res_n_id, edge_src, edge_dst, e_type or None) sliced to their true sizes after the
        one host read of the counts, or None when a hop overflowed its capacity (counts then
        tells the sizes that were reached)."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        layers = len(edge_types)
        et = np.asarray(edge_types, dtype=np.int32).reshape(layers, -1)
        et, et_p, _ = _i32_array(et)
        k = et.size // layers if layers else 0
        n = nodes.numel()
        caps_e = [int(c) for c in edge_caps]
        caps_n = [n]
        for c in caps_e:
            caps_n.append(caps_n[-1] + c)
        dev = self.device
        ecap = (C.c_int64 * layers)(*caps_e)
        n_ids = [torch.empty(max(caps_n[h + 1], 1), dtype=torch.int64, device=dev) for h in range(layers)]
        res = [torch.empty(max(caps_n[h], 1), dtype=torch.int64, device=dev) for h in range(layers)]
        esrc = [torch.empty(max(caps_e[h] + caps_n[h], 1), dtype=torch.int64, device=dev) for h in range(layers)]
        edst = [torch.empty(max(caps_e[h] + caps_n[h], 1), dtype=torch.int64, device=dev) for h in range(layers)]
        etyp = [torch.empty(max(caps_e[h], 1), dtype=torch.int32, device=dev) for h in range(layers)] \
            if with_types else None
        counts = torch.zeros(2 * layers + 2, dtype=torch.int32, device=dev)
        ws = torch.empty(max(int(lib().euler_gpu_full_blocks_workspace(n, ecap, layers)), 16),
                         dtype=torch.uint8, device=dev)
        arr = lambda ts: (C.c_void_p * layers)(*[t.data_ptr() for t in ts])
        with self._on_device():
            check(lib().euler_gpu_full_blocks(
                self._h, _stream(), _ptr(nodes), n, et_p, k, layers, 1 if add_self_loops else 0, ecap,
                _ptr(ws), arr(n_ids), arr(res), arr(esrc), arr(edst),
                arr(etyp) if with_types else None, _ptr(counts)))
        cnt = _read_counts(counts)                             # the one host read
        if cnt[2 * layers + 1]:
            return None, cnt
        blocks = []
        for h in range(layers):
            m_nb = cnt[layers + 1 + h]
            e = m_nb + (cnt[h] if add_self_loops else 0)
            blocks.append((n_ids[h][:cnt[h + 1]], res[h][:cnt[h]], esrc[h][:e], edst[h][:e],
                           etyp[h][:m_nb] if with_types else None))
        return blocks, cnt

    def set_node_sampler(self, ids=None, node_types=None, node_weights=None, n_node_types=None):
        """Graph::BuildGlobalSampler (core/graph/graph.cc:333-370) for a graph that has no
        global node sampler yet (a synthetic one), or in place of the one it has: the nodes
        in the order the sampler enumerates them (ids None = the rows in row order), their
        types (None = 0) and weights (None = 1.0).  Host arrays; host work."""
        n = self.num_nodes if ids is None else len(ids)
        ids_a = None if ids is None else _np(ids, np.uint64)
        ty_a = None if node_types is None else _np(node_types, np.int32)
        w_a = None if node_weights is None else _np(node_weights, np.float32)
        for a in (ty_a, w_a):
            if a is not None and len(a) != n:
                raise ValueError("set_node_sampler: array lengths differ")
        if n_node_types is None:
            n_node_types = int(ty_a.max()) + 1 if ty_a is not None and n else 1
        check(lib().euler_gpu_graph_set_node_sampler(
            self._h, int(n),
            None if ids_a is None else ids_a.ctypes.data_as(_lib.u64p),
            None if ty_a is None else ty_a.ctypes.data_as(_lib.i32p),
            None if w_a is None else w_a.ctypes.data_as(_lib.f32p), int(n_node_types)))

    def sample_node(self, count, node_type=-1, call_id=None):
        """tf_euler sample_node (tf_euler/kernels/sample_node_op.cc:39-98):
        [count] int64 ids drawn by node weight within the type(s)."""
        nt, nt_p, k = _i32_array(np.atleast_1d(node_type))
        out = torch.empty(int(count), dtype=torch.int64, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_sample_node(
                self._h, _stream(), self.seed, self._take_call_ids(1, call_id),
                nt_p, k, int(count), _ptr(out)))
        return out

    def id_range(self):
        """(largest node id of this graph / shard, ids are base + stride * row)."""
        mx = C.c_uint64(0)
        ident = C.c_int32(0)
        check(lib().euler_gpu_graph_id_range(self._h, C.byref(mx), C.byref(ident)))
        return int(mx.value), bool(ident.value)

    @property
    def num_float_features(self):
        return lib().euler_gpu_graph_num_float_features(self._h)

    _FEAT_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}
    _FEAT_TORCH = {v: k for k, v in _FEAT_DT.items()}

    @property
    def dense_feature_dtype(self):
        """storage dtype of the dense feature table: torch.float32 until
        set_dense_feature_dtype converts it"""
        return self._FEAT_TORCH[lib().euler_gpu_graph_dense_feature_dtype(self._h)]

    def set_dense_feature_dtype(self, dtype):
        """Store the dense feature table as torch.bfloat16 or torch.float16
        (euler_gpu_graph_set_dense_feature_dtype): every value rounded once, to nearest even,
        on the device; the fp32 table is freed (device_bytes drops by half the table).  The
        same dtype again is a no-op; a 16-bit table cannot be converted again (ValueError),
        nor can a shard of a sharded graph.  Waits for the device."""
        if dtype not in self._FEAT_DT:
            raise TypeError("set_dense_feature_dtype: float32, bfloat16 or float16, not %s" % (dtype,))
        with self._on_device():
            try:
                check(lib().euler_gpu_graph_set_dense_feature_dtype(self._h, _stream(),
                                                                    self._FEAT_DT[dtype]))
            except _lib.EulerGpuError as err:
                if err.code == _lib.EINVAL:
                    raise ValueError(str(err)) from None
                raise
        return self

    def _feature_out_dtype(self, out_dtype):
        """None = the table's dtype; else fp32 or - for an fp32 table - either 16-bit type"""
        table = self.dense_feature_dtype
        if out_dtype is None:
            return table
        if out_dtype not in self._FEAT_DT:
            raise TypeError("get_dense_feature: out_dtype is float32, bfloat16 or float16, not %s"
                            % (out_dtype,))
        if table != torch.float32 and out_dtype not in (torch.float32, table):
            raise TypeError("get_dense_feature: out_dtype is float32 or the table's dtype (%s), not %s"
                            % (table, out_dtype))
        return out_dtype

    def get_dense_feature(self, nodes, feature_ids, dimensions, out_dtype=None):
        """tf_euler get_dense_feature (euler_ops/feature_ops.py:108-122 over
        tf_euler/kernels/get_dense_feature_op.cc): nodes [n] int64 -> list of
        [n, dim] tensors, one per feature id; unknown nodes and missing
        features are zero rows.  out_dtype: None = the table's dtype (float32 unless
        set_dense_feature_dtype changed it); torch.float32 widens a 16-bit table's rows;
        a 16-bit type on an fp32 table rounds the rows once at the store."""
        od = self._feature_out_dtype(out_dtype)
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        n = nodes.numel()
        outs = []
        with self._on_device():
            for fid, dim in zip(feature_ids, dimensions):
                out = torch.empty((n, int(dim)), dtype=od, device=self.device)
                if od == torch.float32:
                    check(lib().euler_gpu_get_dense_feature(
                        self._h, _stream(), _ptr(nodes), n, int(fid), int(dim), _ptr(out)))
                else:
                    check(lib().euler_gpu_get_dense_feature_t(
                        self._h, _stream(), _ptr(nodes), n, int(fid), int(dim), _ptr(out),
                        self._FEAT_DT[od]))
                outs.append(out)
        return outs

    def fp8_dense_feature(self, fid, dim, chunk_rows=1 << 20):
        """The float feature slot `fid` of every id 0 .. max_id as an id-indexed ops.Fp8Rows table
        of max_id + 1 rows and `dim` columns (an id that is no node, or a short slot: zeros, as
        get_dense_feature) - the constant input features of a GNN at a quarter of their fp32
        bytes, read by ops.gather / ops.gather_segment_reduce with the sampled ids as they are.
        Two passes of get_dense_feature in chunks of chunk_rows ids - the column absmax, then the
        store - so no more than one fp32 chunk is alive at a time: the result equals
        Fp8Rows.quantize(get_dense_feature(all ids)).  Plain Python over those primitives; the
        graph's own table and everything that reads it are untouched."""
        from . import ops
        rows, dim, chunk_rows = int(self.id_range()[0]) + 1, int(dim), max(1, int(chunk_rows))

        def chunks():
            for first in range(0, rows, chunk_rows):
                ids = torch.arange(first, min(first + chunk_rows, rows), dtype=torch.int64, device=self.device)
                yield first, self.get_dense_feature(ids, [fid], [dim], out_dtype=torch.float32)[0]

        absmax = torch.zeros(dim, dtype=torch.float32, device=self.device)
        for _, x in chunks():
            ops.column_absmax(x, out=absmax)
        table = ops.Fp8Rows.empty(rows, dim, ops.Fp8Rows.scale_of(absmax), self.device)
        for first, x in chunks():
            table.store(first, x)
        return table

    def supervise_loss(self, nodes, logits, label_fid, label_dim, metric=None, return_prob=False):
        """SuperviseModel.__call__ after out_fc (tf_euler/python/mp_utils/base.py:35-47) in one
        kernel: nodes [B] int64 and logits [B, label_dim] -> the mean sigmoid cross-entropy against
        the float feature slot label_fid of the nodes, read straight from the feature table with
        get_dense_feature's semantics (an unknown node or slot: zeros; a slot shorter than
        label_dim: zero filled; a longer one: truncated; a 16-bit table: widened) - no [B, C]
        label block is built.  metric, return_prob, the arithmetic and the gradient:
        ops.supervise_loss."""
        from . import ops
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        if logits.dim() != 2 or logits.shape[0] != nodes.numel() or logits.shape[1] != int(label_dim):
            raise ValueError("supervise_loss: logits is [len(nodes), label_dim]")
        return ops._supervise_call("supervise_loss", logits, None, self, nodes, int(label_fid), metric, return_prob)

    def num_u64_features(self):
        return lib().euler_gpu_graph_num_u64_features(self._h)

    def get_sparse_feature(self, nodes, feature_ids, default_values=None):
        """tf_euler get_sparse_feature (euler_ops/feature_ops.py:57-73 over
        tf_euler/kernels/get_sparse_feature_op.cc): nodes [n] int64 -> one
        SparseTensor triple (indices [nnz, 2] int64, values [nnz] int64,
        dense_shape [n, max_len]) per uint64 feature id; a node without values
        contributes the single entry (row, 0) = default value."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        n = nodes.numel()
        if default_values is None:
            default_values = [0] * len(feature_ids)
        outs = []
        with self._on_device():
            for fid, dv in zip(feature_ids, default_values):
                row_off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
                nnz, max_len = C.c_int64(0), C.c_int64(0)
                check(lib().euler_gpu_get_sparse_feature(
                    self._h, _stream(), _ptr(nodes), n, int(fid), int(dv), _ptr(row_off),
                    C.byref(nnz), C.byref(max_len), None, None))
                ind = torch.empty((int(nnz.value), 2), dtype=torch.int64, device=self.device)
                val = torch.empty(int(nnz.value), dtype=torch.int64, device=self.device)
                if nnz.value:
                    check(lib().euler_gpu_get_sparse_feature(
                        self._h, _stream(), _ptr(nodes), n, int(fid), int(dv),
                        _ptr(row_off), C.byref(nnz), C.byref(max_len), _ptr(ind),
                        _ptr(val)))
                outs.append((ind, val, [n, int(max_len.value)] if n else [0, 0]))
        return outs

    def sparse_feature_embedding(self, nodes, feature_ids, tables, combiner="sum", default_values=None,
                                 out_dtype=None, sparse_grad=False):
        """ShallowEncoder's lookup of sparse features (tf_euler/python/utils/encoders.py:146-170:
        get_sparse_feature, then tf.nn.embedding_lookup_sparse(table, sp, None, combiner)) in one
        kernel per feature and without a host wait: nodes [n] int64 -> one [n, dim] tensor per
        (feature id, table [V, dim]; float32, bfloat16 or float16).
        A node's entries are the values of its uint64 slot; a node without any has the one entry
        default_values[j] - or none at all when default_values (or that element) is None.  An
        entry >= V, compared unsigned, names no row: it is left out of the sum and of the count,
        and its gradient is exactly 0.  The counted rows are added in fp32 in stored order;
        combiner "sum", "mean" (sum / count) or "sqrtn" (sum / sqrt(count)); count 0 gives a zero
        row.  out_dtype: None = the table's dtype, or torch.float32.
        The table receives a gradient (nodes do not): dense [V, dim], or with sparse_grad=True a
        torch.sparse_coo_tensor over the distinct rows that were read - what
        torch.optim.SparseAdam and SGD take - with the same bits once coalesced."""
        from . import ops
        if combiner not in _SE_COMBINER:
            raise ValueError("sparse_feature_embedding: combiner is sum, mean or sqrtn")
        feature_ids, tables = list(feature_ids), list(tables)
        if len(feature_ids) != len(tables):
            raise ValueError("sparse_feature_embedding: one table per feature id")
        if default_values is None:
            default_values = [None] * len(feature_ids)
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        outs = []
        for fid, table, dv in zip(feature_ids, tables, default_values):
            if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] < 1:
                raise ValueError("sparse_feature_embedding: a table is [V, dim]")
            ops._need_cuda(table)
            ops._dt("sparse_feature_embedding", table)
            od = ops._out_dt("sparse_feature_embedding", table, out_dtype)
            if not table.is_contiguous():
                table = table.contiguous()
            outs.append(_SparseFeatureEmbedding.apply(
                table, self, nodes, int(fid), None if dv is None else int(dv), combiner, od,
                bool(sparse_grad)))
        return outs

    def get_sparse_feature_core(self, nodes, fid):
        """One uint64 feature slot in the GQL `values()` layout: (idx [n, 2]
        int32 offsets, values int64), no default entries."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        n = nodes.numel()
        idx = torch.empty((n, 2), dtype=torch.int32, device=self.device)
        total = C.c_int64(0)
        with self._on_device():
            check(lib().euler_gpu_get_sparse_feature_core(
                self._h, _stream(), _ptr(nodes), n, int(fid), _ptr(idx), C.byref(total),
                None))
            vals = torch.empty(int(total.value), dtype=torch.int64, device=self.device)
            if total.value:
                check(lib().euler_gpu_get_sparse_feature_core(
                    self._h, _stream(), _ptr(nodes), n, int(fid), _ptr(idx),
                    C.byref(total), _ptr(vals)))
        return idx, vals

    # ---------------------------------------------------------------- edge records
    def set_edges(self, src, dst, types, weights, dense=None, sparse=None, binary=None):
        """The edge store over host records in ordinal order ((src, dst, type) distinct).
        Features, each optional, one entry per slot: an [n, d] array (every record d values;
        binary: uint8) or a list of n per-record sequences (binary: `bytes`)."""
        n = len(src)
        keep = [_np(src, np.uint64), _np(dst, np.uint64), _np(types, np.int32),
                _np(weights, np.float32)]
        e = _lib.HostEdges()
        e.n = n
        e.src, e.dst = keep[0].ctypes.data_as(_lib.u64p), keep[1].ctypes.data_as(_lib.u64p)
        e.type, e.weight = keep[2].ctypes.data_as(_lib.i32p), keep[3].ctypes.data_as(_lib.f32p)
        keep.append(_edge_feature_tables(e, n, dense, sparse, binary))
        with self._on_device():
            check(lib().euler_gpu_graph_set_edges(self._h, C.byref(e)))

    def set_edge_features(self, dense=None, sparse=None, binary=None):
        """Replace the store's feature tables (rows in ordinal order, the forms of set_edges) -
        features for the records edges_from_rows built."""
        n = self.num_edge_records
        e = _lib.HostEdges()
        e.n = n
        keep = _edge_feature_tables(e, n, dense, sparse, binary)   # noqa: F841 (alive for the call)
        with self._on_device():
            check(lib().euler_gpu_graph_set_edge_features(self._h, C.byref(e)))

    def edges_from_rows(self):
        """The edge store over the distinct (src, dst, type) entries of the rows, built on the
        device (row order, then entry order; weights = the entries' own)."""
        with self._on_device():
            check(lib().euler_gpu_graph_edges_from_rows(self._h))

    @property
    def num_edge_records(self):
        """Records of the edge store (-1: none)."""
        return int(lib().euler_gpu_graph_num_edge_records(self._h))

    def export_edges(self, first=0, n=None):
        """Records [first, first + n) in ordinal order: (src, dst, type, weight) numpy arrays."""
        if n is None:
            n = self.num_edge_records - first
        out = (np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.int32),
               np.zeros(n, np.float32))
        check(lib().euler_gpu_graph_export_edges(
            self._h, int(first), int(n), out[0].ctypes.data_as(_lib.u64p),
            out[1].ctypes.data_as(_lib.u64p), out[2].ctypes.data_as(_lib.i32p),
            out[3].ctypes.data_as(_lib.f32p)))
        return out

    def set_edge_sampler(self, order=None):
        """The edge sampler enumerating the records in `order` (ordinals; None = ordinal order)."""
        o = None if order is None else _np(order, np.int64)
        if o is not None and len(o) != self.num_edge_records:
            raise ValueError("set_edge_sampler: order must list every ordinal once")
        with self._on_device():
            check(lib().euler_gpu_graph_set_edge_sampler(
                self._h, None if o is None else o.ctypes.data_as(_lib.i64p)))

    def sample_edge(self, count, edge_type=-1, call_id=None):
        """tf_euler sample_edge (tf_euler/kernels/sample_edge_op.cc): [count, 3] int64
        (src, dst, type) drawn by edge weight within the type(s)."""
        et, et_p, k = _i32_array(np.atleast_1d(edge_type))
        out = torch.empty((int(count), 3), dtype=torch.int64, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_sample_edge(
                self._h, _stream(), self.seed, self._take_call_ids(1, call_id), et_p, k,
                int(count), _ptr(out)))
        return out

    def _edges(self, edges):
        e = torch.as_tensor(edges)
        if e.device != self.device or e.dtype != torch.int64:
            e = e.to(device=self.device, dtype=torch.int64)
        return e.reshape(-1, 3).contiguous()

    def edge_ordinals(self, edges):
        """[n, 3] (src, dst, type) -> [n] int64 ordinals, -1 where there is no record."""
        e = self._edges(edges)
        out = torch.empty(e.shape[0], dtype=torch.int64, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_edge_ordinals(self._h, _stream(), _ptr(e), e.shape[0], _ptr(out)))
        return out

    def get_edge_dense_feature(self, edges, feature_ids, dimensions):
        """tf_euler get_edge_dense_feature: list of [n, dim] float32, zeros for unknown edges."""
        e = self._edges(edges)
        n = e.shape[0]
        outs = []
        with self._on_device():
            for fid, dim in zip(feature_ids, dimensions):
                out = torch.empty((n, int(dim)), dtype=torch.float32, device=self.device)
                check(lib().euler_gpu_get_edge_dense_feature(
                    self._h, _stream(), _ptr(e), n, int(fid), int(dim), _ptr(out)))
                outs.append(out)
        return outs

    def get_edge_sparse_feature(self, edges, feature_ids, default_values=None):
        """tf_euler get_edge_sparse_feature: one (indices, values, dense_shape) per feature."""
        e = self._edges(edges)
        n = e.shape[0]
        if default_values is None:
            default_values = [0] * len(feature_ids)
        outs = []
        with self._on_device():
            for fid, dv in zip(feature_ids, default_values):
                row_off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
                nnz, max_len = C.c_int64(0), C.c_int64(0)
                check(lib().euler_gpu_get_edge_sparse_feature(
                    self._h, _stream(), _ptr(e), n, int(fid), int(dv), _ptr(row_off),
                    C.byref(nnz), C.byref(max_len), None, None))
                ind = torch.empty((int(nnz.value), 2), dtype=torch.int64, device=self.device)
                val = torch.empty(int(nnz.value), dtype=torch.int64, device=self.device)
                if nnz.value:
                    check(lib().euler_gpu_get_edge_sparse_feature(
                        self._h, _stream(), _ptr(e), n, int(fid), int(dv), _ptr(row_off),
                        C.byref(nnz), C.byref(max_len), _ptr(ind), _ptr(val)))
                outs.append((ind, val, [n, int(max_len.value)] if n else [0, 0]))
        return outs

    def _binary(self, fn, keys, n, feature_ids):
        outs = []
        with self._on_device():
            for fid in feature_ids:
                off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
                total = C.c_int64(0)
                check(fn(self._h, _stream(), _ptr(keys), n, int(fid), _ptr(off), C.byref(total),
                         None))
                data = torch.empty(max(int(total.value), 1), dtype=torch.uint8, device=self.device)
                if total.value:
                    check(fn(self._h, _stream(), _ptr(keys), n, int(fid), _ptr(off),
                             C.byref(total), _ptr(data)))
                outs.append((off, data[:int(total.value)]))
        return outs

    def get_edge_binary_feature(self, edges, feature_ids):
        """tf_euler get_edge_binary_feature: one (offsets [n+1] int64, bytes uint8) per feature on
        the device; edge i's value is bytes[offsets[i]:offsets[i+1]], empty when unknown."""
        e = self._edges(edges)
        return self._binary(lib().euler_gpu_get_edge_binary_feature, e, e.shape[0], feature_ids)

    def get_binary_feature(self, nodes, feature_ids):
        """tf_euler get_binary_feature over node rows: (offsets, bytes) per feature."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        return self._binary(lib().euler_gpu_get_binary_feature, nodes, nodes.numel(), feature_ids)

    def feature_info(self, name, edge=False):
        """euler.meta's (type, slot, dim) of a feature of a loaded graph; type 0 sparse, 1 dense,
        2 binary."""
        if self.data_path is None:
            raise ValueError("feature names need a graph loaded from a data directory")
        cache = self.__dict__.setdefault("_feature_info", {})
        key = (str(name), bool(edge))
        if key not in cache:
            cache[key] = dat_feature_info(self.data_path, name, edge)
        return cache[key]

    # ------------------------------------------------------------ graph labels
    @staticmethod
    def _label_bytes(labels):
        """(offsets int64 [n + 1], bytes uint8) of a list of str / bytes labels."""
        enc = [x.encode() if isinstance(x, str) else bytes(x) for x in labels]
        off = np.zeros(len(enc) + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in enc], dtype=np.int64)
        data = np.frombuffer(b"".join(enc) or b"\0", np.uint8).copy()
        return off, data

    def set_graph_labels(self, ids, labels):
        """Graph labels by node id (a str / bytes each; "" = no label) for a graph not read from
        .dat; replaces the index.  An id without a row or listed twice raises, and the old index
        stays."""
        ids = _np(np.asarray(ids).reshape(-1), np.uint64)
        if len(labels) != ids.size:
            raise ValueError("set_graph_labels: one label per id")
        off, data = self._label_bytes(labels)
        with self._on_device():
            check(lib().euler_gpu_graph_set_graph_labels(
                self._h, ids.ctypes.data_as(_lib.u64p), ids.size, off.ctypes.data_as(_lib.i64p),
                data.ctypes.data_as(_lib.u8p)))

    @property
    def num_graph_labels(self):
        """Number of distinct graph labels (0 when the graph has none)."""
        with self._on_device():
            n = int(lib().euler_gpu_graph_num_graph_labels(self._h))
        if n < 0:
            check(n)
        return n

    def graph_labels(self):
        """The label table in table order (by each label's smallest node id, DESIGN Q14)."""
        n = self.num_graph_labels
        if n == 0:
            return []
        off = np.zeros(n + 1, np.int64)
        check(lib().euler_gpu_graph_export_graph_labels(self._h, off.ctypes.data_as(_lib.i64p), None))
        data = np.zeros(max(int(off[-1]), 1), np.uint8)
        check(lib().euler_gpu_graph_export_graph_labels(self._h, off.ctypes.data_as(_lib.i64p),
                                                        data.ctypes.data_as(_lib.u8p)))
        b = data.tobytes()
        return [b[off[i]:off[i + 1]].decode("utf-8", "surrogateescape") for i in range(n)]

    def graph_label_ids(self, labels):
        """Table ids of labels (str / bytes) as int64 numpy, -1 for an unknown label."""
        off, data = self._label_bytes(labels)
        out = np.zeros(len(labels), np.int64)
        with self._on_device():
            check(lib().euler_gpu_graph_label_ids(
                self._h, len(labels), off.ctypes.data_as(_lib.i64p), data.ctypes.data_as(_lib.u8p),
                out.ctypes.data_as(_lib.i64p)))
        return out

    def label_index_info(self):
        """(labelled nodes, device bytes of the label index)."""
        n, b = C.c_int64(0), C.c_int64(0)
        with self._on_device():
            check(lib().euler_gpu_graph_label_index_info(self._h, C.byref(n), C.byref(b)))
        return int(n.value), int(b.value)

    def sample_graph_label(self, count, call_id=None):
        """tf_euler sample_graph_label as table ids: [count] int64 on the device, uniform with
        replacement (RNG domain 7)."""
        out = torch.empty(int(count), dtype=torch.int64, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_sample_graph_label(
                self._h, _stream(), self.seed, self._take_call_ids(1, call_id), int(count),
                _ptr(out)))
        return out

    def _label_id_tensor(self, labels):
        if torch.is_tensor(labels):
            return _as_i64_cuda(labels, self.device).reshape(-1)
        labels = list(labels)
        if all(isinstance(x, (str, bytes)) for x in labels):
            return torch.as_tensor(self.graph_label_ids(labels)).to(self.device)
        return _as_i64_cuda(np.asarray(labels, np.int64), self.device).reshape(-1)

    def get_graph_by_label_core(self, labels):
        """(idx [B, 2] int32 (start, end), node ids int64) of API_GET_GRAPH_BY_LABEL."""
        ids = self._label_id_tensor(labels)
        n = ids.numel()
        idx = torch.empty((n, 2), dtype=torch.int32, device=self.device)
        total = C.c_int64(0)
        with self._on_device():
            check(lib().euler_gpu_get_graph_by_label(self._h, _stream(), _ptr(ids), n, _ptr(idx),
                                                     C.byref(total), None))
            out = torch.empty(int(total.value), dtype=torch.int64, device=self.device)
            if total.value:
                check(lib().euler_gpu_get_graph_by_label(self._h, _stream(), _ptr(ids), n, _ptr(idx),
                                                         C.byref(total), _ptr(out)))
        return idx, out

    def get_graph_by_label(self, labels):
        """tf_euler get_graph_by_label (tf_euler/kernels/get_graph_by_label_op.cc): the
        SparseTensor triple (indices [nnz, 2] (i, j), values int64, dense_shape) of labels (str /
        bytes, or table ids).  A label with no nodes gives the single entry (i, 0) = 0; dense_shape
        is [B, max(len, 1)], [0, 0] for B = 0."""
        idx, ids = self.get_graph_by_label_core(labels)
        return _label_triple(idx, ids)

    def whole_graph_block(self, n_id, edge_types, add_self_loops=True):
        """edge_index [2, E (+ N)] int64 of WholeDataFlow (whole_dataflow.py:37-63, DESIGN Q16):
        (j, c) for every listed-type edge n_id[j] -> n_id[c], sorted by j then c, then the self
        loops (i, i).  One library call when the capacity suffices, a second with room when not."""
        n_id = _as_i64_cuda(n_id, self.device).reshape(-1)
        n = n_id.numel()
        et, et_p, k = _i32_array(edge_types)
        cap = self.__dict__.get("_block_cap", 0)
        cap = max(cap, 8 * n + 64)
        total = C.c_int64(0)
        with self._on_device():
            for _ in range(2):
                out = torch.empty((2, cap), dtype=torch.int64, device=self.device)
                check(lib().euler_gpu_whole_graph_block(
                    self._h, _stream(), _ptr(n_id), n, et_p, k, 1 if add_self_loops else 0, cap,
                    C.byref(total), _ptr(out)))
                if total.value <= cap:
                    break
                cap = int(total.value)
            self._block_cap = max(self.__dict__.get("_block_cap", 0), int(total.value))
        return out[:, :int(total.value)]

    def graph_batch(self, count_or_labels, edge_types, add_self_loops=True, call_id=None):
        """One minibatch of whole-graph classification (graph_estimator.get_train_from_input +
        the whole-graph block): (label ids int64, n_id int64, node_graph_idx int64,
        edge_index [2, E (+ N)] int64).  n_id and node_graph_idx are the get_graph_by_label
        triple's values and indices[:, 0], as the reference reads them: a label without nodes
        contributes its fill entry (node 0, its own row).  An int draws that many labels
        (sample_graph_label); otherwise the labels (str / bytes or table ids) are used as given."""
        if isinstance(count_or_labels, (int, np.integer)):
            label_ids = self.sample_graph_label(int(count_or_labels), call_id)
        else:
            label_ids = self._label_id_tensor(count_or_labels)
        ind, n_id, _shape = self.get_graph_by_label(label_ids)
        node_graph_idx = ind[:, 0]
        edge_index = self.whole_graph_block(n_id, edge_types, add_self_loops)
        return label_ids, n_id, node_graph_idx, edge_index

    _ORDER = {None: 0, "": 0, "id": 1, "weight": 2}

    def get_full_neighbor(self, nodes, edge_types, order_by=None, desc=False,
                          limit=None):
        """GQL `v(nodes).outV(edge_types)[.order_by(f, asc|desc)][.limit(k)]`
        result (idx [n,2] int32, ids int64, weights f32, types int32),
        core/kernels/get_neighbor_op.cc (post-process :117-168)."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        n = nodes.numel()
        et, et_p, k = _i32_array(edge_types)
        idx = torch.empty((n, 2), dtype=torch.int32, device=self.device)
        total = C.c_int64(0)
        with self._on_device():
            check(lib().euler_gpu_get_full_neighbor(
                self._h, _stream(), _ptr(nodes), n, et_p, k, _ptr(idx),
                C.byref(total), None, None, None))
            tot = int(total.value)
            ids = torch.empty(tot, dtype=torch.int64, device=self.device)
            w = torch.empty(tot, dtype=torch.float32, device=self.device)
            t = torch.empty(tot, dtype=torch.int32, device=self.device)
            if n:
                check(lib().euler_gpu_get_full_neighbor(
                    self._h, _stream(), _ptr(nodes), n, et_p, k, _ptr(idx),
                    C.byref(total), _ptr(ids), _ptr(w), _ptr(t)))
            if n and (self._ORDER[order_by] or limit is not None):
                new_total = C.c_int64(0)
                check(lib().euler_gpu_neighbor_post_process(
                    _stream(), n, _ptr(idx), tot, _ptr(ids), _ptr(w), _ptr(t),
                    self._ORDER[order_by], 1 if desc else 0,
                    -1 if limit is None else int(limit), C.byref(new_total)))
                m = int(new_total.value)
                ids, w, t = ids[:m], w[:m], t[:m]
        return idx, ids, w, t

    # ------------------------------------------------- full-neighbour aggregation
    def _neighbor_degree(self, nodes, edge_types, self_loop, as_norm):
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        n = nodes.numel()
        et, et_p, k = _i32_array(edge_types)
        out = torch.empty(n, dtype=torch.float32 if as_norm else torch.int32, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_neighbor_degree(self._h, _stream(), _ptr(nodes), n, et_p, k,
                                                  1 if self_loop else 0, 1 if as_norm else 0, _ptr(out)))
        return out

    def neighbor_degree(self, nodes, edge_types, self_loop=False):
        """int32 [n]: the number of stored neighbours of every node over the listed edge types,
        as get_full_neighbor lists them (a type listed twice counts twice, an unknown id has
        none); self_loop adds 1.  One small kernel, no host wait."""
        return self._neighbor_degree(nodes, edge_types, self_loop, False)

    def neighbor_norm(self, nodes, edge_types, self_loop=False):
        """float32 [n]: 1 / sqrt(neighbor_degree), 0 at degree 0 - ops.gcn_norm's rule and bits."""
        return self._neighbor_degree(nodes, edge_types, self_loop, True)

    def full_neighbor_segments(self, nodes, edge_types, self_loop=False):
        """(seg_ptr int64 [n + 1], ids int64, weights float32) of get_full_neighbor's lists as the
        segment ops take them; self_loop appends every node's own id with weight 1 to its
        segment.  The list neighbor_aggregate does NOT build: 16 bytes per listed edge and a
        host wait, fewer than 2^31 entries a call."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        n = nodes.numel()
        idx, ids, w, _t = self.get_full_neighbor(nodes, edge_types)
        lens = (idx[:, 1] - idx[:, 0]).to(torch.int64)
        seg_ptr = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        if not self_loop:
            torch.cumsum(lens, 0, out=seg_ptr[1:])
            return seg_ptr, ids, w
        torch.cumsum(lens + 1, 0, out=seg_ptr[1:])
        owner = torch.repeat_interleave(torch.arange(n, device=self.device), lens)
        place = torch.arange(ids.numel(), device=self.device) + owner
        all_ids = torch.empty(ids.numel() + n, dtype=torch.int64, device=self.device)
        all_w = torch.ones(ids.numel() + n, dtype=torch.float32, device=self.device)
        all_ids[place] = ids
        all_w[place] = w
        all_ids[seg_ptr[1:] - 1] = nodes
        return seg_ptr, all_ids, all_w

    def _aggregate_composed(self, op, table, nodes, edge_types, kind, norm, self_loop, root, a, b, od):
        from . import ops
        n, rows = nodes.numel(), table.shape[0]
        seg_ptr, ids, w = self.full_neighbor_segments(nodes, edge_types, self_loop)
        if kind == "norm" and op != "max":
            # ops.gcn_aggregate with the scales (a, b) already formed (it refuses max: below)
            if op == "mean" and ids.numel() >= (1 << 24):
                raise ValueError("neighbor_aggregate_composed: a mean needs fewer than 2^24 listed edges")
            return ops._GcnAggregate.apply(table, root, None, ids.to(torch.int32).contiguous(), seg_ptr, 0, n,
                                           norm[0], norm[1], op, a, b, od)
        if kind == "norm":
            g = ids & 0xFFFFFFFF
            owner = torch.repeat_interleave(torch.arange(n, device=self.device), seg_ptr[1:] - seg_ptr[:-1])
            w = torch.where(g < rows, norm[0][owner] * norm[1][torch.clamp(g, max=rows - 1)],
                            torch.zeros((), dtype=torch.float32, device=self.device))
        mid = od if root is None else torch.float32
        agg = ops.gather_segment_reduce(op, table, ids, n, seg_ptr=seg_ptr, out_dtype=mid,
                                        edge_weight=None if kind is None else w)
        if root is None:
            return agg
        return (agg * a + root.float() * b).to(od)

    def neighbor_aggregate_composed(self, op, table, nodes, edge_types, weight=None, norm=None, self_loop=False,
                                    root=None, alpha=None, root_scale=None, out_dtype=None):
        """neighbor_aggregate as the composition of the existing ops - get_full_neighbor (two calls
        and a host wait), the list with the self ids appended, then ops.gather_segment_reduce or
        ops.gcn_aggregate: what neighbor_aggregate equals bit for bit, and what its backward pass
        runs.  Same arguments; the list must have fewer than 2^31 entries."""
        table, nodes, norm, root, a, b, od = self._aggregate_args(
            "neighbor_aggregate_composed", op, table, nodes, edge_types, weight, norm, self_loop, root, alpha,
            root_scale, out_dtype)
        return self._aggregate_composed(op, table, nodes, edge_types, weight, norm, self_loop, root, a, b, od)

    def _aggregate_args(self, name, op, table, nodes, edge_types, weight, norm, self_loop, root, alpha, root_scale,
                        out_dtype):
        from . import ops
        if op not in _NB_MODE:
            raise ValueError("%s: op is add, max or mean" % name)
        if weight not in _NB_KIND:
            raise ValueError("%s: weight is None, 'edge' or 'norm'" % name)
        ops._dt(name, table)
        od = ops._out_dt(name, table, out_dtype)
        ops._need_cuda(table)
        if table.dim() != 2 or table.shape[0] < 1:
            raise ValueError("%s: table is [rows, D] with at least one row, indexed by node id" % name)
        if not table.is_contiguous():
            table = table.contiguous()
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        n = nodes.numel()
        if weight == "norm":
            if norm is None:
                norm = (self.neighbor_norm(nodes, edge_types, self_loop),
                        self.neighbor_norm(torch.arange(table.shape[0], device=self.device), edge_types, self_loop))
            nd, ns = norm
            for t, m, side in ((nd, n, "norm_dst"), (ns, table.shape[0], "norm_src")):
                if t.dtype != torch.float32:
                    raise TypeError("%s: %s is float32, not %s" % (name, side, t.dtype))
                if t.dim() != 1 or t.numel() != m:
                    raise ValueError("%s: %s has %d entries, not %s" % (name, side, m, tuple(t.shape)))
                ops._need_cuda(t)
            norm = (nd.detach().contiguous(), ns.detach().contiguous())
        elif norm is not None:
            raise ValueError("%s: norm comes with weight='norm'" % name)
        a, b = 1.0, 1.0
        if alpha is not None:
            if root is None:
                raise ValueError("%s: alpha needs root" % name)
            a, b = 1.0 - float(alpha), float(alpha)
        if root_scale is not None:
            if root is None:
                raise ValueError("%s: root_scale needs root" % name)
            b = float(root_scale)
        if root is not None:
            if root.dtype != torch.float32 and root.dtype != table.dtype:
                raise TypeError("%s: root is float32 or the dtype of table (%s), not %s"
                                % (name, table.dtype, root.dtype))
            if root.dim() != 2 or tuple(root.shape) != (n, table.shape[1]):
                raise ValueError("%s: root is [n, D] = %s, not %s" % (name, (n, table.shape[1]), tuple(root.shape)))
            ops._need_cuda(root)
            root = root.contiguous()
            # the scales as the fp32 numbers the kernel multiplies by
            a, b = float(np.float32(a)), float(np.float32(b))
        return table, nodes, norm, root, a, b, od

    def neighbor_aggregate(self, op, table, nodes, edge_types, weight=None, norm=None, self_loop=False, root=None,
                           alpha=None, root_scale=None, out_dtype=None):
        """[n, D]: every node's reduce (op "add" / "max" / "mean") of the table rows of its stored
        (full) neighbours over the listed edge types, read straight from the graph's rows in one
        kernel (euler_gpu_neighbor_reduce): SGCN's S^K X, an APPNP step, a GCN layer over full
        neighbours, the embeddings of all nodes after training.  The bits of get_full_neighbor
        followed by ops.gather_segment_reduce / ops.gcn_aggregate (neighbor_aggregate_composed),
        without the [E] list, without a host wait and without the 2^31 limit on E.
        table is [rows, D] (fp32 / bf16 / fp16), indexed by node id: a neighbour id at or past
        `rows` reads the last row (and has weight 0 under weight="norm").  weight None: the plain
        reduce; "edge": every message times its edge's weight; "norm": times norm_dst[i] *
        norm_src[j], norm = (norm_dst [n], norm_src [rows]) fp32 - None computes them from the
        listed degrees (neighbor_norm of `nodes` and of the ids 0 .. rows - 1).  self_loop appends
        the node's own row (weight 1, or its norm product); it counts in a mean.  root [n, D] adds
        out = agg * a + root * b in the same pass; alpha and root_scale as ops.gcn_aggregate.
        out_dtype None = the table's dtype, or torch.float32.
        Gradients flow to table and root only.  The backward pass rebuilds the list with
        get_full_neighbor and differentiates the composition, re-running its forward: it costs the
        [E] list and a host wait, and happens only when a gradient is asked for."""
        table, nodes, norm, root, a, b, od = self._aggregate_args(
            "neighbor_aggregate", op, table, nodes, edge_types, weight, norm, self_loop, root, alpha, root_scale,
            out_dtype)
        return _NeighborAggregate.apply(table, root, self, nodes, edge_types, op, weight, bool(self_loop), norm,
                                        a, b, od)

    def get_sorted_full_neighbor(self, nodes, edge_types):
        """tf_euler get_sorted_full_neighbor: rows ordered by neighbour id
        (tf_euler/kernels/get_sorted_full_neighbor_op.cc:43-46)."""
        return self.get_full_neighbor(nodes, edge_types, order_by="id")

    def get_top_k_neighbor(self, nodes, edge_types, k, default_node=-1):
        """tf_euler get_top_k_neighbor (tf_euler/kernels/get_top_k_neighbor_op.cc):
        the k heaviest neighbours per node as dense [n, k] tensors (ids int64,
        weights f32, types int32), default_node / 0.0 / -1 where a node has
        fewer."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        n = nodes.numel()
        et, et_p, k_types = _i32_array(edge_types)
        out_n = torch.empty((n, k), dtype=torch.int64, device=self.device)
        out_w = torch.empty((n, k), dtype=torch.float32, device=self.device)
        out_t = torch.empty((n, k), dtype=torch.int32, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_get_top_k_neighbor(
                self._h, _stream(), _ptr(nodes), n, et_p, k_types, int(k),
                int(default_node), _ptr(out_n), _ptr(out_w), _ptr(out_t)))
        return out_n, out_w, out_t

    def get_node_type(self, nodes):
        """tf_euler get_node_type (tf_euler/kernels/get_node_type_op.cc): int32
        type of every node, INT32_MIN for an unknown id."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        n = nodes.numel()
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_get_node_type(self._h, _stream(), _ptr(nodes), n,
                                                _ptr(out)))
        return out

    def sample_n_with_types(self, count, types, call_id=None):
        """tf_euler sample_n_with_types (tf_euler/kernels/
        sample_n_with_types_op.cc): [len(types), count] int64, row i drawn from
        the global sampler of node type types[i] (-1: all types).  Raises where
        the reference aborts (unknown / zero-weight type)."""
        types = torch.as_tensor(types, dtype=torch.int32, device=self.device) \
            .reshape(-1).contiguous()
        n = types.numel()
        out = torch.empty((n, int(count)), dtype=torch.int64, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_sample_n_with_types(
                self._h, _stream(), self.seed, self._take_call_ids(1, call_id),
                _ptr(types), n, int(count), _ptr(out)))
        return out

    # ------------------------------------------------- layerwise sampling
    def get_edge_sum_weight(self, nodes, edge_types):
        """API_GET_EDGE_SUM_WEIGHT (core/kernels/get_edge_sum_weight_op.cc):
        f32 sum of each node's out-edge weights over the listed types."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        n = nodes.numel()
        et, et_p, k = _i32_array(edge_types)
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_get_edge_sum_weight(
                self._h, _stream(), _ptr(nodes), n, et_p, k, _ptr(out)))
        return out

    def sample_root(self, roots, weights, m, default_node=-1, call_id=None):
        """API_SAMPLE_ROOT (core/kernels/sample_root_op.cc): roots / weights
        [batch, n] -> [batch, m] draws (alias method per batch row)."""
        roots = _as_i64_cuda(roots, self.device)
        batch, n = roots.shape
        weights = torch.as_tensor(weights, dtype=torch.float32,
                                  device=self.device).reshape(batch, n).contiguous()
        out = torch.empty((batch, int(m)), dtype=torch.int64, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_sample_root(
                _stream(), self.seed, self._take_call_ids(1, call_id), _ptr(roots),
                _ptr(weights), batch, n, int(m), int(default_node), _ptr(out)))
        return out

    def sample_layer(self, roots, edge_types, default_node=-1, call_id=None, positions=None):
        """API_SAMPLE_L (core/kernels/sample_layer_op.cc): one neighbour per
        listed root (position-keyed RNG) or (default_node, 0.0, 0).  positions:
        the RNG stream of every root (default: its index) - what the shard of a
        multi-GPU hop receives from the requester."""
        roots = _as_i64_cuda(roots, self.device).reshape(-1)
        n = roots.numel()
        if positions is not None:
            positions = _as_i64_cuda(positions, self.device).reshape(-1)
            assert positions.numel() == n
        et, et_p, k = _i32_array(edge_types)
        oid = torch.empty(n, dtype=torch.int64, device=self.device)
        ow = torch.empty(n, dtype=torch.float32, device=self.device)
        ot = torch.empty(n, dtype=torch.int32, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_sample_layer_at(
                self._h, _stream(), self.seed, self._take_call_ids(1, call_id),
                _ptr(roots), _ptr(positions), n, et_p, k, int(default_node), _ptr(oid),
                _ptr(ow), _ptr(ot)))
        return oid, ow, ot

    def local_sample_layer(self, idx, ids, w, t, batch, n, m, weight_func="sqrt",
                           default_node=-1, call_id=None):
        """API_LOCAL_SAMPLE_L (core/kernels/local_sample_layer_op.cc): m draws
        per batch row from the distinct (id, type) full neighbours of its n
        nodes, weights of duplicates added and transformed by weight_func;
        (ids, weights, types) each [batch * m]."""
        idx = idx.to(torch.int32).contiguous()
        ids = ids.to(torch.int64).contiguous()
        w = w.to(torch.float32).contiguous()
        t = t.to(torch.int32).contiguous()
        total = ids.numel()
        oid = torch.empty(batch * m, dtype=torch.int64, device=self.device)
        ow = torch.empty(batch * m, dtype=torch.float32, device=self.device)
        ot = torch.empty(batch * m, dtype=torch.int32, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_local_sample_layer(
                _stream(), self.seed, self._take_call_ids(1, call_id), _ptr(idx),
                _ptr(ids), _ptr(w), _ptr(t), total, batch, n, m,
                str(weight_func).encode(), int(default_node), _ptr(oid), _ptr(ow),
                _ptr(ot)))
        return oid, ow, ot

    def sparse_get_adj_core(self, roots, l_nb, n, m, edge_types):
        """API_SPARSE_GEN_ADJ + API_SPARSE_GET_ADJ (core/kernels/
        sparse_get_adj_op.cc): (idx [batch*n, 2] int32, ids int64)."""
        roots = _as_i64_cuda(roots, self.device).reshape(-1)
        l_nb = _as_i64_cuda(l_nb, self.device).reshape(-1)
        n, m = int(n), int(m)
        batch = roots.numel() // n if n else 0
        assert roots.numel() == batch * n and l_nb.numel() == batch * m
        et, et_p, k = _i32_array(edge_types)
        idx = torch.empty((batch * n, 2), dtype=torch.int32, device=self.device)
        ws = self._adj_workspace(batch, n, m)
        total = C.c_int64(0)
        with self._on_device():
            check(lib().euler_gpu_sparse_get_adj(
                self._h, _stream(), _ptr(roots), _ptr(l_nb), batch, n, m, et_p, k,
                _ptr(ws), _ptr(idx), C.byref(total), None))
            vals = torch.empty(int(total.value), dtype=torch.int64, device=self.device)
            if total.value:
                check(lib().euler_gpu_sparse_get_adj(
                    self._h, _stream(), _ptr(roots), _ptr(l_nb), batch, n, m, et_p, k,
                    _ptr(ws), _ptr(idx), C.byref(total), _ptr(vals)))
        return idx, vals

    def _adj_workspace(self, batch, n, m):
        """Scratch of a SparseGetAdj query (offsets + one bit per pair), kept
        between its two calls."""
        nbytes = int(lib().euler_gpu_sparse_get_adj_workspace(batch, n, m))
        return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=self.device)

    def sparse_get_adj(self, nodes, nb_nodes, edge_types, n=-1, m=-1):
        """tf_euler sparse_get_adj (tf_euler/kernels/sparse_get_adj_op.cc):
        COO (indices [nnz, 3] int64, values [nnz] int64, dense_shape) of the
        [batch, n, m] adjacency between nodes [batch*n] and nb_nodes
        [batch*m]; n / m = -1 take the whole input as one batch row."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        nb_nodes = _as_i64_cuda(nb_nodes, self.device).reshape(-1)
        n = nodes.numel() if n == -1 else int(n)
        m = nb_nodes.numel() if m == -1 else int(m)
        batch = nodes.numel() // n if n else 0
        if nodes.numel() != batch * n or nb_nodes.numel() < batch * m:
            raise ValueError("sparse_get_adj: nodes / nb_nodes do not match n, m")
        et, et_p, k = _i32_array(edge_types)
        row_off = self._adj_workspace(batch, n, m)
        nnz = C.c_int64(0)
        with self._on_device():
            check(lib().euler_gpu_sparse_get_adj_tf(
                self._h, _stream(), _ptr(nodes), _ptr(nb_nodes), batch, n, m, et_p, k,
                _ptr(row_off), C.byref(nnz), None, None))
            ind = torch.empty((int(nnz.value), 3), dtype=torch.int64, device=self.device)
            val = torch.empty(int(nnz.value), dtype=torch.int64, device=self.device)
            if nnz.value:
                check(lib().euler_gpu_sparse_get_adj_tf(
                    self._h, _stream(), _ptr(nodes), _ptr(nb_nodes), batch, n, m, et_p,
                    k, _ptr(row_off), C.byref(nnz), _ptr(ind), _ptr(val)))
        shape = [batch, n, m] if nnz.value else [0, 0, 0]
        return ind, val, shape

    def sparse_adj_mask(self, nodes, nb_nodes, batch, n, m, edge_types):
        """The hit mask of SparseGetAdj on THIS graph (shard): int64 [batch * n, (m + 63) // 64],
        bit c of a source = candidate c of its batch row is in the source's row; sources
        without a row here give zeros (euler_gpu_sparse_adj_mask)."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        nb_nodes = _as_i64_cuda(nb_nodes, self.device).reshape(-1)
        words = (int(m) + 63) // 64
        mask = torch.zeros((int(batch) * int(n), words), dtype=torch.int64, device=self.device)
        et, et_p, k = _i32_array(edge_types)
        if mask.numel():
            with self._on_device():
                check(lib().euler_gpu_sparse_adj_mask(
                    self._h, _stream(), _ptr(nodes), _ptr(nb_nodes), int(batch), int(n), int(m),
                    et_p, k, _ptr(mask)))
        return mask

    @staticmethod
    def adj_from_mask(mask, batch, n, m):
        """TF SparseGetAdj triple (indices [nnz, 3], values, dense_shape) from a hit mask
        (euler_gpu_sparse_adj_from_mask_tf) - needs no graph."""
        dev = mask.device
        batch, n, m = int(batch), int(n), int(m)
        mask = mask.contiguous()
        ws = torch.empty(8 * (batch * n + 1) + 16, dtype=torch.uint8, device=dev)
        nnz = C.c_int64(0)
        with torch.cuda.device(dev):
            check(lib().euler_gpu_sparse_adj_from_mask_tf(
                _stream(), _ptr(mask), batch, n, m, _ptr(ws), C.byref(nnz), None, None))
            ind = torch.empty((int(nnz.value), 3), dtype=torch.int64, device=dev)
            val = torch.empty(int(nnz.value), dtype=torch.int64, device=dev)
            if nnz.value:
                check(lib().euler_gpu_sparse_adj_from_mask_tf(
                    _stream(), _ptr(mask), batch, n, m, _ptr(ws), C.byref(nnz), _ptr(ind), _ptr(val)))
        return ind, val, ([batch, n, m] if nnz.value else [0, 0, 0])

    def sample_neighbor_layerwise(self, nodes, edge_types, count, default_node=-1,
                                  weight_func='', call_id=None):
        """tf_euler sample_neighbor_layerwise (euler_ops/neighbor_ops.py:72-77
        over tf_euler/kernels/sample_neighbor_layerwise_with_adj_op.cc):
        nodes [batch, n] -> (neighbors [batch, count] int64, (indices, values,
        dense_shape) of the [batch, n, count] adjacency).  weight_func == ''
        draws a node of the layer by edge weight sum, then one of its
        neighbours; 'sqrt' draws from the layer's distinct neighbours by the
        square root of their accumulated weight."""
        nodes = _as_i64_cuda(nodes, self.device)
        if nodes.dim() != 2:
            raise ValueError("sample_neighbor_layerwise: nodes must be [batch, n]")
        batch, n = nodes.shape
        et, et_p, k = _i32_array(edge_types)
        if weight_func:
            # sampleLNB(edge_types, n, m, weight_func, default_node): API_GET_NB_NODE
            # -> API_LOCAL_SAMPLE_L (parser/translator.cc:388-441)
            idx, ids, w, t = self.get_full_neighbor(nodes.reshape(-1), et)
            out, _w, _t = self.local_sample_layer(idx, ids, w, t, batch, n, int(count),
                                                  weight_func, default_node, call_id)
            out = out.reshape(batch, int(count))
            return out, self.sparse_get_adj(nodes, out, et, n, int(count))
        out = torch.empty((batch, int(count)), dtype=torch.int64, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_sample_neighbor_layerwise(
                self._h, _stream(), self.seed, self._take_call_ids(1, call_id),
                _ptr(nodes), batch, n, et_p, k, int(count), int(default_node),
                _ptr(out)))
        return out, self.sparse_get_adj(nodes, out, et, n, int(count))

    def random_walk(self, nodes, edge_types, p=1.0, q=1.0, default_node=-1,
                    call_id=None):
        """tf_euler random_walk (tf_euler/kernels/random_walk_op.cc):
        edge_types = list (length walk_len) of per-step edge type lists;
        returns [n, walk_len+1] int64."""
        nodes = _as_i64_cuda(nodes, self.device).reshape(-1)
        walk_len = len(edge_types)
        et = np.asarray(edge_types, dtype=np.int32).reshape(walk_len, -1) \
            if walk_len else np.zeros((0, 0), np.int32)
        k = et.shape[1] if walk_len else 0
        et, et_p, _ = _i32_array(et)
        n = nodes.numel()
        out = torch.empty((n, walk_len + 1), dtype=torch.int64, device=self.device)
        with self._on_device():
            check(lib().euler_gpu_random_walk(
                self._h, _stream(), self.seed,
                self._take_call_ids(max(walk_len, 1), call_id), _ptr(nodes), n,
                et_p, k, walk_len, float(p), float(q), int(default_node),
                _ptr(out)))
        return out
