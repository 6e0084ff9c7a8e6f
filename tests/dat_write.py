"""Writes a data directory with node FEATURES in the reference's on-disk layout (test helper):
euler.meta with the feature name tables (graph_builder.cc:230-307) and Node/data_<p>.dat records
with their uint64, float and binary slots (Node::DeSerialize, node.cc:414-526).  Every node gets
one out-edge of type 0 and weight 1 to the next node, so that the directory is a loadable graph.
tests/test_host.py's write_dat_dir writes adjacency and leaves every feature vector empty."""
import os
import struct

import numpy as np

SPARSE, DENSE, BINARY = 0, 1, 2          # euler.meta's feature types
_PREFIX = {SPARSE: "sparse_", DENSE: "dense_", BINARY: "binary_"}


def _vec(dtype, values):
    a = np.ascontiguousarray(values, dtype).reshape(-1)
    return struct.pack("<I", len(a)) + a.tobytes()


def _str(b):
    b = b.encode() if isinstance(b, str) else bytes(b)
    return struct.pack("<I", len(b)) + b


def _slots(dtype, slots):
    """(the slot ends, all values): the idx / value pair of one feature kind of one record."""
    vals = [np.frombuffer(v, np.uint8) if isinstance(v, (bytes, bytearray)) else np.asarray(v, dtype)
            for v in slots]
    ends = np.cumsum([v.size for v in vals]) if vals else []
    flat = np.concatenate(vals) if vals else np.zeros(0, dtype)
    return _vec("<i4", ends), flat.astype(dtype)


def feature_table(n_float, n_u64, n_binary, float_dims=None, u64_dims=None):
    """Names f<kind letter><slot> -> (type, slot, dim) in the order euler.meta lists them."""
    out = []
    for s in range(n_u64):
        out.append(("sparse_fs%d" % s, SPARSE, s, int(u64_dims[s]) if u64_dims else 0))
    for s in range(n_float):
        out.append(("dense_fd%d" % s, DENSE, s, int(float_dims[s]) if float_dims else 0))
    for s in range(n_binary):
        out.append(("binary_fb%d" % s, BINARY, s, 0))
    return out


def write_feature_dat_dir(path, ids, floats=None, u64s=None, binaries=None, partitions=2,
                          node_type=None, node_weight=None):
    """ids [n]; floats / u64s / binaries: per node a list of slots (sequences; `bytes` for
    binary), or None for a kind the graph does not have.  Node i goes to file id % partitions.
    Returns the feature name table written to euler.meta."""
    path = str(path)
    os.makedirs(os.path.join(path, "Node"), exist_ok=True)
    ids = np.asarray(ids, np.uint64)
    n = len(ids)
    nt = np.zeros(n, np.int32) if node_type is None else np.asarray(node_type, np.int32)
    nw = np.ones(n, np.float32) if node_weight is None else np.asarray(node_weight, np.float32)
    width = lambda per: max((len(x) for x in per), default=0) if per is not None else 0   # noqa: E731
    dims = lambda per, k: [max(len(x[s]) if s < len(x) else 0 for x in per) for s in range(k)]   # noqa: E731
    n_f, n_u, n_b = width(floats), width(u64s), width(binaries)
    names = feature_table(n_f, n_u, n_b, dims(floats, n_f) if n_f else None,
                          dims(u64s, n_u) if n_u else None)
    meta = _str("g") + _str("1") + struct.pack("<QQi", n, n, partitions)
    meta += struct.pack("<I", len(names))
    for name, kind, slot, dim in names:
        meta += _str(name) + struct.pack("<iiq", kind, slot, dim)
    meta += struct.pack("<I", 0)                                   # no edge features
    n_nt = int(nt.max()) + 1 if n else 1
    meta += struct.pack("<I", n_nt) + b"".join(_str(str(i)) + struct.pack("<I", i) for i in range(n_nt))
    meta += struct.pack("<I", 1) + _str("0") + struct.pack("<I", 0)
    with open(os.path.join(path, "euler.meta"), "wb") as f:
        f.write(meta)
    files = [[] for _ in range(partitions)]
    none = _vec("<i4", [])
    for r in range(n):
        rec = struct.pack("<Qif", int(ids[r]), int(nt[r]), float(nw[r]))
        # one edge group: type 0, weight 1, one neighbour (the next node)
        rec += _vec("<i4", [0]) + _vec("<f4", [1.0]) + _vec("<i4", [1])
        rec += _vec("<u8", [ids[(r + 1) % n]]) + _vec("<f4", [1.0])
        rec += none * 5                                            # no in-neighbours
        for per, dtype in ((u64s, "<u8"), (floats, "<f4")):
            ends, flat = _slots(dtype, per[r] if per is not None else [])
            rec += ends + _vec(dtype, flat)
        ends, flat = _slots(np.uint8, binaries[r] if binaries is not None else [])
        rec += ends + _str(flat.tobytes())
        files[int(ids[r]) % partitions].append(struct.pack("<I", len(rec)) + rec)
    for p in range(partitions):
        with open(os.path.join(path, "Node", "data_%d.dat" % p), "wb") as f:
            f.write(b"".join(files[p]))
    return names
