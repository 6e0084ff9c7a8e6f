"""The contract of Graph.from_edges restated in numpy, and the case table of its tests.

`reference(case)` lays an edge list out by the reference's rules - the rows, the stable grouping by
(row, type), Node::Init's sequential fp32 sums (np.float32 adds in a Python loop, one add at a time:
no cumsum, no pairwise sum), the three flags of the build and the id map's kind - and returns what
`Graph.from_csr` takes.  tests/test_graph_from_edges_host.py holds it against the C restatement of
Node::Init (oracle.csr_from_raw); tests/test_graph_from_edges_gpu.py builds both graphs from it.

A case is a dict of numpy arrays: src, dst (uint64), edge_type (int32 or None), weight (float32 or
None), n_edge_types, nodes (uint64 or None), node_type, node_weight, features (list of [N, d]
float32 or None), undirected.  Cases are built once and never written to."""
import functools

import numpy as np

U64 = np.uint64
BIG = np.float32(2.0 ** 24)


def case(src, dst, edge_type=None, weight=None, n_edge_types=None, nodes=None, node_type=None,
         node_weight=None, features=None, undirected=False):
    src = np.asarray(src, dtype=U64).reshape(-1)
    dst = np.asarray(dst, dtype=U64).reshape(-1)
    if edge_type is not None:
        edge_type = np.asarray(edge_type, dtype=np.int32).reshape(-1)
    if weight is not None:
        weight = np.asarray(weight, dtype=np.float32).reshape(-1)
    if n_edge_types is None:
        n_edge_types = int(edge_type.max()) + 1 if edge_type is not None and len(edge_type) else 1
    if nodes is not None:
        nodes = np.asarray(nodes, dtype=U64).reshape(-1)
    if node_type is not None:
        node_type = np.asarray(node_type, dtype=np.int32)
    if node_weight is not None:
        node_weight = np.asarray(node_weight, dtype=np.float32)
    c = dict(src=src, dst=dst, edge_type=edge_type, weight=weight, n_edge_types=int(n_edge_types),
             nodes=nodes, node_type=node_type, node_weight=node_weight, features=features,
             undirected=bool(undirected))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return c


def edge_list(c):
    """(src, dst, type, weight) of the list the build sees: the edges, then - undirected - all of them
    reversed; a missing type is 0, a missing weight 1.0f"""
    src, dst = c["src"], c["dst"]
    t = c["edge_type"] if c["edge_type"] is not None else np.zeros(len(src), np.int32)
    w = c["weight"] if c["weight"] is not None else np.ones(len(src), np.float32)
    if c["undirected"]:
        return (np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([t, t]),
                np.concatenate([w, w]))
    return src, dst, t, w


def layout(c):
    """The rows and the grouped entries with RAW weights: (row_id [N] u64, seg_ptr [N * T + 1] i64,
    nbr [E] u64, w [E] f32) - what oracle.csr_from_raw takes."""
    src, dst, t, w = edge_list(c)
    T = c["n_edge_types"]
    if c["nodes"] is not None:
        row_id = c["nodes"]
    else:
        row_id = np.unique(np.concatenate([src, dst]))        # uint64: ascending as unsigned numbers
    row_of = {int(x): r for r, x in enumerate(row_id.tolist())}
    assert len(row_of) == len(row_id), "an id twice in nodes"
    rows = np.array([row_of[int(s)] for s in src.tolist()], dtype=np.int64)
    assert len(t) == 0 or (t.min() >= 0 and t.max() < T)
    key = rows * T + t.astype(np.int64)
    order = np.argsort(key, kind="stable")
    seg_ptr = np.searchsorted(key[order], np.arange(len(row_id) * T + 1), side="left").astype(np.int64)
    return row_id, seg_ptr, dst[order].astype(U64), w[order].astype(np.float32)


def node_init(n_rows, T, seg_ptr, w):
    """Node::Init (core/graph/node.cc:46-66) row by row, every add an np.float32 add in order:
    prefix_w runs over the whole row, each group sums on its own, type_prefix runs over the groups' sums"""
    row_ptr = np.zeros(n_rows + 1, np.int64)
    type_end = np.zeros(n_rows * T, np.int32)
    prefix = np.zeros(len(w), np.float32)
    type_prefix = np.zeros(n_rows * T, np.float32)
    wl = [np.float32(x) for x in w]
    zero = np.float32(0)
    with np.errstate(all="ignore"):
        for r in range(n_rows):
            base = int(seg_ptr[r * T])
            row_ptr[r] = base
            total, type_sum = zero, zero
            for t in range(T):
                tw = zero
                for j in range(int(seg_ptr[r * T + t]), int(seg_ptr[r * T + t + 1])):
                    total = total + wl[j]
                    tw = tw + wl[j]
                    prefix[j] = total
                type_end[r * T + t] = int(seg_ptr[r * T + t + 1]) - base
                type_sum = type_sum + tw
                type_prefix[r * T + t] = type_sum
    row_ptr[n_rows] = int(seg_ptr[n_rows * T])
    return row_ptr, type_end, prefix, type_prefix


def flags(row_ptr, nbr, prefix):
    """has_zero_nbr, monotone, uniform_w as the host build computes them (per row: prev starts at 0,
    the running sum j + 1 below 2^24, a NaN ends monotone)"""
    zero_nbr = bool((nbr == 0).any())
    monotone = uniform = True
    with np.errstate(invalid="ignore"):
        for r in range(len(row_ptr) - 1):
            p = prefix[row_ptr[r]:row_ptr[r + 1]]
            if len(p) == 0:
                continue
            prev = np.concatenate([np.zeros(1, np.float32), p[:-1]])
            monotone &= bool((p >= prev).all())
            j1 = np.arange(1, len(p) + 1)
            uniform &= bool(((p == j1.astype(np.float32)) & (j1 < (1 << 24))).all())
    return zero_nbr, monotone, uniform and monotone and len(nbr) > 0


def identity_map(row_id):
    """(base, stride) when row r has the id base + r * stride with stride > 0, else None"""
    n = len(row_id)
    if n == 0:
        return None
    ids = [int(x) for x in row_id.tolist()]
    stride = 1
    if n > 1:
        if ids[1] <= ids[0]:
            return None
        stride = ids[1] - ids[0]
    mask = (1 << 64) - 1
    if all(ids[i] == (ids[0] + i * stride) & mask for i in range(n)):
        return ids[0], stride
    return None


def feature_table(c, n_rows):
    """from_csr's features argument: the uniform layout, the slots of a row side by side"""
    feats = c["features"]
    if not feats:
        return None
    ends = np.cumsum([f.shape[1] for f in feats]).astype(np.int32)
    val = np.concatenate([np.asarray(f, np.float32) for f in feats], axis=1).reshape(-1)
    fptr = np.arange(n_rows + 1, dtype=np.int64) * int(ends[-1])
    return len(feats), fptr, np.tile(ends, n_rows), val


def reference(c):
    """dict: csr = the keyword arguments of Graph.from_csr; raw = layout(c); has_zero_nbr, monotone,
    uniform_w, identity ((base, stride) or None), max_id"""
    row_id, seg_ptr, nbr, w = layout(c)
    T = c["n_edge_types"]
    n = len(row_id)
    row_ptr, type_end, prefix, type_prefix = node_init(n, T, seg_ptr, w)
    zero_nbr, monotone, uniform = flags(row_ptr, nbr, prefix)
    csr = dict(row_id=row_id, row_ptr=row_ptr, type_end=type_end, nbr=nbr, prefix_w=prefix,
               type_prefix=type_prefix, n_edge_types=T, node_type=c["node_type"],
               node_weight=c["node_weight"], features=feature_table(c, n))
    return dict(csr=csr, raw=(row_id, seg_ptr, nbr, w), has_zero_nbr=zero_nbr, monotone=monotone,
                uniform_w=uniform, identity=identity_map(row_id),
                max_id=max([int(x) for x in row_id.tolist()], default=0))


# ------------------------------------------------------------------------------------------ cases
def _rng(seed):
    return np.random.default_rng(seed)


def _pattern(n):
    """the order-sensitive weights: 2^24, 1, 1, 1, 1, 2^24 and so on ((2^24 + 1) + 1 = 2^24 in f32,
    (1 + 1) + 2^24 = 2^24 + 2)"""
    return np.resize(np.array([BIG, 1, 1, 1, 1, BIG], np.float32), n)


def _empty_e():
    return case([], [], nodes=np.arange(1, 6))


def _empty_n():
    return case([], [])


def _one_edge():
    return case([5], [9], weight=[2.5])


def _isolated():
    # rows 1 (front), 4 (middle), 7 and 8 (last) have no out-edge
    return case([2, 3, 3, 5, 6, 6], [1, 8, 4, 7, 2, 2], weight=[1, 2, 3, 4, 5, 6], nodes=np.arange(1, 9))


def _dst_only():
    # nodes None: 40, 50 and 2^40 occur only as dst and are rows of degree 0
    return case([10, 10, 20, 30], [40, 20, 50, 1 << 40], weight=[1, .5, 2, 4])


def _missing_types():
    # T = 3; row 1 lacks type 0, row 2 type 1, row 3 type 2, row 4 types 0 and 2, row 5 has all
    src = [1, 1, 1, 2, 2, 3, 3, 3, 4, 5, 5, 5, 5]
    typ = [1, 2, 1, 0, 2, 0, 1, 0, 1, 2, 0, 1, 0]
    dst = [2, 3, 4, 5, 1, 2, 2, 4, 5, 1, 2, 3, 4]
    return case(src, dst, edge_type=typ, weight=np.arange(1, 14) * 0.37, n_edge_types=3, nodes=np.arange(1, 6))


def _one_type_of_32():
    r = _rng(1)
    return case(r.integers(1, 9, 40), r.integers(1, 9, 40), edge_type=np.full(40, 17), weight=r.random(40) + .1,
                n_edge_types=32, nodes=np.arange(1, 9))


def _shuffled_duplicates():
    # not grouped by source, repeated (src, dst, type) with different weights: the stable sort alone
    # fixes the entry order
    r = _rng(2)
    src = r.integers(1, 30, 400)
    dst = r.integers(1, 6, 400)
    typ = r.integers(0, 2, 400)
    return case(src, dst, edge_type=typ, weight=(r.random(400) * 8 + .5), n_edge_types=2)


def _order_sums():
    # row 1: 2^24, 1, 1 in one group; row 2: 1, 1, 2^24; row 3: 2^24, 1 | 1 and row 4: 1, 1 | 2^24
    # across the boundary of types 0 and 1; given interleaved, so the input order within a row counts
    src = [1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4]
    typ = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    w = [BIG, 1, BIG, 1, 1, 1, 1, 1, 1, BIG, 1, BIG]
    return case(src, np.arange(10, 22), edge_type=typ, weight=w, n_edge_types=2, nodes=[1, 2, 3, 4])


def _long_rows():
    # a hub of 70 000 entries and a row of 300 among rows of degree 1 to 3; rows of exactly 64, 65,
    # 1024 and 1025 entries (one lane's limit, a staged chunk); two types, so the hub's sums cross a
    # type boundary inside a chunk; the hub and the long rows weigh by the order-sensitive pattern
    r = _rng(3)
    n = 400
    deg = r.integers(1, 4, n + 1)
    deg[[0]] = 0
    deg[7], deg[8], deg[100], deg[101], deg[200], deg[399] = 70000, 300, 64, 65, 1024, 1025
    src = np.repeat(np.arange(n + 1), deg)
    w = (r.random(len(src)) * 4 + .25).astype(np.float32)
    for row in (7, 8, 100, 101, 200, 399):
        at = np.flatnonzero(src == row)
        w[at] = _pattern(len(at))
    typ = (r.random(len(src)) < .4).astype(np.int32)
    dst = r.integers(1, n + 1, len(src))
    perm = r.permutation(len(src))
    return case(src[perm], dst[perm], edge_type=typ[perm], weight=w[perm], n_edge_types=2, nodes=np.arange(1, n + 1))


def _long_row_unweighted():
    # weight None on a row past the lane limit and one past a chunk: uniform_w through the wave path
    src = np.concatenate([np.full(1500, 3), np.full(70, 2), [1, 4]])
    return case(src, np.arange(len(src)) % 5 + 1, nodes=[1, 2, 3, 4, 5])


def _weight_none():
    r = _rng(4)
    return case(r.integers(1, 20, 100), r.integers(1, 20, 100), edge_type=r.integers(0, 2, 100), n_edge_types=2)


def _negative_weight():
    return case([1, 1, 1, 2], [2, 3, 4, 1], weight=[1, -0.5, 2, 1])


def _nan_weight():
    return case([1, 1, 1, 2, 2], [2, 3, 4, 1, 3], weight=[1, np.nan, 2, 1, 3])


def _zero_nbr_nodes():
    return case([1, 2, 2], [0, 1, 3], weight=[1, 2, 3], nodes=[1, 2, 3])


def _zero_nbr_row():
    # nodes None: id 0 becomes a row, and a key of the hash id map
    return case([5, 9, 0], [0, 5, 9], weight=[1, 2, 3])


def _ids_1_n():
    r = _rng(5)
    return case(np.concatenate([np.arange(1, 51), r.integers(1, 51, 150)]), r.integers(1, 51, 200),
                weight=r.random(200) + .5)


def _ids_strided():
    r = _rng(6)
    nodes = 10 + 3 * np.arange(20)
    return case(r.choice(nodes, 60), r.choice(nodes, 60), weight=r.random(60) + .5, nodes=nodes)


def _single_row():
    return case([7, 7], [7, 3], weight=[1, 2], nodes=[7])


def _ids_u64():
    r = _rng(7)
    ids = np.concatenate([r.integers(1, 1 << 62, 30, dtype=np.uint64),
                          np.array([(1 << 63) + 5, (1 << 64) - 1, 3], dtype=U64)])
    return case(r.choice(ids, 120), r.choice(ids, 120), edge_type=r.integers(0, 2, 120), weight=r.random(120) + .5,
                n_edge_types=2)


def _nodes_descending():
    r = _rng(8)
    nodes = np.arange(40, 0, -1)
    return case(r.integers(1, 41, 100), r.integers(1, 60, 100), weight=r.random(100) + .5, nodes=nodes)


def _key_bits(n, T, seed):
    r = _rng(seed)
    src = np.concatenate([np.arange(1, n + 1), r.integers(1, n + 1, 5 * n)])
    typ = np.concatenate([np.full(n, T - 1), r.integers(0, T, 5 * n)])     # the top key n * T - 1 occurs
    return case(src, r.integers(1, n + 1, 6 * n), edge_type=typ, weight=r.random(6 * n) + .5, n_edge_types=T,
                nodes=np.arange(1, n + 1))


def _undirected():
    # a self loop (3, 3), typed and weighted; nodes None
    src = [1, 3, 2, 5, 1, 3]
    dst = [2, 3, 4, 1, 2, 9]
    return case(src, dst, edge_type=[0, 1, 1, 0, 1, 0], weight=[1, 2, 3, 4, 5, 6], n_edge_types=2, undirected=True)


def _undirected_nodes():
    r = _rng(9)
    return case(r.integers(1, 31, 200), r.integers(1, 31, 200), edge_type=r.integers(0, 3, 200),
                weight=r.random(200) + .5, n_edge_types=3, nodes=np.arange(1, 31), undirected=True)


def _features(d0, seed):
    r = _rng(seed)
    n = 50
    feats = [r.standard_normal((n, d0)).astype(np.float32), r.standard_normal((n, 64)).astype(np.float32)]
    return case(r.integers(1, n + 1, 300), r.integers(1, n + 1, 300), weight=r.random(300) + .5,
                nodes=np.arange(1, n + 1), features=feats)


def _node_types():
    r = _rng(10)
    n = 60
    return case(r.integers(1, n + 1, 300), r.integers(1, n + 1, 300), weight=r.random(300) + .5,
                nodes=np.arange(1, n + 1), node_type=r.integers(0, 2, n), node_weight=r.random(n) * 3 + .1)


_BUILDERS = {
    "empty_edges_5_nodes": _empty_e,
    "empty_graph": _empty_n,
    "one_edge": _one_edge,
    "isolated_rows": _isolated,
    "ids_only_as_dst": _dst_only,
    "missing_types": _missing_types,
    "one_type_of_32": _one_type_of_32,
    "shuffled_duplicates": _shuffled_duplicates,
    "order_sensitive_sums": _order_sums,
    "long_rows": _long_rows,
    "long_row_unweighted": _long_row_unweighted,
    "weight_none": _weight_none,
    "negative_weight": _negative_weight,
    "nan_weight": _nan_weight,
    "zero_nbr": _zero_nbr_nodes,
    "zero_id_row": _zero_nbr_row,
    "ids_1_to_n": _ids_1_n,
    "ids_strided": _ids_strided,
    "single_row": _single_row,
    "ids_u64": _ids_u64,
    "nodes_descending": _nodes_descending,
    "keys_power_of_two": lambda: _key_bits(8, 4, 11),         # N * T = 32
    "keys_power_of_two_plus_1": lambda: _key_bits(11, 3, 12),  # N * T = 33
    "undirected_self_loop": _undirected,
    "undirected_nodes": _undirected_nodes,
    "features_3_64": lambda: _features(3, 13),
    "features_4_64": lambda: _features(4, 14),
    "node_types": _node_types,
}
CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def get_case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def get_reference(name):
    return reference(get_case(name))
