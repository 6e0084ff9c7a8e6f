"""numpy restatement of the graph-label semantics: the label table, the
get_graph_by_label triple, the SampleGraphLabel draws (RNG domain 7) and the whole-graph block
read off a SparseGetAdj result.  Also a builder of multi-graph CSRs for the GPU tests."""
import numpy as np

SALT = [0x00000000, 0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x6A09E667, 0xB5C0FBCF, 0x3C6EF372,
        0xA54FF53A]
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 on uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(x, np.uint64) & M32 for x in (c0, c1, c2, c3))
    k0 = np.uint64(k0) & M32
    k1 = np.uint64(k1) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & M32
        hi1, lo1 = p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def rng_draws(seed, call_id, domain, stream, count):
    """u[j] for draws j = 0 .. count-1 of (seed, call_id, domain, stream)."""
    j = np.arange(count, dtype=np.uint64)
    blk = j >> np.uint64(1)
    w = philox4x32_10(np.full(count, call_id, np.uint64), np.full(count, stream & 0xFFFFFFFF, np.uint64),
                      np.full(count, stream >> 32, np.uint64), blk, seed & 0xFFFFFFFF,
                      ((seed >> 32) ^ SALT[domain]) & 0xFFFFFFFF)
    odd = (j & np.uint64(1)).astype(bool)
    a = np.where(odd, w[2], w[0])
    b = np.where(odd, w[3], w[1])
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0
            + (b >> np.uint64(6)).astype(np.float64)) * (1.0 / 9007199254740992.0)


def sample_graph_label(seed, call_id, count, n_labels):
    """Draw j is sample j: label = min(floor(u * L), L - 1)."""
    u = rng_draws(seed, call_id, 7, 0, count)
    return np.minimum(np.floor(u * n_labels).astype(np.int64), n_labels - 1)


def label_table(ids, labels):
    """(table, nodes): labels ordered by their smallest node id (Q14), the nodes of each in
    ascending id order; "" is no label (Q15)."""
    groups = {}
    for i, lab in zip(np.asarray(ids, np.uint64).tolist(), labels):
        lab = lab.decode() if isinstance(lab, bytes) else lab
        if lab == "":
            continue
        groups.setdefault(lab, []).append(i)
    table = sorted(groups, key=lambda k: min(groups[k]))
    return table, [sorted(groups[k]) for k in table]


def graph_by_label(table, nodes, labels):
    """SparseTensorBuilder triple of get_graph_by_label: (indices [nnz, 2], values, dense_shape);
    a label with no nodes emits (i, 0) = 0."""
    pos = {k: r for r, k in enumerate(table)}
    ind, val, width = [], [], 1
    for i, lab in enumerate(labels):
        ns = nodes[pos[lab]] if lab in pos else []
        width = max(width, len(ns))
        if not ns:
            ind.append((i, 0))
            val.append(0)
        for j, v in enumerate(ns):
            ind.append((i, j))
            val.append(v)
    if not labels:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64), [0, 0]
    return np.asarray(ind, np.int64).reshape(-1, 2), np.asarray(val, np.uint64).astype(np.int64), \
        [len(labels), width]


def block_from_adj(ind, val, n, add_self_loops=True):
    """Whole-graph block read off sparse_get_adj(n_id, n_id): ind[val == 1][:, 1:] without the
    explicit zero at (N-1, N-1), then the self loops (Q16)."""
    ind = np.asarray(ind).reshape(-1, 3)
    val = np.asarray(val).reshape(-1)
    e = ind[val == 1][:, 1:]
    order = np.lexsort((e[:, 1], e[:, 0]))
    e = e[order].T.astype(np.int64)
    if add_self_loops:
        loops = np.arange(n, dtype=np.int64)
        e = np.concatenate([e, np.stack([loops, loops])], 1)
    return e


def block_ref(n_id, adj):
    """The block from a host adjacency {id: set of out-neighbour ids of the listed types}."""
    pos = {}
    for c, x in enumerate(n_id):
        pos.setdefault(int(x), []).append(c)
    src, dst = [], []
    for j, x in enumerate(n_id):
        cs = sorted(c for nb in adj.get(int(x), ()) for c in pos.get(int(nb), ()))
        src += [j] * len(cs)
        dst += cs
    n = len(n_id)
    return np.asarray([src + list(range(n)), dst + list(range(n))], np.int64).reshape(2, -1)


def multigraph_csr(n_graphs, seed, min_nodes=10, max_nodes=40, cross=0.01, n_hubs=8,
                   hub_degree=5000, unlabelled=0.01):
    """A MUTAG-like set at scale: graph g is a run of consecutive ids 1.. with 10-40 nodes, 2 edge
    types, 1-4 edges per node and type (about `cross` of them to another graph), `n_hubs` rows of
    `hub_degree` edges, and `unlabelled` of the nodes without a label.  Labels are the decimal
    graph index (multigraph_util.py).  Returns (from_csr kwargs, ids, labels, adjacency by type)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(min_nodes, max_nodes + 1, n_graphs)
    n = int(sizes.sum())
    gof = np.repeat(np.arange(n_graphs), sizes)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    ids = np.arange(1, n + 1, dtype=np.uint64)
    T = 2
    deg = rng.integers(1, 5, (n, T))
    hubs = rng.choice(n, n_hubs, replace=False)
    deg[hubs, 0] = hub_degree
    tot = deg.sum(1)
    row_ptr = np.concatenate([[0], np.cumsum(tot)]).astype(np.int64)
    E = int(row_ptr[-1])
    src = np.repeat(np.arange(n), tot)
    local = rng.integers(0, 1 << 30, E) % sizes[gof[src]]
    nbr = first[gof[src]] + local
    far = rng.random(E) < cross
    nbr[far] = rng.integers(0, n, int(far.sum()))
    nbr = nbr.astype(np.uint64) + np.uint64(1)
    type_end = np.cumsum(deg, 1).astype(np.int32)
    prefix_w = (np.arange(E) - np.repeat(row_ptr[:-1], tot) + 1).astype(np.float32)
    type_prefix = type_end.astype(np.float32)
    labels = [str(g) for g in gof.tolist()]
    for i in rng.choice(n, int(n * unlabelled), replace=False).tolist():
        labels[i] = ""
    kw = dict(row_id=ids, row_ptr=row_ptr, type_end=type_end, nbr=nbr, prefix_w=prefix_w,
              type_prefix=type_prefix, n_edge_types=T)
    return kw, ids, labels, (src, nbr, deg)
