"""numpy restatement of the full-neighbour aggregation (euler_amd/csrc/mp_rows.h, include/euler_gpu.h:
euler_gpu_neighbor_reduce / euler_gpu_neighbor_degree), per node, from the CSR arrays handed to
Graph.from_csr - independent of the kernels and of the ops it is compared with.  Every fp32
operation is one numpy float32 operation, in the enumerated order."""
import numpy as np

F = np.float32


class Rows(object):
    """the arrays of Graph.from_csr: row_id [R], row_ptr [R + 1], type_end [R, T] (cumulative,
    row-relative), nbr [E] uint64, prefix_w [E] float32 (running sums per row)"""

    def __init__(self, row_id, row_ptr, type_end, nbr, prefix_w, n_types):
        self.row_id = np.asarray(row_id, np.uint64)
        self.row_ptr = np.asarray(row_ptr, np.int64)
        self.T = int(n_types)
        self.type_end = np.asarray(type_end, np.int32).reshape(-1, self.T)
        self.nbr = np.asarray(nbr, np.uint64)
        self.prefix_w = np.asarray(prefix_w, np.float32)
        self.row_of = {int(i): r for r, i in enumerate(self.row_id)}

    def positions(self, node, edge_types):
        """row-relative positions of the listed entries of `node`, in get_full_neighbor's order;
        (None, empty) when the id has no row"""
        r = self.row_of.get(int(node) & 0xFFFFFFFFFFFFFFFF)
        if r is None:
            return None, np.zeros(0, np.int64)
        pos = []
        for t in edge_types:
            if 0 <= t < self.T:
                b = 0 if t == 0 else int(self.type_end[r, t - 1])
                pos.extend(range(b, int(self.type_end[r, t])))
        return r, np.asarray(pos, np.int64)

    def edge_weight(self, r, p):
        """fl(prefix_w[p] - prefix_w[p - 1]), p row-absolute (0 before the row's first entry)"""
        base = self.row_ptr[r]
        pre = F(0) if p == 0 else self.prefix_w[base + p - 1]
        return F(self.prefix_w[base + p] - pre)


def degree(G, nodes, edge_types, self_loop=False):
    return np.array([len(G.positions(v, edge_types)[1]) + (1 if self_loop else 0) for v in nodes], np.int32)


def norm_of(deg):
    deg = np.asarray(deg)
    out = np.zeros(deg.shape, F)
    pos = deg > 0
    out[pos] = F(1) / np.sqrt(deg[pos].astype(F))
    return out


def updates(G, i, node, edge_types, kind, norm, self_loop, table_rows):
    """[(table row, weight)] of queried node i, in order"""
    r, pos = G.positions(node, edge_types)
    ids = [int(G.nbr[G.row_ptr[r] + p]) for p in pos]
    ws = [G.edge_weight(r, p) if kind == "edge" else F(1) for p in pos]
    if self_loop:
        ids.append(int(node) & 0xFFFFFFFFFFFFFFFF)
        ws.append(F(1))
    out = []
    for j, w in zip(ids, ws):
        g = j & 0xFFFFFFFF
        if kind == "norm":
            w = F(norm[0][i] * norm[1][g]) if g < table_rows else F(0)
        out.append((min(g, table_rows - 1), w))
    return out


def reduce_updates(op, x, ups):
    """one node: x fp32 [rows, d], ups [(row, weight)]"""
    d = x.shape[1]
    acc = np.full(d, -1e9 if op == "max" else 0.0, F)
    for row, w in ups:
        m = x[row] * w                      # float32 * float32: one rounding
        acc = np.where(m > acc, m, acc) if op == "max" else acc + m
    if op == "mean":
        acc = acc / F(F(len(ups)) + F(1e-7))
    return acc.astype(F)


def aggregate(G, op, x, nodes, edge_types, kind=None, norm=None, self_loop=False, root=None, a=1.0, b=1.0):
    """fp32 [n, d], before the one rounding to a 16-bit out dtype.  x and root are fp32 (a 16-bit
    table widened, which is exact).  Repeated nodes are computed once (kind "norm": per (node,
    norm_dst) pair)."""
    x = np.asarray(x, F)
    nodes = np.asarray(nodes, np.int64)
    out = np.empty((len(nodes), x.shape[1]), F)
    seen = {}
    for i, v in enumerate(nodes):
        key = (int(v), None if kind != "norm" else norm[0][i].tobytes())
        if key not in seen:
            seen[key] = reduce_updates(op, x, updates(G, i, v, edge_types, kind, norm, self_loop, x.shape[0]))
        out[i] = seen[key]
    if root is not None:
        out = (out * F(a) + np.asarray(root, F) * F(b)).astype(F)
    return out


def exact_f64(op, x, ups):
    """(the reduce in float64 from the same fp32 weights - and, for a mean, the same fp32
    denominator fl(length + 1e-7f) -, sum of |terms|): against it the fp32 result has one rounding
    per message, length - 1 for the sum and one for the mean's divide"""
    terms = np.array([x[row].astype(np.float64) * np.float64(w) for row, w in ups]).reshape(len(ups), x.shape[1])
    s = terms.sum(0)
    if op == "mean":
        denom = np.float64(F(F(len(ups)) + F(1e-7)))
        return s / denom, np.abs(terms).sum(0) / denom
    return s, np.abs(terms).sum(0)
