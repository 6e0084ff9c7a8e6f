"""A plain restatement of the sparse-feature embedding lookup (euler_amd/csrc/sparse_embed.h) for
tests/test_sparse_embedding_host.py and tests/test_sparse_embedding_gpu.py: numpy float32 loops,
nothing of the library.

  entry list   the node's uint64 values; an empty list becomes [default] when there is a default
  range rule   an entry >= V (unsigned) is left out of the sum and of the count
  sum          the counted rows in stored order, one float32 add per entry, starting from the first
  combiners    sum; mean = sum / float32(cnt); sqrtn = sum / sqrt(float32(cnt)); cnt == 0: zeros
"""
import numpy as np

COMBINERS = ("sum", "mean", "sqrtn")
CODE = {"sum": 0, "mean": 1, "sqrtn": 2}


def entries(values, default):
    """The uint64 entry list of a node with the stored `values`."""
    values = np.asarray(values, np.uint64).reshape(-1)
    if len(values) == 0 and default is not None:
        return np.array([int(default) % (1 << 64)], np.uint64)
    return values


def embed_row(values, default, table32, combiner):
    """-> (row [dim] float32, cnt).  table32: the table widened to float32."""
    V, dim = table32.shape
    acc, cnt = None, 0
    for v in entries(values, default).tolist():
        if v >= V:
            continue
        row = table32[v]
        acc = row.copy() if acc is None else (acc + row).astype(np.float32)
        cnt += 1
    if cnt == 0:
        return np.zeros(dim, np.float32), 0
    if combiner == "mean":
        acc = (acc / np.float32(cnt)).astype(np.float32)
    elif combiner == "sqrtn":
        acc = (acc / np.sqrt(np.float32(cnt))).astype(np.float32)
    else:
        assert combiner == "sum"
    assert acc.dtype == np.float32
    return acc, cnt


def counted(lists, default, V):
    """Per node the table rows its combiner counts, in stored order."""
    out = []
    for v in lists:
        e = entries(v, default)
        out.append(e[e < np.uint64(V)].astype(np.int64))
    return out


def pad(ids_per_node):
    """-> (ids [n, longest] int64, padded with 0; counts [n] int32)"""
    counts = np.array([len(x) for x in ids_per_node], np.int32)
    P = np.zeros((len(ids_per_node), int(counts.max()) if len(counts) else 0), np.int64)
    for i, x in enumerate(ids_per_node):
        P[i, :len(x)] = x
    return P, counts


def embed_sums(ids_per_node, table32, padded=None):
    """The ordered float32 sums of all nodes at once: step k adds entry k of every node that has
    one - the same adds as embed_row, node by node.  -> (sum [n, dim] float32, counts int32)."""
    P, counts = padded if padded is not None else pad(ids_per_node)
    acc = np.zeros((len(counts), table32.shape[1]), np.float32)
    for k in range(P.shape[1]):
        live = np.nonzero(counts > k)[0]
        rows = table32[P[live, k]]
        acc[live] = rows if k == 0 else (acc[live] + rows).astype(np.float32)
    return acc, counts


def combine(sums, counts, combiner):
    """sum -> the combiner's rows (float32 division, a zero row for cnt == 0)."""
    out = sums.copy()
    if combiner == "sum":
        return out
    c = counts.astype(np.float32)
    d = c if combiner == "mean" else np.sqrt(c)
    has = counts > 0
    out[has] = (sums[has] / d[has, None]).astype(np.float32)
    return out


def embed(lists, default, table32, combiner):
    """lists: one sequence of uint64 values per node -> ([n, dim] float32, counts [n] int32)."""
    sums, counts = embed_sums(counted(lists, default, table32.shape[0]), table32)
    return combine(sums, counts, combiner), counts


def pairs(lists, default, V):
    """(batch row, table row) of every counted entry: batch order, then stored order."""
    rows, ids = [], []
    for i, v in enumerate(lists):
        for x in entries(v, default).tolist():
            if x < V:
                rows.append(i)
                ids.append(x)
    return np.array(rows, np.int64), np.array(ids, np.int64)


def grad_table_f64(lists, default, V, counts, grad, combiner):
    """float64 gradient of the table for the output gradient `grad` [n, dim]."""
    g = np.asarray(grad, np.float64)
    c = counts.astype(np.float64).reshape(-1, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = g if combiner == "sum" else g / (c if combiner == "mean" else np.sqrt(c))
    s = np.where(c == 0, 0.0, s)
    rows, ids = pairs(lists, default, V)
    out = np.zeros((V, g.shape[1]), np.float64)
    np.add.at(out, ids, s[rows])
    return out
