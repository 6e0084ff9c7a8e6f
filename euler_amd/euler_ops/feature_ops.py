"""tf_euler.python.euler_ops.feature_ops (module path kept for ported code).  Node dense / sparse
features live in node_ops; the edge and binary features (feature_ops.py:75-160 in the reference)
are here.  Feature names: a name that parses as an integer is a slot index; any other name is
looked up in the dataset's euler.meta as dense_<name> / sparse_<name> / binary_<name>."""
from . import base
from .node_ops import get_dense_feature, get_sparse_feature  # noqa: F401

_KIND = {0: "sparse", 1: "dense", 2: "binary"}


def _slots(graph, names, kind, edge):
    out = []
    for name in names:
        try:
            out.append(int(str(name)))
            continue
        except ValueError:
            pass
        if graph.data_path is None:
            raise ValueError("feature name %r needs a graph loaded from a data directory" % (name,))
        t, slot, _ = graph.feature_info("%s_%s" % (kind, name), edge)
        if _KIND.get(t) != kind:
            raise ValueError("feature %r is not a %s feature" % (name, kind))
        out.append(slot)
    return out


def _as_bytes(pairs, n):
    """(offsets, bytes) per feature -> per feature a list of n `bytes` (the TF op's strings)."""
    out = []
    for off, data in pairs:
        o = off.cpu().numpy()
        d = data.cpu().numpy().tobytes()
        out.append([d[o[i]:o[i + 1]] for i in range(n)])
    return out


def get_edge_dense_feature(edges, feature_names, dimensions, thread_num=1):
    """[n, 3] (src, dst, type) -> list of [n, dim] float32, zeros for unknown edges."""
    g = base.get_default_graph()
    return g.get_edge_dense_feature(edges, _slots(g, feature_names, "dense", True), list(dimensions))


def get_edge_sparse_feature(edges, feature_names, default_values=None, thread_num=1):
    """[n, 3] edges -> one SparseTensor triple per feature (default value for an empty edge)."""
    g = base.get_default_graph()
    return g.get_edge_sparse_feature(edges, _slots(g, feature_names, "sparse", True), default_values)


def get_edge_binary_feature(edges, feature_names, thread_num=1):
    """[n, 3] edges -> per feature a list of n `bytes` (b"" for an unknown edge)."""
    g = base.get_default_graph()
    e = g._edges(edges)
    return _as_bytes(g.get_edge_binary_feature(e, _slots(g, feature_names, "binary", True)),
                     e.shape[0])


def get_binary_feature(nodes, feature_names, thread_num=1):
    """nodes -> per feature a list of n `bytes` (b"" for an unknown node)."""
    g = base.get_default_graph()
    pairs = g.get_binary_feature(nodes, _slots(g, feature_names, "binary", False))
    return _as_bytes(pairs, pairs[0][0].numel() - 1 if pairs else 0)


def sparse_feature_embedding(nodes, feature_names, tables, combiner="sum", default_values=None,
                             out_dtype=None, sparse_grad=False):
    """nodes -> per (sparse feature, table [V, dim]) the [n, dim] combined embedding rows
    (ShallowEncoder, utils/encoders.py:146-170), fused and differentiable in the table:
    Graph.sparse_feature_embedding."""
    g = base.get_default_graph()
    return g.sparse_feature_embedding(nodes, _slots(g, feature_names, "sparse", False), tables, combiner,
                                      default_values, out_dtype, sparse_grad)


def supervise_loss(nodes, logits, label_name, label_dim, metric=None, return_prob=False):
    """SuperviseModel.__call__ after out_fc (mp_utils/base.py:35-47) on the default graph: the mean
    sigmoid cross-entropy of logits [n, label_dim] against the dense feature `label_name` of the
    nodes, read straight from the feature table, plus a streaming metric: Graph.supervise_loss."""
    g = base.get_default_graph()
    return g.supervise_loss(nodes, logits, _slots(g, [label_name], "dense", False)[0], label_dim, metric, return_prob)
