"""tf_euler.python.euler_ops.sample_ops (module path kept for ported code); the node functions live
in node_ops.  Graph labels come from the node binary feature binary_graph_label."""
from . import base
from .node_ops import sample_node, sample_node_with_src, get_node_type  # noqa: F401
from .type_ops import get_edge_type_id


def sample_edge(count, edge_type=None):
    """[count, 3] int64 (src, dst, type) sampled by edge weight (sample_ops.py:62-72); edge_type
    '-1' / -1 / None = all types, or a type (name or id) or a list of them."""
    if edge_type is None or edge_type == '-1' or edge_type == -1:
        types = -1
    else:
        types = get_edge_type_id(edge_type if isinstance(edge_type, (list, tuple)) else [edge_type])
    return base.get_default_graph().sample_edge(int(count), types)


def sample_graph_label(count):
    """tf_euler sample_graph_label (sample_ops.py): `count` graph labels drawn uniformly with
    replacement, as a list of str (torch has no string tensors)."""
    g = base.get_default_graph()
    table = g.graph_labels()
    ids = g.sample_graph_label(int(count)).cpu().tolist()
    return [table[i] for i in ids]


def get_graph_by_label(labels):
    """tf_euler get_graph_by_label: the SparseTensor triple (indices [nnz, 2], values, dense_shape)
    of the nodes of every label."""
    return base.get_default_graph().get_graph_by_label(list(labels))
