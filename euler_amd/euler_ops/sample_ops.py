"""tf_euler.python.euler_ops.sample_ops (module path kept for ported code); the node functions live
in node_ops.  get_graph_by_label needs graph labels, which this backend does not load."""
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
