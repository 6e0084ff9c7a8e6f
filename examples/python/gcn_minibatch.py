#!/usr/bin/env python3
"""A GCN input pipeline on the tf_euler operator surface, end to end on one MI355X.

What tf_euler/python/dataflow/gcn_dataflow.py + tf_euler/python/convolution/gcn_conv.py do per
training step in the reference: build the full-neighbour blocks of a batch of roots
(GCNDataFlow), fetch the dense features of the outermost layer, and aggregate block by block
with GCN's symmetric normalisation - message norm_i * norm_j * x_j (gcn_conv.py:50-51), where
norm = deg ** -0.5 of both sides of the block (gcn_conv.py:33-40).  The normalisation is a
per-edge scalar, so the whole aggregation of a block is ONE fused call:

    gather_scatter("add", x, src, dst, n, edge_weight=norm_i * norm_j)

with the bits of the composition scatter_add(norm_i * norm_j * gather(x, src), dst, n) and
without its [E, D] intermediates.

    python examples/python/gcn_minibatch.py [--data DIR] [--batch 4] [--dim 8] [--composed]

--data: a directory written by euler/tools (default: the repository's fixture graph).
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402
from euler_amd import euler_ops, ops               # noqa: E402
from euler_amd.dataflow import GCNDataFlow         # noqa: E402


def gcn_norm(edge_index, size):
    """deg ** -0.5 of the destinations and of the sources of a block (gcn_conv.py:33-40)"""
    ones = torch.ones((edge_index.shape[1], 1), device=edge_index.device)
    return tuple(ops.scatter_add(ones, edge_index[i], size[i]) ** -0.5 for i in (0, 1))


def edge_norm(blk):
    """norm_i * norm_j per edge, [E, 1]"""
    norm_i, norm_j = gcn_norm(blk.edge_index, blk.size)
    return ops.gather(norm_i, blk.edge_index[0]) * ops.gather(norm_j, blk.edge_index[1])


def aggregate(x, blk, composed=False):
    dst, src = blk.edge_index[0], blk.edge_index[1]
    w = edge_norm(blk)
    if composed:        # the three ops and two [E, D] blocks the fused call replaces
        return ops.scatter_add(w * ops.gather(x, src), dst, blk.size[0])
    return ops.gather_scatter("add", x, src, dst, blk.size[0], edge_weight=w)


def run(graph, roots, dim, metapath=((0, 1), (0, 1)), composed=False):
    """-> the aggregated rows of `roots` after len(metapath) GCN aggregations"""
    flow = GCNDataFlow(graph, [list(h) for h in metapath], add_self_loops=True)
    df = flow(roots)
    x = graph.get_dense_feature(df[0].n_id, [0], [dim])[0]
    for blk in df:
        x = aggregate(x, blk, composed)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=os.path.join(ROOT, "tests", "golden", "fixture_dat"))
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--composed", action="store_true")
    a = ap.parse_args()
    euler_ops.initialize_graph({"mode": "local", "data_path": a.data})
    G = euler_ops.get_default_graph()
    G.set_seed(42)
    roots = euler_ops.sample_node(a.batch, -1)
    out = run(G, roots, a.dim, composed=a.composed)
    torch.cuda.synchronize()
    print("GCN aggregation (%s) of %d roots over 2 full-neighbour blocks: [%d, %d], |sum| = %.6f"
          % ("composed" if a.composed else "fused", roots.numel(), out.shape[0], out.shape[1],
             float(out.abs().sum())))


if __name__ == "__main__":
    main()
