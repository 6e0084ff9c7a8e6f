#!/usr/bin/env python3
"""The GCN family's propagation steps over full-neighbour blocks, each block in two fused calls.

Six convolutions of tf_euler/python/convolution multiply every message by the symmetric degree
normalisation norm_i * norm_j, norm = deg ** -0.5 on both sides of the block (gcn_conv.py:33-51,
sgcn_conv.py, tag_conv.py, appnp_conv.py:34-60, arma_conv.py:46-78, dna_conv.py:106-170).  Per block:

    norm = ops.gcn_norm(blk.edge_index, blk.size)               # a histogram: no sort, no host wait
    h = ops.gcn_aggregate(x, blk.edge_index, blk.size, norm)    # norm_i * norm_j * x_j, summed

and with the destination's own row in the same pass: an APPNP step (alpha: (1 - alpha) * agg +
alpha * h0, appnp_conv.py:57-60) or an ARMA step (agg + root, arma_conv.py:72-75).  Over the three
blocks of a batch this script runs one of each: GCN / SGCN aggregation, APPNP step, ARMA step.

    python examples/python/gcn_norm_minibatch.py [--data DIR] [--batch 4] [--dim 8] [--composed]

--composed runs the same steps with gcn_norm's tables and the existing ops (per-edge weight,
weighted gather_scatter, elementwise epilogue): the same bits, more passes.
--data: a directory written by euler/tools (default: the repository's fixture graph).
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402,F401
from euler_amd import euler_ops, ops               # noqa: E402
from euler_amd.dataflow import GCNDataFlow         # noqa: E402

ALPHA = 0.1
STEPS = ("gcn", "appnp", "arma")


def step(kind, x, blk, composed=False):
    """one propagation step over a block: x [n_src, D] -> [n_dst, D]"""
    norm = ops.gcn_norm(blk.edge_index, blk.size)
    root = None if kind == "gcn" else x[blk.res_n_id]          # the destinations' own rows
    alpha = ALPHA if kind == "appnp" else None
    if not composed:
        return ops.gcn_aggregate(x, blk.edge_index, blk.size, norm, root=root, alpha=alpha)
    dst, src = blk.edge_index[0], blk.edge_index[1]
    w = norm[0][dst.long()] * norm[1][src.long()]              # norm_i * norm_j per edge, [E]
    agg = ops.gather_scatter("add", x, src, dst, blk.size[0], edge_weight=w)
    if kind == "gcn":
        return agg
    return agg * (1 - ALPHA) + root * ALPHA if kind == "appnp" else agg + root


def run(graph, roots, dim, composed=False):
    """-> the rows of `roots` after a GCN aggregation, an APPNP step and an ARMA step"""
    flow = GCNDataFlow(graph, [[0, 1]] * len(STEPS), add_self_loops=True)
    df = flow(roots)
    x = graph.get_dense_feature(df[0].n_id, [0], [dim])[0]
    for kind, blk in zip(STEPS, df):
        x = step(kind, x, blk, composed)
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
    print("GCN / APPNP / ARMA steps (%s) of %d roots over %d full-neighbour blocks: [%d, %d], |sum| = %.6f"
          % ("composed" if a.composed else "fused", roots.numel(), len(STEPS), out.shape[0], out.shape[1],
             float(out.abs().sum())))


if __name__ == "__main__":
    main()
