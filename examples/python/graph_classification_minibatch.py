#!/usr/bin/env python3
"""A whole-graph classification input pipeline (GIN / set2set / gated_graph / graphgcn in the
reference), end to end on one MI355X.

What euler_estimator/python/graph_estimator.py (get_train_from_input) and
tf_euler/python/dataflow/whole_dataflow.py do per training step - sample graph labels, fetch the
nodes of those graphs, build the WholeDataFlow block over the whole batch, fetch node features
and pool them by graph - with the same operators (tensors are torch tensors in HBM).

    python examples/python/graph_classification_minibatch.py [--graphs 188] [--batch 128] [--steps 20]

The data is a synthetic MUTAG-shaped set: about 18 nodes per graph, two edge types, labels =
the decimal graph index (as tf_euler/python/dataset/multigraph_util.py writes them), an 8-float
dense feature per node.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402
from euler_amd import ops                          # noqa: E402
from euler_amd.dataflow import WholeGraphDataFlow       # noqa: E402


def mutag_like(n_graphs, seed, dim=8):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(12, 25, n_graphs)
    n = int(sizes.sum())
    gof = np.repeat(np.arange(n_graphs), sizes)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    deg = rng.integers(1, 3, (n, 2))
    tot = deg.sum(1)
    row_ptr = np.concatenate([[0], np.cumsum(tot)]).astype(np.int64)
    src = np.repeat(np.arange(n), tot)
    nbr = (first[gof[src]] + rng.integers(0, 1 << 30, len(src)) % sizes[gof[src]] + 1).astype(np.uint64)
    prefix_w = (np.arange(len(src)) - np.repeat(row_ptr[:-1], tot) + 1).astype(np.float32)
    type_end = np.cumsum(deg, 1).astype(np.int32)
    feats = (1, np.arange(n + 1, dtype=np.int64) * dim, np.full(n, dim, np.int32),
             rng.standard_normal(n * dim).astype(np.float32))
    g = euler_amd.Graph.from_csr(np.arange(1, n + 1, dtype=np.uint64), row_ptr, type_end, nbr,
                                 prefix_w, type_end.astype(np.float32), 2, features=feats)
    g.set_graph_labels(np.arange(1, n + 1, dtype=np.uint64), [str(x) for x in gof.tolist()])
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=188)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dim", type=int, default=8)
    a = ap.parse_args()
    G = mutag_like(a.graphs, 0, a.dim)
    G.set_seed(1)
    flow_of = WholeGraphDataFlow(G, [[0, 1], [0, 1]])
    t0 = time.perf_counter()
    for _ in range(a.steps):
        # 1. graph labels and their nodes (get_train_from_input)
        labels = G.sample_graph_label(a.batch)
        ind, n_id, _ = G.get_graph_by_label(labels)
        node_graph_idx = ind[:, 0]
        # 2. the whole-graph block, shared by every hop
        flow = flow_of(n_id)
        # 3. node features; 4. one propagation over the block, then pooling by graph
        x, = G.get_dense_feature(n_id, [0], [a.dim])
        ei = flow[0].edge_index
        h = ops.scatter_add(x[ei[0]], ei[1], n_id.numel())
        pooled = ops.scatter_add(h, node_graph_idx, a.batch)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    assert pooled.shape == (a.batch, a.dim)
    # check the last step against a host restatement of the pooling
    xs, e, gi = x.cpu().numpy(), ei.cpu().numpy(), node_graph_idx.cpu().numpy()
    hh = np.zeros_like(xs)
    np.add.at(hh, e[1], xs[e[0]])
    want = np.zeros((a.batch, a.dim), np.float32)
    np.add.at(want, gi, hh)
    assert np.allclose(pooled.cpu().numpy(), want, rtol=1e-4, atol=1e-3)
    print("graph classification minibatch ok: %d graphs, %d nodes, %d block edges, %.3f ms/step"
          % (a.batch, n_id.numel(), ei.shape[1], dt * 1e3))


if __name__ == "__main__":
    main()
