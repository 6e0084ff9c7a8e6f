#!/usr/bin/env python3
"""Attention pooling over whole-graph batches, end to end on one MI355X: AttentionPool
(tf_euler/python/graph_pool/attention_pool.py:36-40) and one Set2Set step
(graph_pool/set2set_pool.py:45-49) over the WholeGraphDataFlow batches of
graph_classification_minibatch.py - where that example pools with scatter_add only.

    AttentionPool:  gate = x @ w                         [N, 1] per-node score
                    out  = attention_aggregate("additive", None, gate, nodes, B, v=x,
                                               negative_slope=1.0, indices=node_graph_idx)
    Set2Set step:   q    = the per-graph query           [B, D]
                    r    = attention_aggregate("dot", q, x, nodes, B, indices=node_graph_idx)

(v=None: every node row is loaded once, for the logit and for the sum.)  --composed also runs the
three-op formulation on the same batch and prints the largest difference of the outputs and of
the gate's gradient.

    python examples/python/graph_pool_minibatch.py [--graphs 188] [--batch 128] [--steps 5] [--composed]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from euler_amd import ops                                          # noqa: E402
from euler_amd.dataflow import WholeGraphDataFlow                  # noqa: E402
from graph_classification_minibatch import mutag_like              # noqa: E402


def attention_pool(x, gate, nodes, graph, batch, composed):
    if not composed:
        return ops.attention_aggregate("additive", None, gate, nodes, batch, v=x, negative_slope=1.0, indices=graph)
    alpha = ops.edge_softmax(gate, indices=graph, size=batch)
    return ops.gather_scatter("add", x, nodes, graph, batch, edge_weight=alpha)


def set2set_step(x, q, nodes, graph, batch, composed):
    if not composed:
        return ops.attention_aggregate("dot", q, x, nodes, batch, indices=graph)
    alpha = ops.edge_softmax(ops.edge_dot(q, graph, x, nodes), indices=graph, size=batch)
    return ops.gather_scatter("add", x, nodes, graph, batch, edge_weight=alpha)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=188)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--composed", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    G = mutag_like(a.graphs, 0, a.dim)
    G.set_seed(1)
    flow_of = WholeGraphDataFlow(G, [[0, 1], [0, 1]])
    w = torch.nn.Parameter(torch.randn(a.dim, 1, device="cuda") * 0.3)
    lstm = torch.nn.LSTMCell(2 * a.dim, a.dim).cuda()
    for step in range(a.steps):
        labels = G.sample_graph_label(a.batch)
        ind, n_id, _ = G.get_graph_by_label(labels)
        graph = ind[:, 0].to(torch.int32).contiguous()
        flow = flow_of(n_id)
        x, = G.get_dense_feature(n_id, [0], [a.dim])
        ei = flow[0].edge_index
        h = ops.scatter_add(x[ei[0]], ei[1], n_id.numel())               # one propagation over the block
        nodes = torch.arange(n_id.numel(), device="cuda", dtype=torch.int32)
        pooled = attention_pool(h, h @ w, nodes, graph, a.batch, False)
        q, _ = lstm(torch.zeros((a.batch, 2 * a.dim), device="cuda"))
        r = set2set_step(h, q, nodes, graph, a.batch, False)
        loss = pooled.square().mean() + r.square().mean()
        loss.backward()
        line = "step %d: %d graphs, %d nodes, loss %.5f, |grad w| %.3e" % (
            step, a.batch, n_id.numel(), loss.item(), w.grad.abs().sum().item())
        if a.composed:
            g_w = w.grad.clone()
            w.grad = None
            p2 = attention_pool(h, h @ w, nodes, graph, a.batch, True)
            r2 = set2set_step(h, q.detach(), nodes, graph, a.batch, True)
            p2.square().mean().backward()
            line += ", fused - composed: attention pool %.2e, set2set %.2e, grad w %.2e" % (
                (pooled - p2).abs().max().item(), (r - r2).abs().max().item(), (g_w - w.grad).abs().max().item())
        w.grad = None
        lstm.zero_grad()
        print(line)
    assert pooled.shape == (a.batch, a.dim) and r.shape == (a.batch, a.dim)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
