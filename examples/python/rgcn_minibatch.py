#!/usr/bin/env python3
"""Two-layer RGCN node classification on a synthetic typed graph, one optimiser step, on one MI355X.

What tf_euler/python/convolution/relation_conv.py does per block in the reference: one
[dim, fea_dim] matrix per EDGE (gathered by the edge's type), a matmul per edge, then scatter_mean
over the edges of every destination.  By linearity the matrices never have to be gathered:

    h   = relation_reduce("mean", x, src, edge_type, R, n_dst, ...)     [n_dst, R, F], one pass
    out = h.view(n_dst, R * F) @ W.permute(0, 2, 1).reshape(R * F, dim)  one GEMM

which is ops.relation_conv; the layer adds the caller's own Linear on the destination's row
(apply_node's fc(x), relation_conv.py:72-73).  The model runs twice:

  - over RelationDataFlow blocks (full neighbours; e_id = the edge type of every edge): the
    destinations are the scatter keys block.edge_index[0], the rows block.edge_index[1];
  - over sampled blocks: sample_neighbor(nodes, all_types, count) returns ids and types, `count`
    draws per destination in order - no key column, no host wait; the -1 type of a default_node
    fill drops the padding without a mask.

    python examples/python/rgcn_minibatch.py [--batch 256] [--fanout 10] [--types 4] [--dim 32]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402
from euler_amd import ops                          # noqa: E402
from euler_amd.dataflow import RelationDataFlow    # noqa: E402


class RGCNLayer(torch.nn.Module):
    def __init__(self, in_dim, dim, relations):
        super().__init__()
        self.matrix = torch.nn.Parameter(torch.randn(relations, dim, in_dim) * (in_dim ** -0.5))
        self.fc = torch.nn.Linear(in_dim, dim, bias=False)

    def forward(self, x_dst, x_src, src, edge_type, n_dst, **segments):
        """x_dst [n_dst, F] the destinations' own rows; x_src [*, F] the table `src` indexes"""
        return self.fc(x_dst) + ops.relation_conv(x_src, self.matrix, src, edge_type, n_dst, **segments)


class RGCN(torch.nn.Module):
    def __init__(self, in_dim, dim, classes, relations):
        super().__init__()
        self.l1 = RGCNLayer(in_dim, dim, relations)
        self.l2 = RGCNLayer(dim, classes, relations)


def loss_of(logits, labels):
    return torch.nn.functional.cross_entropy(logits, labels)


def full_neighbour_step(G, model, feats, labels, roots, types):
    """blocks[0] aggregates the outer layer into blocks[0].size[0] = len(roots) nodes, blocks[1]
    the layer before it; the model runs from the outermost block inwards"""
    flow = RelationDataFlow(G, [types, types])(roots)
    b0, b1 = flow.blocks
    x2 = feats[b1.n_id]                                                   # the outermost layer's rows
    x1 = feats[b0.n_id]
    h1 = torch.relu(model.l1(x1, x2, b1.edge_index[1].to(torch.int32), b1.e_id, int(b1.size[0]),
                             indices=b1.edge_index[0].to(torch.int32)))
    out = model.l2(h1[b0.res_n_id], h1, b0.edge_index[1].to(torch.int32), b0.e_id, int(b0.size[0]),
                   indices=b0.edge_index[0].to(torch.int32))
    return loss_of(out, labels[roots])


def sampled_step(G, model, feats, labels, roots, types, fanout, default_node):
    """hop 1 samples `fanout` typed neighbours of the roots, hop 2 of those; feats is indexed by node
    id (the default node has a row of its own), and the ids are read in place as int64"""
    n = roots.numel()
    ids1, _, t1 = G.sample_neighbor(roots, types, fanout, default_node=default_node)
    ids1, t1 = ids1.reshape(-1), t1.reshape(-1)
    ids2, _, t2 = G.sample_neighbor(ids1, types, fanout, default_node=default_node)
    h_roots = torch.relu(model.l1(feats[roots], feats, ids1, t1, n, count=fanout))
    h_hop1 = torch.relu(model.l1(feats[ids1], feats, ids2.reshape(-1), t2.reshape(-1), n * fanout, count=fanout))
    out = model.l2(h_roots, h_hop1, None, t1, n, count=fanout)              # update p is row p of h_hop1
    return loss_of(out, labels[roots])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--fanout", type=int, default=10)
    ap.add_argument("--types", type=int, default=4)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--in-dim", type=int, default=32)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--nodes", type=int, default=20_000)
    a = ap.parse_args()
    torch.manual_seed(0)
    G = euler_amd.Graph.synthetic(euler_amd.synth_params(20240521, a.nodes, 8 * a.nodes, n_types=a.types,
                                                         weighted=True), device=0)
    G.set_seed(7)
    default_node = a.nodes + 1
    feats = torch.randn((a.nodes + 2, a.in_dim), device="cuda")          # row = node id (last: the default node)
    labels = torch.randint(0, a.classes, (a.nodes + 2,), device="cuda")
    types = list(range(a.types))
    roots = torch.randint(1, a.nodes + 1, (a.batch,), device="cuda", dtype=torch.int64)
    for name in ("RelationDataFlow blocks", "sampled blocks"):
        model = RGCN(a.in_dim, a.dim, a.classes, a.types).cuda()
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        if name.startswith("Relation"):
            loss = full_neighbour_step(G, model, feats, labels, roots, types)
        else:
            loss = sampled_step(G, model, feats, labels, roots, types, a.fanout, default_node)
        opt.zero_grad()
        loss.backward()
        opt.step()
        grad = sum(float(p.grad.abs().sum()) for p in model.parameters())
        print("%s: loss %.6f  |grad| %.3e" % (name, float(loss), grad))
        assert torch.isfinite(loss) and grad > 0
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
