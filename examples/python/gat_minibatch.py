#!/usr/bin/env python3
"""One GAT layer on a sampled block, trained for a few steps end to end on one MI355X.

What tf_euler/python/convolution/gat_conv.py does per block in the reference: a logit per edge and
head from the two endpoints, scatter_softmax over the edges of every destination (gat_conv.py:66-72),
and the sum of the neighbours' rows weighted by the result.  Here no [E, D] block exists at any
point - neither gathered rows nor messages:

    s_i, s_j = h @ a_i, h @ a_j                              per-NODE scores, [N, H]
    logits   = leaky_relu(gather(s_i, dst) + gather(s_j, src))          [E, H]
    alpha    = edge_softmax(logits, count=fanout)                        [E, H], one read, one write
    out      = gather_segment_reduce("add", h, src, n, count=fanout, edge_weight=alpha)

and autograd runs back through all of it (edge_softmax's gradient is its own kernel; the weighted
reduce returns the gradient of alpha through edge_dot).

    python examples/python/gat_minibatch.py [--batch 1024] [--fanout 10] [--heads 4] [--dim 16] [--steps 3]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402
from euler_amd import ops                          # noqa: E402


class GATLayer(torch.nn.Module):
    def __init__(self, in_dim, heads, dim):
        super().__init__()
        self.heads, self.dim = heads, dim
        self.lin = torch.nn.Linear(in_dim, heads * dim, bias=False)
        self.att_i = torch.nn.Parameter(torch.randn(heads, dim) * 0.1)
        self.att_j = torch.nn.Parameter(torch.randn(heads, dim) * 0.1)

    def forward(self, x, dst, src, n_dst, fanout):
        """x [N, in_dim]; dst / src [n_dst * fanout] rows of x, the edges of a destination adjacent"""
        h = self.lin(x)                                                  # [N, H * F]
        hh = h.view(-1, self.heads, self.dim)
        s_i = (hh * self.att_i).sum(-1)                                  # [N, H]
        s_j = (hh * self.att_j).sum(-1)
        logits = torch.nn.functional.leaky_relu(ops.gather(s_i, dst) + ops.gather(s_j, src), 0.2)
        alpha = ops.edge_softmax(logits, count=fanout, size=n_dst)
        return ops.gather_segment_reduce("add", h, src, n_dst, count=fanout, edge_weight=alpha), alpha


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--fanout", type=int, default=10)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--in-dim", type=int, default=32)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=50_000)
    a = ap.parse_args()
    torch.manual_seed(0)
    G = euler_amd.Graph.synthetic(euler_amd.synth_params(20240521, a.nodes, 10 * a.nodes, weighted=True), device=0)
    G.set_seed(7)
    feats = torch.randn((a.nodes + 2, a.in_dim), device="cuda")          # row = node id (last: the default node)
    layer = GATLayer(a.in_dim, a.heads, a.dim).cuda()
    opt = torch.optim.SGD(layer.parameters(), lr=0.05)
    for step in range(a.steps):
        roots = torch.randint(1, a.nodes + 1, (a.batch,), device="cuda", dtype=torch.int64)
        ids, _, _ = G.sample_fanout(roots, [[0]], [a.fanout], a.nodes + 1, call_id=step)
        src = ids[1].to(torch.int32)                                     # [batch * fanout] neighbour ids
        dst = roots.to(torch.int32).repeat_interleave(a.fanout)
        out, alpha = layer(feats, dst, src, a.batch, a.fanout)
        loss = (out - 1.0).square().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        rows = alpha.detach().view(a.batch, a.fanout, a.heads).sum(1)
        print("step %d: loss %.6f, attention rows sum to 1 within %.1e, |grad att_i| %.3e"
              % (step, float(loss), float((rows - 1).abs().max()), float(layer.att_i.grad.abs().sum())))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
