#!/usr/bin/env python3
"""One AGNN layer on a sampled block, trained for a few steps end to end on one MI355X.

What tf_euler/python/convolution/agnn_conv.py:36-54 does per block in the reference: the cosine of
the two endpoints times a learnable beta as the logit of an edge, scatter_softmax over the edges of
every destination, and the sum of the neighbours' rows weighted by the result.  Here it is ONE op:

    xn  = l2norm(x)
    out = attention_aggregate("dot", beta * xn, xn, src, n_dst, v=x, q_index=roots, count=fanout)

beta is a learnable temperature, so it lives in q (the op's `scale` is a plain float).  --composed
also runs the three-op formulation (edge_dot, edge_softmax, weighted gather_segment_reduce) on the
same block and prints the largest difference of the outputs and of beta's gradient.

    python examples/python/agnn_minibatch.py [--batch 1024] [--fanout 10] [--dim 64] [--steps 3] [--composed]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402
from euler_amd import ops                          # noqa: E402


class AGNNLayer(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.beta = torch.nn.Parameter(torch.ones(1))

    def forward(self, x, roots, src, fanout, composed=False):
        """x [N, D]; roots [n_dst] and src [n_dst * fanout] rows of x, a destination's edges adjacent"""
        xn = torch.nn.functional.normalize(x, p=2.0, dim=-1)
        n_dst = roots.numel()
        if not composed:
            return ops.attention_aggregate("dot", self.beta * xn, xn, src, n_dst, v=x, q_index=roots, count=fanout)
        dst = roots.repeat_interleave(fanout)
        logits = ops.edge_dot(self.beta * xn, dst, xn, src)
        alpha = ops.edge_softmax(logits, count=fanout, size=n_dst)
        return ops.gather_segment_reduce("add", x, src, n_dst, count=fanout, edge_weight=alpha)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--fanout", type=int, default=10)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--composed", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    G = euler_amd.Graph.synthetic(euler_amd.synth_params(20240521, a.nodes, 10 * a.nodes, weighted=True), device=0)
    G.set_seed(7)
    feats = torch.randn((a.nodes + 2, a.dim), device="cuda", requires_grad=True)   # row = node id
    layer = AGNNLayer().cuda()
    opt = torch.optim.SGD(list(layer.parameters()) + [feats], lr=0.05)
    for step in range(a.steps):
        roots = torch.randint(1, a.nodes + 1, (a.batch,), device="cuda", dtype=torch.int64)
        ids, _, _ = G.sample_fanout(roots, [[0]], [a.fanout], a.nodes + 1, call_id=step)
        src, r32 = ids[1].to(torch.int32), roots.to(torch.int32)
        out = layer(feats, r32, src, a.fanout)
        loss = (out - 1.0).square().mean()
        opt.zero_grad()
        loss.backward()
        line = "step %d: loss %.6f, |grad beta| %.3e" % (step, float(loss), float(layer.beta.grad.abs().sum()))
        if a.composed:
            g_beta = layer.beta.grad.clone()
            layer.beta.grad = None
            other = layer(feats, r32, src, a.fanout, composed=True)
            (other - 1.0).square().mean().backward()
            line += ", fused - composed: out %.2e, grad beta %.2e" % (
                float((out - other).abs().max()), float((g_beta - layer.beta.grad).abs().max()))
            layer.beta.grad = g_beta
        opt.step()
        print(line)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
