#!/usr/bin/env python3
"""LGCN (Large-Scale Learnable Graph Convolutional Networks), optimiser steps on one MI355X.

What the reference's LGCEncoder (tf_euler/python/utils/encoders.py:872-922, examples/lgcn) does per
batch:

    sample_neighbor(roots, nb_num=10)     -> [B, nb] neighbour ids (default_node fills where a
                                             node has no neighbour)
    get_dense_feature, reshape, transpose,
    tf.nn.top_k(k=3), transpose           -> per FEATURE COLUMN the k largest neighbour values
    concat with the root's own row        -> [B, k + 1, d]
    conv1d(hidden, k // 2 + 1), conv1d(out, k // 2 + 1), slice -> [B, out_dim]

The neighbour ids come from Graph.sample_neighbor; the lookup, the two transposes and the top_k are
ONE kernel, ops.gather_segment_topk, which reads the B * nb feature rows once and writes
[B, k, d] - the [B * nb, d] block never exists (--composed builds it with ops.gather and
torch.topk for the same numbers).  The feature table is a trainable embedding here, so the
gradient flows through the selected positions back into it.

    python examples/python/lgcn_minibatch.py [--steps 2] [--composed] [--batch 512] [--dim 32]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402
from euler_amd import ops                          # noqa: E402


class LGCEncoder(torch.nn.Module):
    """encoders.py:872-922 over a feature table [max_id + 1, d] (row = node id)"""

    def __init__(self, dim, k=3, hidden_dim=128, nb_num=10, out_dim=64, composed=False):
        super().__init__()
        self.k, self.nb_num, self.composed = k, nb_num, composed
        self.conv1 = torch.nn.Conv1d(dim, hidden_dim, k // 2 + 1)
        self.conv2 = torch.nn.Conv1d(hidden_dim, out_dim, k // 2 + 1)

    def topk(self, table, neighbors):
        b = neighbors.shape[0]
        if not self.composed:
            return ops.gather_segment_topk(table, neighbors.reshape(-1), b, self.k, count=self.nb_num)
        # the composition: an id that names no row reads a row of zeros, as the reference's
        # default_node fill does
        flat = neighbors.reshape(-1)
        valid = (flat >= 0) & (flat < table.shape[0])
        rows = ops.gather(table, torch.where(valid, flat, torch.zeros_like(flat))) * valid.reshape(-1, 1)
        return torch.topk(rows.view(b, self.nb_num, -1), self.k, dim=1).values

    def forward(self, G, table, roots):
        neighbors = G.sample_neighbor(roots, [0], self.nb_num)[0]           # [B, nb] int64
        top = self.topk(table, neighbors)                                   # [B, k, d]
        x = torch.cat([ops.gather(table, roots).unsqueeze(1), top], 1)      # [B, k + 1, d]
        out = self.conv2(self.conv1(x.transpose(1, 2)))                     # channels = features
        return out[:, :, 0]                                                 # [B, out_dim]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--composed", action="store_true", help="ops.gather + torch.topk instead of the fused op")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--classes", type=int, default=8)
    a = ap.parse_args()
    torch.manual_seed(0)
    G = euler_amd.Graph.synthetic(euler_amd.synth_params(11, a.nodes, 10 * a.nodes, weighted=True))
    G.set_seed(7)
    table = torch.nn.Parameter(torch.randn((a.nodes + 1, a.dim), device="cuda"))
    enc = LGCEncoder(a.dim, out_dim=a.classes, composed=a.composed).cuda()
    opt = torch.optim.Adam([table] + list(enc.parameters()), lr=0.01)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    for step in range(a.steps):
        roots = torch.randint(1, a.nodes + 1, (a.batch,), device="cuda", generator=gen)
        labels = roots % a.classes                                          # a synthetic target
        loss = torch.nn.functional.cross_entropy(enc(G, table, roots), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        print("step %d (%s): loss %.6f" % (step, "composed" if a.composed else "fused", float(loss)))
        assert torch.isfinite(loss)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
