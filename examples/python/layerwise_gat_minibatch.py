#!/usr/bin/env python3
"""One layerwise GAT layer (the reference's AttentionAggregator, utils/sparse_aggregators.py:87-139, the
default aggregator of GenieEncoder; renorm=True, 4 heads) forward and backward on one MI355X, over
Graph.sample_neighbor_layerwise(adj_format="mask") on a synthetic Graph.from_edges graph.

The adjacency stays the bit mask the sampler wrote: ops.mask_attention forms the softmax numerators from the
two score tables in registers and multiplies on the matrix units - no COO triple, no nnz, no host wait.
--composed runs the route a user had before beside it - Graph.adj_from_mask (a host wait for nnz), index arrays,
ops.attention_aggregate("additive", indices=...) with the source's own row as one more candidate - and asserts
that the two agree: the fused route rounds every numerator to bf16 where the composed one keeps fp32 weights,
so the aggregates may differ by 2 * 2^-8 * sum alpha |z| and one bf16 unit of each result.

    python examples/python/layerwise_gat_minibatch.py [--steps 5] [--composed] [--batch 8]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402
from euler_amd import ops                          # noqa: E402

UNIT, DT, HEADS = 2.0 ** -8, torch.bfloat16, 4


def composed_attention(mask, z, s_src, s_nb, root, s_root, batch, n, m):
    ind, val, _shape = euler_amd.Graph.adj_from_mask(mask, batch, n, m)
    ind = ind[val != 0]                            # (the triple's explicit zero at the corner)
    src, cand = (ind[:, 0] * n + ind[:, 1]).to(torch.int32), (ind[:, 0] * m + ind[:, 2]).to(torch.int32)
    own = torch.arange(batch * n, device=z.device, dtype=torch.int32)
    return ops.attention_aggregate("additive", s_src, torch.cat([s_nb, s_root]), torch.cat([cand, batch * m + own]), batch * n,
                                   v=torch.cat([z, root]), heads=HEADS, indices=torch.cat([src, own]))


class LayerwiseGat(torch.nn.Module):
    def __init__(self, dim, hidden, composed):
        super().__init__()
        self.composed = composed
        mk = lambda *s: torch.nn.Parameter((torch.randn(*s, device="cuda") / s[0] ** 0.5).to(DT))
        self.w, self.a_self, self.a_nb = mk(dim, hidden), mk(dim, HEADS), mk(dim, HEADS)

    def forward(self, x_self, x_all, mask, batch, n, m):
        z, root = x_all @ self.w, x_self @ self.w
        s_src, s_nb, s_root = (x_self @ self.a_self).float(), (x_all @ self.a_nb).float(), (x_self @ self.a_nb).float()
        if self.composed:
            return torch.relu(composed_attention(mask, z, s_src, s_nb, root, s_root, batch, n, m))
        return ops.mask_attention(mask, z, s_src, s_nb, batch, n, m, heads=HEADS, root=root, s_root=s_root, activation="relu")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed training steps")
    ap.add_argument("--composed", action="store_true", help="also run adj_from_mask + attention_aggregate")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--roots", type=int, default=512, help="roots per batch row")
    ap.add_argument("--layer", type=int, default=1024, help="candidates of the layer")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nodes", type=int, default=100000)
    a = ap.parse_args()
    torch.manual_seed(0)
    edges = torch.randint(1, a.nodes + 1, (2, 20 * a.nodes), device="cuda")
    G = euler_amd.Graph.from_edges(edges, undirected=True)
    G.set_seed(7)
    table = torch.randn((a.nodes + 1, a.dim), device="cuda").to(DT)
    roots = torch.randint(1, a.nodes + 1, (a.batch, a.roots), device="cuda")
    nb, mask = G.sample_neighbor_layerwise(roots, [0], a.layer, default_node=0, call_id=0, adj_format="mask")
    x_self, x_all = ops.gather(table, roots.reshape(-1)), ops.gather(table, nb.reshape(-1))
    args = (x_self, x_all, mask, a.batch, a.roots, a.layer)
    outs = {}
    for name, composed in ({"fused": False, "composed": True} if a.composed else {"fused": False}).items():
        torch.manual_seed(1)        # the same weights on both routes
        net = LayerwiseGat(a.dim, a.dim, composed)
        outs[name] = net(*args).detach()
        step = lambda: net(*args).float().square().mean().backward()
        step()                                                                        # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        print("%s: step %.3f ms, peak %d bytes above the inputs" % (name, ms, torch.cuda.max_memory_allocated() - base))
        assert all(torch.isfinite(p.grad.float()).all() for p in net.parameters())
    if a.composed:
        with torch.no_grad():       # sum alpha |z|: the composed route over |z| and |root|
            z, root = (x_all @ net.w).abs(), (x_self @ net.w).abs()
            s = [(x_self @ net.a_self).float(), (x_all @ net.a_nb).float(), (x_self @ net.a_nb).float()]
            mag = composed_attention(mask, z, s[0], s[1], root, s[2], a.batch, a.roots, a.layer).double()
        err = (outs["fused"].double() - outs["composed"].double()).abs()
        bound = 2 * UNIT * mag + UNIT * (outs["fused"].double().abs() + outs["composed"].double().abs())
        assert torch.all(err <= bound), "the two routes disagree"
        print("the two routes agree: largest difference / bound %.3g" % float((err / bound.clamp_min(1e-300)).max()))


if __name__ == "__main__":
    main()
