#!/usr/bin/env python3
"""A two-layer layerwise GCN (the reference's GCNEncoder over LayerwiseDataFlow: utils/sparse_aggregators.py:
37-54, GCNAggregator with renorm) forward and backward on one MI355X, over Graph.sample_neighbor_layerwise
(adj_format="mask") on a synthetic Graph.from_edges graph.

Each layer's adjacency stays the bit mask the sampler wrote: ops.mask_aggregate("gcn_renorm") multiplies by
it on the matrix units, and its backward transposes the mask and runs the same kernel - no COO triple, no nnz,
no host wait in the step.  --composed runs the route a user had before beside it: Graph.adj_from_mask (a host
wait for nnz), the edge list, ops.gather_scatter and the division in torch.  Every aggregate of the fused route
is asserted to agree with the composed one on the same inputs within twice the bound of
tests/test_mask_aggregate_gpu.py (each route is within it of the exact value), and ms per step and peak device
bytes are printed per route.

    python examples/python/layerwise_gcn_minibatch.py [--steps 5] [--composed] [--batch 8]
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

U24, UNIT, DT = 2.0 ** -24, 2.0 ** -8, torch.bfloat16


def composed_aggregate(mask, x, root, batch, n, m):
    """(root + A @ x) / (1 + deg) through the COO triple and gather_scatter; the sums in fp32"""
    ind, val, _shape = euler_amd.Graph.adj_from_mask(mask, batch, n, m)
    ind = ind[val != 0]                            # (the triple's explicit zero at the corner)
    src, cand = ind[:, 0] * n + ind[:, 1], ind[:, 0] * m + ind[:, 2]
    s = ops.gather_scatter("add", x, cand, src, batch * n, out_dtype=torch.float32)
    deg = torch.bincount(src, minlength=batch * n).reshape(-1, 1)
    return ((root.float() + s) / (1 + deg)).to(x.dtype)


class LayerwiseGcn(torch.nn.Module):
    def __init__(self, dim, hidden, composed):
        super().__init__()
        self.composed, self.worst = composed, 0.0
        mk = lambda *s: torch.nn.Parameter((torch.randn(*s, device="cuda") / s[0] ** 0.5).to(DT))
        self.w1, self.w2 = mk(dim, hidden), mk(hidden, hidden)

    def aggregate(self, mask, x, root, batch, n, m, check):
        if self.composed:
            return composed_aggregate(mask, x, root, batch, n, m)
        out = ops.mask_aggregate("gcn_renorm", mask, x, batch, n, m, root=root)
        if check:
            with torch.no_grad():
                other = composed_aggregate(mask, x, root, batch, n, m).double()
                mag, deg = ops.mask_aggregate("add", mask, x.abs(), batch, n, m, out_dtype=torch.float32, return_degree=True)
                deg = deg.double().reshape(-1, 1)
                bound = 4 * (deg + 2) * U24 * (root.abs().double() + mag.double()) / (1 + deg) + UNIT * other.abs()
                err = (out.double() - other).abs()
                assert torch.all(err <= 2 * bound), "the two routes disagree"
                self.worst = max(self.worst, float((err / (2 * bound).clamp_min(1e-300)).max()))
        return out

    def forward(self, feats, masks, shape, check=False):
        """feats: the rows of (roots, layer 1, layer 2); masks: (roots x layer 1, layer 1 x layer 2)"""
        batch, n0, m1, m2 = shape
        h1 = torch.relu(self.aggregate(masks[1], feats[2], feats[1], batch, m1, m2, check) @ self.w1)
        h0 = torch.relu(feats[0] @ self.w1)        # the roots' own layer-1 embedding: their self term alone
        return self.aggregate(masks[0], h1, h0, batch, n0, m1, check) @ self.w2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed training steps")
    ap.add_argument("--composed", action="store_true", help="also run adj_from_mask + gather_scatter")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--roots", type=int, default=512, help="roots per batch row")
    ap.add_argument("--layer", type=int, nargs=2, default=[1024, 2048], help="candidates of layer 1 and 2")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nodes", type=int, default=100000)
    a = ap.parse_args()
    torch.manual_seed(0)
    edges = torch.randint(1, a.nodes + 1, (2, 20 * a.nodes), device="cuda")
    G = euler_amd.Graph.from_edges(edges, undirected=True)
    G.set_seed(7)
    table = torch.randn((a.nodes + 1, a.dim), device="cuda").to(DT)
    roots = torch.randint(1, a.nodes + 1, (a.batch, a.roots), device="cuda")
    m1, m2 = a.layer
    # (default_node 0: a layer without neighbours fills with id 0, row 0 of the table)
    nb1, mask1 = G.sample_neighbor_layerwise(roots, [0], m1, default_node=0, call_id=0, adj_format="mask")
    nb2, mask2 = G.sample_neighbor_layerwise(nb1, [0], m2, default_node=0, call_id=1, adj_format="mask")
    feats = [ops.gather(table, t.reshape(-1)) for t in (roots, nb1, nb2)]
    shape = (a.batch, a.roots, m1, m2)
    for name, composed in ({"fused": False, "composed": True} if a.composed else {"fused": False}).items():
        torch.manual_seed(1)        # the same weights on both routes
        net = LayerwiseGcn(a.dim, a.dim, composed)
        step = lambda check=False: net(feats, (mask1, mask2), shape, check).float().square().mean().backward()
        step(check=a.composed and not composed)                                       # warm-up, and the check
        if a.composed and not composed:
            print("fused vs composed over both layers: largest difference / (2 x bound) %.3g" % net.worst)
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
        print("the two routes agree within the bound")


if __name__ == "__main__":
    main()
