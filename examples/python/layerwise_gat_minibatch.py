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
--fused-backward trains the same layer once more with ops.mask_attention(backward="fused") - the two gradient kernels
instead of the recomputation in torch ops - prints its step time and peak beside the others and asserts, on the first
batch row, that the op's five gradients agree between the two routes: each is within the bound of
tests/test_mask_attention_backward_gpu.py of the exact gradient - `unit` times the sum of the absolute values of an
element's own terms - so they differ by at most twice that, plus one bf16 unit of each result for d z and d root.
(That comparison runs without relu: the recomputation gates by the sign of its own fp32 output, the kernels by the saved
one, and an output whose sign differs in the last bit would count as a gradient error.  Where a pre-activation is exactly
0 the two routes take different subgradients of the leaky relu; those score gradients are left out.)

    python examples/python/layerwise_gat_minibatch.py [--steps 5] [--composed] [--fused-backward] [--batch 8]
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


def backward_routes_agree(mask, tensors, n, m):
    """the five gradients of one batch row by backward="recompute" and by backward="fused" under the same incoming
    gradient, each element held to the sum of the two routes' bounds; -> the largest difference / bound"""
    z, s_src, s_nb, root, s_root = tensors
    dh = z.shape[1] // HEADS
    grad = torch.randn((n, z.shape[1]), device="cuda").to(DT)
    got = {}
    for route in ("recompute", "fused"):
        leaves = [t.detach().requires_grad_(True) for t in tensors]
        out = ops.mask_attention(mask, leaves[0], leaves[1], leaves[2], 1, n, m, heads=HEADS, root=leaves[3], s_root=leaves[4],
                                 backward=route)
        got[route] = [g.double() for g in torch.autograd.grad(out, leaves, grad)]
    with torch.no_grad():           # alpha and the sum of |terms| of every element, from the dense composed form in float64
        bits = ((mask.view(torch.int64)[:, :, None] >> torch.arange(64, device="cuda")) & 1).reshape(n, -1)[:, :m].bool()
        leaky = lambda v: torch.where(v < 0, 0.2 * v, v)
        e = leaky(s_src.double()[:, None] + s_nb.double()[None]).masked_fill(~bits[:, :, None], float("-inf"))
        e = torch.cat([e, leaky(s_src.double() + s_root.double())[:, None]], 1)
        alpha, emax = torch.softmax(e, 1), float(e[e.isfinite()].abs().max())
        big = grad.double().abs().view(n, HEADS, dh)
        za, ra, nb = z.double().abs().view(m, HEADS, dh), root.double().abs().view(n, HEADS, dh), alpha[:, :m]
        mag = torch.einsum("nmh,mhd->nhd", nb, za) + alpha[:, m, :, None] * ra
        dot = (big * mag).sum(-1)
        t = nb * (torch.einsum("nhd,mhd->nmh", big, za) + dot[:, None])
        t0 = alpha[:, m] * ((big * ra).sum(-1) + dot)
        terms = [torch.einsum("nmh,nhd->mhd", nb, big).reshape(m, -1), t.sum(1) + t0, t.sum(0),
                 (big * alpha[:, m, :, None]).reshape(n, -1), t0]
        # the fused route's unit and the recomputation's (the headers of the two test files derive them)
        unit = (12 * emax + 4 * (max(m, n) + 1 + dh + 3)) * 2.0 ** -24 + 4 * 1.77e-6 + 3 * UNIT \
            + (12 * emax + 4 * (m + dh + 4)) * 2.0 ** -24
        # a pre-activation of exactly 0 (bf16 scores meet): torch's leaky_relu takes the slope there, the kernels 1 as
        # AttAdditiveGrad does - the score gradients of that source and candidate are not compared
        kink = ((s_src.double()[:, None] + s_nb.double()[None]) == 0) & bits[:, :, None]
        kink0 = (s_src.double() + s_root.double()) == 0
        skip = [None, kink.any(1) | kink0, kink.any(0), None, kink0]
        worst = 0.0
        for k, (p, q, lim) in enumerate(zip(got["recompute"], got["fused"], terms)):
            lim = unit * lim + (UNIT * (p.abs() + q.abs()) if k in (0, 3) else 0)
            if skip[k] is not None:
                lim = lim.masked_fill(skip[k], float("inf"))
            worst = max(worst, float(((p - q).abs() / lim.clamp_min(1e-300)).max()))
    assert worst <= 1.0, "the two backward routes disagree: %.3g of the bound" % worst
    return worst


class LayerwiseGat(torch.nn.Module):
    def __init__(self, dim, hidden, composed, backward="recompute"):
        super().__init__()
        self.composed, self.backward = composed, backward
        mk = lambda *s: torch.nn.Parameter((torch.randn(*s, device="cuda") / s[0] ** 0.5).to(DT))
        self.w, self.a_self, self.a_nb = mk(dim, hidden), mk(dim, HEADS), mk(dim, HEADS)

    def forward(self, x_self, x_all, mask, batch, n, m):
        z, root = x_all @ self.w, x_self @ self.w
        s_src, s_nb, s_root = (x_self @ self.a_self).float(), (x_all @ self.a_nb).float(), (x_self @ self.a_nb).float()
        if self.composed:
            return torch.relu(composed_attention(mask, z, s_src, s_nb, root, s_root, batch, n, m))
        return ops.mask_attention(mask, z, s_src, s_nb, batch, n, m, heads=HEADS, root=root, s_root=s_root, activation="relu",
                                  backward=self.backward)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed training steps")
    ap.add_argument("--composed", action="store_true", help="also run adj_from_mask + attention_aggregate")
    ap.add_argument("--fused-backward", action="store_true", help="also train with mask_attention(backward=\"fused\")")
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
    names = ["fused"] + ["composed"] * a.composed + ["fused-backward"] * a.fused_backward
    for name in names:
        torch.manual_seed(1)        # the same weights on every route
        net = LayerwiseGat(a.dim, a.dim, name == "composed", "fused" if name == "fused-backward" else "recompute")
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
    if a.fused_backward:
        with torch.no_grad():
            x_s, x_a = x_self[:a.roots], x_all[:a.layer]
            t = [x_a @ net.w, (x_s @ net.a_self).float(), (x_a @ net.a_nb).float(), x_s @ net.w, (x_s @ net.a_nb).float()]
        worst = backward_routes_agree(mask[:a.roots], t, a.roots, a.layer)
        print("the two backward routes agree: largest difference / bound %.3g" % worst)
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
