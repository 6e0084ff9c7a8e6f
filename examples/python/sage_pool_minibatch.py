#!/usr/bin/env python3
"""GraphSAGE with the maxpool aggregator on a sampled 2-hop block, forward steps on one MI355X.

What the reference's SageEncoder(aggregator='maxpool') (tf_euler/python/utils/encoders.py with
utils/aggregators.py:75-114) does per layer and hop:

    neigh = reduce_max(relu(dense(neighbour features)), over the fan-out)
    out   = relu(self_dense(self features) + neigh_dense(neigh))

The neighbour ids come from Graph.sample_fanout.  dense + relu + reduce_max over the gathered rows
is ONE kernel, ops.pool_aggregate: it reads every neighbour row once and writes [n_dst, F] - neither
the [e, d] gathered block nor the [e, F] activation block exists.  --composed runs ops.gather +
matmul + relu + ops.scatter_max beside it and prints ms per step and peak device bytes of both
routes; --check compares the two routes' hop-2 aggregation with each other under the rounding
bound of both against exact arithmetic.  --fused-backward also TRAINS: a step (forward, a loss, backward) through
backward="recompute" and through backward="fused" (euler_gpu_pool_aggregate_backward: the gradients on the matrix
units, no Python loop), ms per step and peak bytes of both, and the two routes' weight and bias gradients of the
hop-2 aggregation against each other.

    python examples/python/sage_pool_minibatch.py [--steps 5] [--composed] [--check] [--fused-backward] [--batch 4096]
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


def rows_of(table, ids):
    """table[ids]; an id that names no row reads a row of zeros, as the reference's default_node fill does"""
    ids = ids.reshape(-1)
    valid = (ids >= 0) & (ids < table.shape[0])
    return ops.gather(table, torch.where(valid, ids, torch.zeros_like(ids))) * valid.reshape(-1, 1)


class PoolSageLayer(torch.nn.Module):
    def __init__(self, dim, hidden, dtype, composed, backward="recompute"):
        super().__init__()
        self.composed, self.backward = composed, backward
        mk = lambda *s: torch.nn.Parameter((torch.randn(*s, device="cuda") / s[0] ** 0.5).to(dtype))
        self.pool_w, self.pool_b = mk(dim, hidden), torch.nn.Parameter(torch.zeros(hidden, device="cuda"))
        self.self_w, self.neigh_w = mk(dim, hidden), mk(hidden, hidden)

    def aggregate(self, table, ids, n_dst, count):
        """[n_dst, hidden]: max over each destination's `count` neighbours of relu(row @ W + b); ids None:
        neighbour p is row p of table"""
        if not self.composed:
            return ops.pool_aggregate("max", table, self.pool_w, ids, n_dst, bias=self.pool_b, count=count,
                                      backward=self.backward)
        rows = table if ids is None else rows_of(table, ids)
        h = torch.relu(torch.addmm(self.pool_b.to(rows.dtype), rows, self.pool_w))
        dst = torch.arange(n_dst, device="cuda", dtype=torch.int32).repeat_interleave(count)
        return ops.scatter_max(h, dst, n_dst)

    def forward(self, self_rows, table, ids, count):
        neigh = self.aggregate(table, ids, self_rows.shape[0], count)
        return torch.relu(self_rows @ self.self_w + neigh @ self.neigh_w)


def encode(layers, table, nodes, fanouts):
    """two layers over the block nodes[0] (roots), nodes[1], nodes[2]"""
    h0 = layers[0](rows_of(table, nodes[0]), table, nodes[1], fanouts[0])
    h1 = layers[0](rows_of(table, nodes[1]), table, nodes[2], fanouts[1])
    return layers[1](h0, h1, None, fanouts[0])


def check(layer_f, layer_c, table, ids, n_dst, count):
    """both routes of one aggregation against float64 on the CPU: each within 4 (d + 2) 2^-24 |x||w| (the
    accumulation, with the margin of the tests) + 2^-8 |result| (one rounding to bf16), so they differ
    by at most twice that"""
    fused = layer_f.aggregate(table, ids, n_dst, count).double().cpu()
    composed = layer_c.aggregate(table, ids, n_dst, count).double().cpu()
    ids = ids.cpu()
    valid = (ids >= 0) & (ids < table.shape[0])
    x = table.double().cpu()[torch.where(valid, ids, torch.zeros_like(ids))] * valid[:, None]
    w, b = layer_f.pool_w.detach().double().cpu(), layer_f.pool_b.detach().double().cpu()
    ref = torch.relu(x @ w + b).view(n_dst, count, -1).amax(1)
    mag = (x.abs() @ w.abs() + b.abs()).view(n_dst, count, -1).amax(1)
    bound = 4 * (table.shape[1] + 2) * 2.0 ** -24 * mag + 2.0 ** -8 * ref.abs()
    worst = float(((fused - composed).abs() / (2 * bound).clamp_min(1e-300)).max())
    print("fused vs composed: largest difference / bound %.3f" % worst)
    assert torch.all((fused - ref).abs() <= bound) and torch.all((fused - composed).abs() <= 2 * bound)
    print("routes agree within the bound")


U = 2.0 ** -24


def check_backward(layer_r, layer_f, table, ids, count, n=1024):
    """the hop-2 aggregation's weight and bias gradients of both backward routes, over its first n destinations,
    against each other.  Each is within B of float64 autograd, so they differ by 2 B at most: B = M ((1 + 2^-8)^2 - 1 +
    4 (terms + 2) 2^-24) + 2^-8 M, M the gradient of the same graph on absolute values with the masks and the selection
    held, terms = n count + d + F, the narrowings being the dZ operand and the stored gradient
    (tests/test_pool_aggregate_backward_gpu.py).  Where a pre-activation lies within the forward's bound of 0, or the
    two largest candidates of a (destination, column) within twice it of each other, the routes may disagree on the mask
    or the selection: those elements get no incoming gradient."""
    n = min(n, ids.numel() // count)
    ids = ids.reshape(-1)[:n * count]
    at = ids.cpu()
    valid = (at >= 0) & (at < table.shape[0])
    x = table.double().cpu()[torch.where(valid, at, torch.zeros_like(at))] * valid[:, None]
    w, b = layer_f.pool_w.detach().double().cpu(), layer_f.pool_b.detach().double().cpu()
    (d, f), shape = w.shape, (n, count, w.shape[1])
    z, fwd = (x @ w + b).view(shape), (4 * (d + 2) * U * (x.abs() @ w.abs() + b.abs())).view(shape)
    top = torch.topk(torch.relu(z), 2, dim=1).values
    sure = (top[:, 0] - top[:, 1] > 2 * fwd.amax(1)) & (z.abs() > fwd).all(1)
    g = (torch.randn(n, f, generator=torch.Generator().manual_seed(3)) * sure).to(torch.bfloat16)
    picked = ((torch.relu(z) == top[:, :1]) & (z > 0)).double()
    mags = [w.abs().requires_grad_(True), b.abs().requires_grad_(True)]
    ((x.abs() @ mags[0] + mags[1]).view(shape) * picked * g.double().abs()[:, None]).sum().backward()
    got = []
    for layer in (layer_r, layer_f):
        layer.pool_w.grad = layer.pool_b.grad = None
        layer.aggregate(table, ids, n, count).backward(g.cuda())
        got.append([layer.pool_w.grad.double().cpu(), layer.pool_b.grad.double().cpu()])
    worst = 0.0
    for k, a, c, m in zip(("pool_w", "pool_b"), got[0], got[1], mags):
        bound = 2 * ((1 + 2.0 ** -8) ** 2 - 1 + 4 * (n * count + d + f + 2) * U + 2.0 ** -8) * m.grad
        worst = max(worst, float(((a - c).abs() / bound.clamp(min=1e-300)).max()))
        assert torch.all((a - c).abs() <= bound), k
    print("recompute vs fused backward: largest difference / bound %.3f" % worst)
    print("fused backward agrees within the bound")


def train(name, layers, table, nodes, fanouts, steps):
    """ms per training step (forward, a loss, backward) and its peak bytes"""
    params = [p for layer in layers for p in layer.parameters()]

    def step():
        for p in params:
            p.grad = None
        encode(layers, table, nodes, fanouts).float().square().mean().backward()

    step()                                                                             # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    assert all(torch.isfinite(p.grad.float()).all() for p in params)
    print("%s: training, %.3f ms per step, peak %d bytes above the inputs"
          % (name, ms, torch.cuda.max_memory_allocated() - base))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--composed", action="store_true", help="also run gather + matmul + relu + scatter_max")
    ap.add_argument("--check", action="store_true", help="compare the two routes' hop-2 aggregation")
    ap.add_argument("--fused-backward", action="store_true", help="also train through both backward routes")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--nodes", type=int, default=200000)
    a = ap.parse_args()
    fanouts = [25, 10]
    torch.manual_seed(0)
    G = euler_amd.Graph.synthetic(euler_amd.synth_params(11, a.nodes, 10 * a.nodes, weighted=True))
    G.set_seed(7)
    table = torch.randn((a.nodes + 1, a.dim), device="cuda").to(torch.bfloat16)
    routes = {"fused": False, "composed": True} if a.composed or a.check else {"fused": False}
    models = {}
    for name, composed in routes.items():
        torch.manual_seed(1)        # the same weights on both routes
        models[name] = [PoolSageLayer(a.dim, a.hidden, torch.bfloat16, composed),
                        PoolSageLayer(a.hidden, a.hidden, torch.bfloat16, composed)]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    roots = torch.randint(1, a.nodes + 1, (a.batch,), device="cuda", generator=gen)
    nodes = G.sample_fanout(roots, [[0], [0]], fanouts, a.nodes + 1, call_id=0)[0]     # fills name no row
    with torch.no_grad():
        for name, layers in models.items():
            encode(layers, table, nodes, fanouts)                                      # warm-up
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                out = encode(layers, table, nodes, fanouts)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
            assert torch.isfinite(out.float()).all()
            print("%s: %.3f ms per step, peak %d bytes above the inputs"
                  % (name, ms, torch.cuda.max_memory_allocated() - base))
        if a.check:
            check(models["fused"][0], models["composed"][0], table, nodes[2].reshape(-1), nodes[1].numel(), fanouts[1])
    if a.fused_backward:
        torch.manual_seed(1)        # the same weights again
        trained = [PoolSageLayer(a.dim, a.hidden, torch.bfloat16, False, "fused"),
                   PoolSageLayer(a.hidden, a.hidden, torch.bfloat16, False, "fused")]
        train("recompute backward", models["fused"], table, nodes, fanouts, a.steps)
        train("fused backward", trained, table, nodes, fanouts, a.steps)
        check_backward(models["fused"][0], trained[0], table, nodes[2], fanouts[1])


if __name__ == "__main__":
    main()
