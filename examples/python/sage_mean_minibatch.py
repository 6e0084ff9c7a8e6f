#!/usr/bin/env python3
"""GraphSAGE with the mean aggregator (SageEncoder's default) on a sampled 2-hop block, training steps
on one MI355X.

What the reference's MeanAggregator (tf_euler/python/utils/aggregators.py:38-72) does per layer and hop:

    out = relu(self_dense(self features)) + relu(neigh_dense(mean over the fan-out of neighbour features))

The neighbour ids come from Graph.sample_fanout.  The mean, both dense layers, the activations and the
add are ONE kernel per hop, ops.aggregate_dense: the [n_dst, d] aggregate and the two [n_dst, F] partial
results are never written.  --composed runs ops.gather_segment_reduce + two matmuls + relu + add beside
it, asserts that the two routes' hop-2 layer agree within the rounding bound of both against float64
(the bound of tests/test_aggregate_dense_gpu.py), and prints ms per step (forward and backward through
both layers) and peak device bytes of both routes.  --fp8-features also runs layer 0 of the outermost hop
over the features as an ops.Fp8Rows table (a quarter of their fp32 bytes; the sampler's ids go in as
gather_indices and root_index), asserts it against float64 on the dequantised table within the bound of
tests/test_fp8_dense_gpu.py, and prints its relative error against the bf16-feature run.  The synthetic
graph carries no float features, so the table is quantised from the example's own id-indexed rows; with
features in the graph it is G.fp8_dense_feature(fid, dim).  --fused-backward adds a third route, the fused op
with backward="fused" (euler_gpu_aggregate_dense_backward: no Python loop, no fp32 [rows, d] scatter result
per chunk), prints its step time and peak beside the others, and asserts the hop-2 layer's weight and bias
gradients of the two backward routes against each other within the bound of
tests/test_aggregate_dense_backward_gpu.py.

    python examples/python/sage_mean_minibatch.py [--steps 5] [--composed] [--fused-backward] [--batch 4096]
                                                  [--fp8-features]
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

U = 2.0 ** -24


class MeanSageLayer(torch.nn.Module):
    def __init__(self, dim, hidden, dtype, composed, backward="recompute"):
        super().__init__()
        self.composed, self.backward = composed, backward
        mk = lambda *s: torch.nn.Parameter((torch.randn(*s, device="cuda") / s[0] ** 0.5).to(dtype))
        self.self_w, self.neigh_w = mk(dim, hidden), mk(dim, hidden)
        self.bias = torch.nn.Parameter(torch.zeros(hidden, device="cuda"))

    def forward(self, self_rows, table, ids, count):
        """[n_dst, hidden]; ids None: neighbour p is row p of table"""
        n_dst = self_rows.shape[0]
        if not self.composed:
            return ops.aggregate_dense("mean", table, self.neigh_w, ids, n_dst, root=self_rows, root_weight=self.self_w,
                                       bias=self.bias, count=count, backward=self.backward)
        if ids is None:
            ids = torch.arange(table.shape[0], device="cuda", dtype=torch.int32)
        agg = ops.gather_segment_reduce("mean", table, ids.reshape(-1), n_dst, count=count)
        return torch.relu(torch.addmm(self.bias.to(agg.dtype), agg, self.neigh_w)) + torch.relu(self_rows @ self.self_w)


def encode(layers, table, nodes, fanouts):
    """two layers over the block nodes[0] (roots), nodes[1], nodes[2]"""
    h0 = layers[0](ops.gather(table, nodes[0].reshape(-1)), table, nodes[1], fanouts[0])
    h1 = layers[0](ops.gather(table, nodes[1].reshape(-1)), table, nodes[2], fanouts[1])
    return layers[1](h0, h1, None, fanouts[0])


def check(layer_f, layer_c, table, self_ids, ids, count, n=4096):
    """the hop-2 layer of both routes, its first n destinations, against float64 on the CPU.  With M the formula
    on absolute values: the fused route is within (4 (d + ds + 2) + count + 4) 2^-24 M (accumulation with the
    tests' margin, fold, mean) + 2^-8 M (the one narrowing of the aggregate) + 2^-8 |result| (the bf16 output);
    the composed route also rounds each path's matmul result and activation sum to bf16: 2 x 2^-8 M more."""
    n = min(n, self_ids.numel())
    self_ids, ids = self_ids.reshape(-1)[:n], ids.reshape(-1)[:n * count]
    with torch.no_grad():
        rows = ops.gather(table, self_ids)
        fused = layer_f(rows, table, ids, count).double().cpu()
        composed = layer_c(rows, table, ids, count).double().cpu()
    t64 = table.double().cpu()
    x, r = t64[ids.cpu()].view(n, count, -1), t64[self_ids.cpu()]
    wn, ws, b = [p.detach().double().cpu() for p in (layer_f.neigh_w, layer_f.self_w, layer_f.bias)]
    a = x.mean(1).to(torch.bfloat16).double()
    ref = torch.relu(a @ wn + b) + torch.relu(r @ ws)
    mag = x.abs().mean(1) @ wn.abs() + b.abs() + r.abs() @ ws.abs()
    d = table.shape[1]
    bound_f = ((4 * (2 * d + 2) + count + 4) * U + 2.0 ** -8) * mag + 2.0 ** -8 * ref.abs()
    bound_c = bound_f + 2 * 2.0 ** -8 * mag
    print("fused vs float64: largest error / bound %.3f; fused vs composed: %.3f"
          % (float(((fused - ref).abs() / bound_f).max()), float(((fused - composed).abs() / (bound_f + bound_c)).max())))
    assert torch.all((fused - ref).abs() <= bound_f) and torch.all((fused - composed).abs() <= bound_f + bound_c)
    print("routes agree within the bound")


def check_backward(layer_r, layer_f, table, self_ids, ids, count, n=1024):
    """the hop-2 layer's gradients of both backward routes, over its first n destinations, against each other.  Each
    is within B of float64 autograd, so they differ by 2 B at most: B = M ((1 + 2^-8)^3 - 1 + 4 (terms + 2) 2^-24) + 2^-8
    |gradient| for the bf16 bias, M the gradient of the same graph on absolute values with the masks held, terms = n count
    + 2 d + F, the three narrowings A, dZ and the stored gradient (tests/test_aggregate_dense_backward_gpu.py).  Where a
    pre-activation lies within the forward's bound of 0 the routes may disagree on its mask: those elements get no
    incoming gradient."""
    n = min(n, self_ids.numel())
    self_ids, ids = self_ids.reshape(-1)[:n], ids.reshape(-1)[:n * count]
    t64 = table.double().cpu()
    x, r = t64[ids.cpu()].view(n, count, -1), t64[self_ids.cpu()]
    names = ("neigh_w", "self_w", "bias")
    leaves = [getattr(layer_f, k).detach().double().cpu().requires_grad_(True) for k in names]
    mags = [t.detach().abs().requires_grad_(True) for t in leaves]
    zn, zs = x.mean(1) @ leaves[0] + leaves[2], r @ leaves[1]
    mn, ms = x.abs().mean(1) @ mags[0] + mags[2], r.abs() @ mags[1]
    d, f = table.shape[1], zn.shape[1]
    far = (zn.abs() > ((4 * (d + 2) + count + 4) * U + 2.0 ** -8) * mn) & (zs.abs() > 4 * (d + 2) * U * ms)
    g = torch.randn(n, f, generator=torch.Generator().manual_seed(3)) * far
    (mn * (zn > 0) + ms * (zs > 0)).backward(g.double().abs())
    got = []
    for layer in (layer_r, layer_f):
        for k in names:
            getattr(layer, k).grad = None
        layer(ops.gather(table, self_ids), table, ids, count).backward(g.cuda().to(torch.bfloat16))
        got.append([getattr(layer, k).grad.double().cpu() for k in names])
    worst = 0.0
    for k, a, b, m in zip(names, got[0], got[1], mags):
        bound = 2 * (((1 + 2.0 ** -8) ** 3 - 1 + 4 * (n * count + 2 * d + f + 2) * U) * m.grad + 2.0 ** -8 * m.grad)
        worst = max(worst, float(((a - b).abs() / bound.clamp(min=1e-300)).max()))
        assert torch.all((a - b).abs() <= bound), k
    print("recompute vs fused backward: largest difference / bound %.3f" % worst)
    print("fused backward agrees within the bound")


def check_fp8(layer, table, self_ids, ids, count, n=4096):
    """layer 0 of the outermost hop over the Fp8Rows table of the same features: its first n destinations
    against float64 on the dequantised table.  With M the formula on absolute values: (4 (2 d + 2) + count + 4)
    2^-24 M (accumulation with the tests' margin, fold, mean) + 2^-8 M (the narrowing of the aggregate and of the
    root rows) + 2^-8 |result| (the bf16 output).  Quantisation adds no term: the reference reads the same x^."""
    t8 = ops.Fp8Rows.quantize(table.float())
    n = min(n, self_ids.numel())
    self_ids, ids = self_ids.reshape(-1)[:n], ids.reshape(-1)[:n * count]
    with torch.no_grad():
        out8 = ops.aggregate_dense("mean", t8, layer.neigh_w, ids, n, root_index=self_ids, root_weight=layer.self_w,
                                   bias=layer.bias, count=count).double().cpu()
        out16 = layer(ops.gather(table, self_ids), table, ids, count).double().cpu()
    t64 = t8.dequantize().double().cpu()
    x, r = t64[ids.cpu()].view(n, count, -1), t64[self_ids.cpu()]
    wn, ws, b = [p.detach().double().cpu() for p in (layer.neigh_w, layer.self_w, layer.bias)]
    ref = torch.relu(x.mean(1).to(torch.bfloat16).double() @ wn + b) + torch.relu(r.to(torch.bfloat16).double() @ ws)
    mag = x.abs().mean(1) @ wn.abs() + b.abs() + r.abs() @ ws.abs()
    bound = ((4 * (2 * table.shape[1] + 2) + count + 4) * U + 2.0 ** -8) * mag + 2.0 ** -8 * ref.abs()
    print("fp8 features vs float64 on the dequantised table: largest error / bound %.3f"
          % float(((out8 - ref).abs() / bound).max()))
    assert torch.all((out8 - ref).abs() <= bound)
    print("fp8 features vs bf16 features: relative error %.3e" % float((out8 - out16).norm() / out16.norm()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--composed", action="store_true", help="also run gather_segment_reduce + matmuls + relu + add")
    ap.add_argument("--fused-backward", action="store_true", help="also train through backward=\"fused\"")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--nodes", type=int, default=200000)
    ap.add_argument("--fp8-features", action="store_true", help="also run layer 0 of the outermost hop over an Fp8Rows table")
    a = ap.parse_args()
    fanouts = [25, 10]
    torch.manual_seed(0)
    G = euler_amd.Graph.synthetic(euler_amd.synth_params(11, a.nodes, 10 * a.nodes, weighted=True))
    G.set_seed(7)
    # rows 0 .. nodes are the nodes' features; row nodes + 1 is the default_node fill: zeros on both routes
    table = torch.randn((a.nodes + 2, a.dim), device="cuda").to(torch.bfloat16)
    table[a.nodes + 1] = 0
    routes = {"fused": False, **({"composed": True} if a.composed else {}), **({"fused-backward": False} if a.fused_backward else {})}
    models = {}
    for name, composed in routes.items():
        torch.manual_seed(1)        # the same weights on every route
        how = "fused" if name == "fused-backward" else "recompute"
        models[name] = [MeanSageLayer(a.dim, a.hidden, torch.bfloat16, composed, how),
                        MeanSageLayer(a.hidden, a.hidden, torch.bfloat16, composed, how)]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    roots = torch.randint(1, a.nodes + 1, (a.batch,), device="cuda", generator=gen)
    nodes = G.sample_fanout(roots, [[0], [0]], fanouts, a.nodes + 1, call_id=0)[0]
    for name, layers in models.items():
        params = [p for layer in layers for p in layer.parameters()]

        def step():
            for p in params:
                p.grad = None
            out = encode(layers, table, nodes, fanouts)
            out.float().square().mean().backward()
            return out

        step()                                                                         # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            out = step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        assert torch.isfinite(out.float()).all() and all(torch.isfinite(p.grad.float()).all() for p in params)
        print("%s: %.3f ms per step, peak %d bytes above the inputs" % (name, ms, torch.cuda.max_memory_allocated() - base))
        with torch.no_grad():
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            encode(layers, table, nodes, fanouts)
            torch.cuda.synchronize()
            print("%s: forward alone, peak %d bytes above the inputs" % (name, torch.cuda.max_memory_allocated() - base))
    if a.composed:
        check(models["fused"][0], models["composed"][0], table, nodes[1], nodes[2], fanouts[1])
    if a.fused_backward:
        check_backward(models["fused"][0], models["fused-backward"][0], table, nodes[1], nodes[2], fanouts[1])
    if a.fp8_features:
        check_fp8(models["fused"][0], table, nodes[1], nodes[2], fanouts[1])


if __name__ == "__main__":
    main()
