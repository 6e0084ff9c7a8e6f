#!/usr/bin/env python3
"""The reference's GatedConv (tf_euler/python/convolution/gated_graph_conv.py:26-57) over a sampled block on
one MI355X: two processing steps, a stack of two TF GRU cells.

Per processing step i the layer projects the source rows (fc[i], no bias), sums a destination's projected
neighbours, and runs the stack of cells over that sum as a length-1 sequence - every cell seeded with the
destination's own row h, the second cell fed the first one's output; the stack's output is the next step's h.
The cells' weights are shared by the steps.  Here the neighbour ids come from Graph.sample_fanout, and each
cell is ONE kernel, ops.aggregate_gru: the first with the neighbour sum fused in, the second with no gather
array and count=1 over the first one's output.  --composed runs ops.gather_segment_reduce + cat + two matmuls
+ the elementwise steps beside it.  Every cell call of every route is asserted against float64 on the values
that call was given, within the bound of tests/test_aggregate_gru_gpu.py, and the forward's ms and peak device
bytes are printed per route.

    python examples/python/gated_graph_minibatch.py [--steps 5] [--composed] [--batch 4096]
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

U24, UNIT, ACT = 2.0 ** -24, 2.0 ** -8, 4 * 2.0 ** -24      # fp32 and bf16 units; kGruActUlps of mp_gru.h
DT = torch.bfloat16


class GatedConv(torch.nn.Module):
    def __init__(self, dim, processing_steps, cells, composed):
        super().__init__()
        self.composed = composed
        mk = lambda *s: torch.nn.Parameter((torch.randn(*s, device="cuda") / s[0] ** 0.5).to(DT))
        self.fc = torch.nn.ParameterList([mk(dim, dim) for _ in range(processing_steps)])
        self.gate_w = torch.nn.ParameterList([mk(2 * dim, 2 * dim) for _ in range(cells)])
        self.cand_w = torch.nn.ParameterList([mk(2 * dim, dim) for _ in range(cells)])
        # GRUCell's initialisers: 1.0 for the gates, 0 for the candidate
        self.gate_b = torch.nn.ParameterList([torch.nn.Parameter(torch.ones(2 * dim, device="cuda")) for _ in range(cells)])
        self.cand_b = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(dim, device="cuda")) for _ in range(cells)])

    def cell(self, k, rows, ids, count, h):
        """cell k over the sums of `count` rows per destination (ids None: row p is position p), state h"""
        n = h.shape[0]
        wg, wc, bg, bc = self.gate_w[k], self.cand_w[k], self.gate_b[k], self.cand_b[k]
        if not self.composed:
            return ops.aggregate_gru("add", rows, ids, n, h, wg, wc, bg, bc, count=count)
        m = rows if ids is None and count == 1 else ops.gather_segment_reduce(
            "add", rows, torch.arange(n * count, device="cuda", dtype=torch.int32) if ids is None else ids.reshape(-1),
            n, count=count)
        u_dim = h.shape[1]
        zg = (torch.cat([m, h], 1) @ wg).float() + bg                     # bf16 products, the rest in fp32
        r, u = torch.sigmoid(zg[:, :u_dim]), torch.sigmoid(zg[:, u_dim:])
        zc = (torch.cat([m, (r * h.float()).to(DT)], 1) @ wc).float() + bc
        return (u * h.float() + (1 - u) * torch.tanh(zc)).to(DT)

    def forward(self, x_dst, table, ids, count, calls=None):
        """[n_dst, dim]; calls: a list that receives (rows, ids, count, h, k, out) of every cell call"""
        h = x_dst
        for fc in self.fc:
            rows, gi, cnt = table @ fc, ids, count
            for k in range(len(self.gate_w)):
                out = self.cell(k, rows, gi, cnt, h)
                if calls is not None:
                    calls.append((rows, gi, cnt, h, k, out))
                rows, gi, cnt = out, None, 1
            h = out
        return h


def check(layer, calls, n=2048):
    """every recorded cell call, its first n destinations, against float64 on the CPU within the bound the tests
    derive: accumulation (K + 2) 2^-24 sum |a||w| with the 4x margin, the fold's (count + 1) 2^-24 sum |x| and one
    bf16 unit on m, r's error times |h| and one unit on r * h, sigmoid's slope 1/4 and tanh's 1, the blend, the
    bf16 output.  The composed route also rounds both matmul results to bf16: one unit more on each pre-activation.
    -> the largest error / bound ratio"""
    worst = 0.0
    f64 = lambda t: t.detach().double().cpu()
    for rows, ids, count, h, k, out in calls:
        n = min(n, h.shape[0])
        gi = torch.arange(n * count) if ids is None else ids.reshape(-1)[:n * count].cpu().long()
        x = f64(rows)[gi].view(n, count, -1)
        h, got = f64(h[:n]), f64(out[:n])
        wg, wc, bg, bc = [f64(p[k]) for p in (layer.gate_w, layer.cand_w, layer.gate_b, layer.cand_b)]
        d, u_dim = x.shape[2], h.shape[1]
        m = x.sum(1).to(DT).double()
        zg = torch.cat([m, h], 1) @ wg + bg
        r, u = torch.sigmoid(zg[:, :u_dim]), torch.sigmoid(zg[:, u_dim:])
        rh = (r * h).to(DT).double()
        c = torch.tanh(torch.cat([m, rh], 1) @ wc + bc)
        ref = u * h + (1 - u) * c
        dm = (count + 1) * U24 * x.abs().sum(1) + UNIT * m.abs()
        acc = 4 * (d + u_dim + 2) * U24 + (UNIT if layer.composed else 0.0)
        e_g = acc * (torch.cat([m.abs(), h.abs()], 1) @ wg.abs() + bg.abs()) + dm @ wg[:d].abs()
        dr, du = e_g[:, :u_dim] / 4 + ACT, e_g[:, u_dim:] / 4 + ACT
        drh = dr * h.abs() + (U24 + UNIT) * rh.abs()
        e_c = acc * (torch.cat([m.abs(), rh.abs()], 1) @ wc.abs() + bc.abs()) + dm @ wc[:d].abs() + drh @ wc[d:].abs()
        bound = (h - c).abs() * du + (1 - u) * (e_c + ACT) + (4 * U24 + UNIT) * (h.abs() + c.abs())
        assert torch.all((got - ref).abs() <= bound), "cell %d of a step is outside the bound" % k
        worst = max(worst, float(((got - ref).abs() / bound).max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed forward passes")
    ap.add_argument("--composed", action="store_true", help="also run gather_segment_reduce + matmuls + elementwise")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--fanout", type=int, default=25)
    ap.add_argument("--nodes", type=int, default=200000)
    a = ap.parse_args()
    torch.manual_seed(0)
    G = euler_amd.Graph.synthetic(euler_amd.synth_params(11, a.nodes, 10 * a.nodes, weighted=True))
    G.set_seed(7)
    # rows 0 .. nodes are the nodes' features; row nodes + 1 is the default_node fill: zeros on both routes
    table = (torch.randn((a.nodes + 2, a.dim), device="cuda") / a.fanout ** 0.5).to(DT)
    table[a.nodes + 1] = 0
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    roots = torch.randint(1, a.nodes + 1, (a.batch,), device="cuda", generator=gen)
    nodes = G.sample_fanout(roots, [[0]], [a.fanout], a.nodes + 1, call_id=0)[0]
    x_dst, ids = ops.gather(table, nodes[0].reshape(-1)), nodes[1].reshape(-1)
    for name, composed in ({"fused": False, "composed": True} if a.composed else {"fused": False}).items():
        torch.manual_seed(1)        # the same weights on both routes
        layer = GatedConv(a.dim, 2, 2, composed)
        with torch.no_grad():
            calls = []
            layer(x_dst, table, ids, a.fanout, calls)                                  # warm-up, and the check
            print("%s vs float64 over %d cell calls: largest error / bound %.3f" % (name, len(calls), check(layer, calls)))
            del calls
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                out = layer(x_dst, table, ids, a.fanout)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
            print("%s: forward %.3f ms, peak %d bytes above the inputs" % (name, ms, torch.cuda.max_memory_allocated() - base))
        # one training step: the backward is the chunked fp32 recomputation on the fused route
        layer(x_dst, table, ids, a.fanout).float().square().mean().backward()
        assert torch.isfinite(out.float()).all() and all(torch.isfinite(p.grad.float()).all() for p in layer.parameters())
    print("every cell call of every route is within the bound")


if __name__ == "__main__":
    main()
