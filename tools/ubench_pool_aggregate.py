#!/usr/bin/env python3
"""Times ops.pool_aggregate against the composed route (gather + addmm + relu + scatter_max / _mean)
on one aggregation of a sampled block - hop 2 of fanout [25, 10] by default - and relates the fused
time to the bytes and FLOP the shape needs.

Each window runs one route back to back for --seconds and ends in a device synchronise; the routes
alternate over --repeats windows, every shape warmed up first.  Prints one JSON line: per route the
median / min / max ms per call over the windows, and for the fused route the HBM and MFMA floors.
--route fused --calls N runs N calls and nothing else: the form to put under a kernel trace.
--backward times forward + backward instead, on three routes - the fused forward with backward="recompute", with
backward="fused" (DESIGN 4.37), and torch autograd of the composed route - for the weight and bias gradients, with
--table-grad for the table's too, and adds each route's peak bytes above the inputs.

    python tools/ubench_pool_aggregate.py [--roots 131072] [--op max] [--seconds 2] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from euler_amd import ops                          # noqa: E402

HBM_BYTES_PER_S = 8.0e12        # MI355X peak
BF16_FLOP_PER_S = 2.5e15        # dense bf16 MFMA peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=131072)
    ap.add_argument("--fanout", type=int, nargs=2, default=[25, 10])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--table-rows", type=int, default=1 << 20)
    ap.add_argument("--op", default="max", choices=["max", "mean", "add"])
    ap.add_argument("--route", default="both", choices=["both", "fused", "composed", "recompute", "autograd"])
    ap.add_argument("--backward", action="store_true", help="time forward + backward: recompute, fused, autograd")
    ap.add_argument("--table-grad", action="store_true", help="--backward: the table wants a gradient too")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="run this many calls of --route and exit")
    a = ap.parse_args()
    torch.manual_seed(0)
    n_dst, count = a.roots * a.fanout[0], a.fanout[1]
    e, dt = n_dst * count, torch.bfloat16
    table = torch.randn((a.table_rows, a.dim), device="cuda").to(dt)
    w = (torch.randn((a.dim, a.hidden), device="cuda") / a.dim ** 0.5).to(dt)
    b = torch.randn(a.hidden, device="cuda")
    ids = torch.randint(0, a.table_rows, (e,), device="cuda")
    dst = torch.arange(n_dst, device="cuda", dtype=torch.int32).repeat_interleave(count)

    def fused():
        return ops.pool_aggregate(a.op, table, w, ids, n_dst, bias=b, count=count)

    def composed():
        h = torch.relu(torch.addmm(b.to(dt), ops.gather(table, ids), w))
        return (ops.scatter_max if a.op == "max" else ops.scatter_mean if a.op == "mean" else ops.scatter_add)(h, dst, n_dst)

    routes = {"fused": fused, "composed": composed}
    if a.backward:
        g_out = torch.randn((n_dst, a.hidden), device="cuda").to(dt)
        table.requires_grad_(a.table_grad)
        w.requires_grad_(True)
        b.requires_grad_(True)

        def both_ways(forward):
            def fn():
                table.grad = w.grad = b.grad = None
                forward().backward(g_out)
            return fn
        routes = {"recompute": both_ways(fused), "autograd": both_ways(composed),
                  "fused": both_ways(lambda: ops.pool_aggregate(a.op, table, w, ids, n_dst, bias=b, count=count, backward="fused"))}
    if a.route != "both":
        routes = {a.route: routes[a.route]}
    if a.calls:
        for _ in range(a.calls):
            routes[a.route]()
        torch.cuda.synchronize()
        return
    calls, peak = {}, {}
    for name, fn in routes.items():             # warm up, and size a window from one timed call
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        calls[name] = max(3, int(a.seconds / (time.perf_counter() - t0)))
        peak[name] = torch.cuda.max_memory_allocated() - base
    ms = {name: [] for name in routes}
    for _ in range(a.repeats):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            for _ in range(calls[name]):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / calls[name])
    bytes_needed = e * (2 * a.dim + 8) + n_dst * a.hidden * 2 + a.dim * a.hidden * 2      # rows + ids in, result out, W
    flop = 2 * e * a.dim * a.hidden
    out = {"shape": {"e": e, "n_dst": n_dst, "d": a.dim, "F": a.hidden, "op": a.op, "dtype": "bf16"},
           "calls_per_window": calls, "windows": a.repeats, "backward": a.backward, "table_grad": a.table_grad,
           "peak_bytes": peak,
           "ms": {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in ms.items()},
           "bytes_needed": bytes_needed, "flop": flop,
           "hbm_floor_ms": bytes_needed / HBM_BYTES_PER_S * 1e3, "mfma_floor_ms": flop / BF16_FLOP_PER_S * 1e3}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
