#!/usr/bin/env python3
"""Times ops.aggregate_dense against the composed route (gather_segment_reduce + addmm + the root matmul
+ relu + add, all from this library and torch) on one mean-aggregator layer over a sampled block - hop 2
of fanout [25, 10] by default - and relates the fused time to the bytes the shape needs.

Each window runs one route back to back for --seconds and ends in a device synchronise; the routes
alternate over --repeats windows, every shape warmed up first.  Prints one JSON line: per route the
median / min / max ms per call over the windows and the peak bytes a call allocates, and for the fused
route the HBM floor.  --route fused --calls N runs N calls and nothing else: the form to put under a
kernel trace.

--table fp8 times layer 0 over an Fp8Rows table of the same values instead, three routes in one
call: fused_fp8 (aggregate_dense on the Fp8Rows, the roots by root_index), fused_bf16 (the route above,
unchanged, on the bf16 table) and composed_fp8 (gather_segment_reduce on the Fp8Rows with a bf16 result +
ops.gather for the roots + the matmuls); the floor is then that of fused_fp8.  --route fused selects fused_fp8.

--backward times forward + backward per call instead, gradients to the table, both weights, the
bias and the roots, three routes in one call: recompute (the fused forward, backward="recompute"), fused (the
fused forward, backward="fused": euler_gpu_aggregate_dense_backward) and composed (torch autograd through the
composed route).  --route recompute | fused | composed with --calls N is the form for a kernel trace.

    python tools/ubench_aggregate_dense.py [--roots 131072] [--op mean] [--seconds 2] [--repeats 5] [--table fp8]
                                           [--backward]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=131072)
    ap.add_argument("--fanout", type=int, nargs=2, default=[25, 10])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--table-rows", type=int, default=1 << 20)
    ap.add_argument("--op", default="mean", choices=["mean", "add"])
    ap.add_argument("--route", default="both", choices=["both", "fused", "composed", "recompute"])
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="run this many calls of --route and exit")
    ap.add_argument("--table", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--backward", action="store_true", help="time forward + backward: recompute, fused, composed")
    a = ap.parse_args()
    torch.manual_seed(0)
    n_dst, count = a.roots * a.fanout[0], a.fanout[1]
    e, dt = n_dst * count, torch.bfloat16
    table = torch.randn((a.table_rows, a.dim), device="cuda").to(dt)
    w, ws = [(torch.randn((a.dim, a.hidden), device="cuda") / a.dim ** 0.5).to(dt) for _ in range(2)]
    b = torch.randn(a.hidden, device="cuda")
    b_dt = b.to(dt)             # what a composed layer would keep: no conversion inside the timed call
    ids = torch.randint(0, a.table_rows, (e,), device="cuda")
    root = torch.randn((n_dst, a.dim), device="cuda").to(dt)

    def fused():
        return ops.aggregate_dense(a.op, table, w, ids, n_dst, root=root, root_weight=ws, bias=b, count=count)

    def composed():
        agg = ops.gather_segment_reduce(a.op, table, ids, n_dst, count=count)
        return torch.relu(torch.addmm(b_dt, agg, w)) + torch.relu(root @ ws)

    routes = {"fused": fused, "composed": composed}
    if a.table == "fp8":
        t8 = ops.Fp8Rows.quantize(table)
        root_ids = torch.randint(0, a.table_rows, (n_dst,), device="cuda")

        def fused_fp8():
            return ops.aggregate_dense(a.op, t8, w, ids, n_dst, root_index=root_ids, root_weight=ws, bias=b, count=count)

        def composed_fp8():
            agg = ops.gather_segment_reduce(a.op, t8, ids, n_dst, count=count, out_dtype=dt)
            return torch.relu(torch.addmm(b_dt, agg, w)) + torch.relu(ops.gather(t8, root_ids, out_dtype=dt) @ ws)

        routes = {"fused_fp8": fused_fp8, "fused_bf16": fused, "composed_fp8": composed_fp8}
        a.route = {"fused": "fused_fp8", "composed": "composed_fp8"}.get(a.route, a.route)
    if a.backward:
        leaves = [t.requires_grad_(True) for t in (table, w, ws, b, root)]
        g_out = torch.randn((n_dst, a.hidden), device="cuda").to(dt)

        def trained(forward):
            def call():
                for t in leaves:
                    t.grad = None
                forward().backward(g_out)
            return call

        def composed_fwd():             # (the bias stays an fp32 leaf: its conversion is part of the graph)
            agg = ops.gather_segment_reduce(a.op, table, ids, n_dst, count=count)
            return torch.relu(torch.addmm(b.to(dt), agg, w)) + torch.relu(root @ ws)

        fwd = lambda how: lambda: ops.aggregate_dense(a.op, table, w, ids, n_dst, root=root, root_weight=ws, bias=b,
                                                      count=count, backward=how)
        routes = {"recompute": trained(fwd("recompute")), "fused": trained(fwd("fused")), "composed": trained(composed_fwd)}
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
        held = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        calls[name] = max(3, int(a.seconds / (time.perf_counter() - t0)))
        peak[name] = torch.cuda.max_memory_allocated() - held
    ms = {name: [] for name in routes}
    for _ in range(a.repeats):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            for _ in range(calls[name]):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / calls[name])
    # rows + ids in, root in, result out, both W
    bytes_needed = e * (2 * a.dim + 8) + n_dst * a.dim * 2 + n_dst * a.hidden * 2 + 2 * a.dim * a.hidden * 2
    if a.table == "fp8":        # one byte per code, the roots by id from the same table, the column scales
        bytes_needed = e * (a.dim + 8) + n_dst * (a.dim + 8) + n_dst * a.hidden * 2 + 2 * a.dim * a.hidden * 2 + 4 * a.dim
    out = {"shape": {"e": e, "n_dst": n_dst, "d": a.dim, "F": a.hidden, "op": a.op, "dtype": "bf16", "combine": "add",
                     **({"table": "fp8"} if a.table == "fp8" else {}), **({"backward": True} if a.backward else {})},
           "calls_per_window": calls, "windows": a.repeats,
           "ms": {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in ms.items()},
           "peak_bytes_per_call": peak, "bytes_needed": bytes_needed,
           "hbm_floor_ms": bytes_needed / HBM_BYTES_PER_S * 1e3}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
