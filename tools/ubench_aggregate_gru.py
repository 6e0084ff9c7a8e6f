#!/usr/bin/env python3
"""Times ops.aggregate_gru against the composed route (gather_segment_reduce + cat + two addmm + the
elementwise steps of the TF GRU cell, all from this library and torch, in bf16) on one gated-graph step
over a sampled block - hop 2 of fanout [25, 10] by default - and relates the fused time to the bytes the
shape needs.

Each window runs one route back to back for --seconds and ends in a device synchronise; the routes
alternate over --repeats windows, every shape warmed up first.  Prints one JSON line: per route the
median / min / max ms per call over the windows and the peak bytes a call allocates, and for the fused
route the HBM floor.  --route fused --calls N runs N calls and nothing else: the form to put under a
kernel trace.

    python tools/ubench_aggregate_gru.py [--roots 131072] [--op add] [--seconds 2] [--repeats 5]
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
    ap.add_argument("--units", type=int, default=128)
    ap.add_argument("--table-rows", type=int, default=1 << 20)
    ap.add_argument("--op", default="add", choices=["mean", "add"])
    ap.add_argument("--route", default="both", choices=["both", "fused", "composed"])
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="run this many calls of --route and exit")
    a = ap.parse_args()
    torch.manual_seed(0)
    n_dst, count, d, u = a.roots * a.fanout[0], a.fanout[1], a.dim, a.units
    e, dt = n_dst * count, torch.bfloat16
    table = (torch.randn((a.table_rows, d), device="cuda") / count ** 0.5).to(dt)
    state = torch.randn((n_dst, u), device="cuda").to(dt)
    wg = (torch.randn((d + u, 2 * u), device="cuda") / (d + u) ** 0.5).to(dt)
    wc = (torch.randn((d + u, u), device="cuda") / (d + u) ** 0.5).to(dt)
    bg, bc = torch.ones(2 * u, device="cuda"), torch.zeros(u, device="cuda")
    bg_dt, bc_dt = bg.to(dt), bc.to(dt)     # what a composed layer would keep: no conversion inside the timed call
    ids = torch.randint(0, a.table_rows, (e,), device="cuda")

    def fused():
        return ops.aggregate_gru(a.op, table, ids, n_dst, state, wg, wc, bg, bc, count=count)

    def composed():
        m = ops.gather_segment_reduce(a.op, table, ids, n_dst, count=count)
        zg = torch.addmm(bg_dt, torch.cat([m, state], 1), wg)
        r, z = torch.sigmoid(zg[:, :u]), torch.sigmoid(zg[:, u:])
        c = torch.tanh(torch.addmm(bc_dt, torch.cat([m, r * state], 1), wc))
        return z * state + (1 - z) * c

    routes = {"fused": fused, "composed": composed}
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
    # rows + ids in, state in, result out, both W
    bytes_needed = e * (2 * d + 8) + n_dst * u * 2 + n_dst * u * 2 + 3 * u * (d + u) * 2
    out = {"shape": {"e": e, "n_dst": n_dst, "d": d, "U": u, "op": a.op, "dtype": "bf16"},
           "calls_per_window": calls, "windows": a.repeats,
           "ms": {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in ms.items()},
           "peak_bytes_per_call": peak, "bytes_needed": bytes_needed,
           "hbm_floor_ms": bytes_needed / HBM_BYTES_PER_S * 1e3}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
