#!/usr/bin/env python3
"""Times ops.mask_aggregate against the route a user had before it - Graph.adj_from_mask (two calls around
a host wait for nnz) followed by gather_scatter over the resulting edge list - on one layerwise adjacency
[1, n, m] of a given density, and relates the fused time to the bytes the shape needs.

Each window runs one route back to back for --seconds and ends in a device synchronise; the routes
alternate over --repeats windows, every shape warmed up first.  Prints one JSON line: per route the
median / min / max ms per call over the windows and the peak bytes a call allocates, the fused route's HBM
floor (mask + one read of x + root + output), and the matrix instructions the fused kernel issues with and
without its zero-word skip, counted from the mask.  --route fused --calls N runs N calls and nothing else:
the form to put under a kernel trace.

    python tools/ubench_mask_aggregate.py [--n 16384] [--m 4096] [--density 0.01] [--op mean] [--seconds 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from euler_amd import Graph, ops                   # noqa: E402

HBM_BYTES_PER_S = 8.0e12        # MI355X peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--op", default="mean", choices=["add", "mean", "gcn", "gcn_renorm"])
    ap.add_argument("--route", default="both", choices=["both", "fused", "composed"])
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="run this many calls of --route and exit")
    a = ap.parse_args()
    torch.manual_seed(0)
    n, m, d, dt = a.n, a.m, a.dim, torch.bfloat16
    words = (m + 63) // 64
    bits = torch.rand((n, words * 64), device="cuda") < a.density
    bits[:, m:] = False
    mask = (bits.view(n, words, 64).to(torch.int64) << torch.arange(64, device="cuda")).sum(2)
    x = torch.randn((m, d), device="cuda").to(dt)
    root = torch.randn((n, d), device="cuda").to(dt) if a.op.startswith("gcn") else None

    def fused():
        return ops.mask_aggregate(a.op, mask, x, 1, n, m, root=root)

    def composed():
        ind, _val, _shape = Graph.adj_from_mask(mask, 1, n, m)
        src, cand = ind[:, 1], ind[:, 2]
        if a.op == "add":
            return ops.gather_scatter("add", x, cand, src, n)
        mean = ops.gather_scatter("mean", x, cand, src, n)
        if a.op == "mean":
            return mean
        if a.op == "gcn":
            return root + mean
        deg = torch.bincount(src, minlength=n).reshape(-1, 1)
        return ((root.float() + ops.gather_scatter("add", x, cand, src, n, out_dtype=torch.float32)) / (1 + deg)).to(dt)

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
    # one v_mfma_f32_16x16x32 per run of 16 sources, chunk of 32 candidates and 16 columns; a run skips a
    # word (two chunks) that is zero for all its sources
    runs = (n + 15) // 16
    pad = torch.zeros((runs * 16 - n, words), dtype=torch.int64, device="cuda")
    live_words = int((torch.cat([mask, pad]).view(runs, 16, words) != 0).any(1).sum())
    nt = 1                                      # (the fragments of the plan: a column tile rides whole)
    while nt < 8 and 16 * nt < d:
        nt *= 2
    frags = (d + 16 * nt - 1) // (16 * nt) * nt
    bytes_needed = n * words * 8 + m * d * 2 + (n * d * 2 if root is not None else 0) + n * d * 2
    out = {"shape": {"n": n, "m": m, "d": d, "density": a.density, "nnz": int(bits.sum()), "op": a.op, "dtype": "bf16"},
           "calls_per_window": calls, "windows": a.repeats,
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()},
           "peak_bytes_per_call": peak, "bytes_needed": bytes_needed,
           "hbm_floor_ms": bytes_needed / HBM_BYTES_PER_S * 1e3,
           "mfma": {"with_skip": 2 * live_words * frags, "without_skip": 2 * runs * words * frags}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
