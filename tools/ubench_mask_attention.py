#!/usr/bin/env python3
"""Times ops.mask_attention against the route a user had before it - Graph.adj_from_mask (two calls around a
host wait for nnz), int32 index arrays from the triple, and attention_aggregate("additive", indices=...) over
the edge list, timed whole - on one layerwise adjacency [1, n, m] of a given density.

Each window runs one route back to back for --seconds and ends in a device synchronise; the routes alternate
over --repeats windows, every shape warmed up first.  Prints one JSON line: per route the median / min / max ms
per call over the windows and the peak bytes a call allocates, and for the fused route the numerators it
evaluates (every source, candidate and head once per column tile of the head, zero words of a run of 16 sources
skipped) with the rate that makes, beside its matrix instructions and the bytes the shape needs.  --route fused
--calls N runs N calls and nothing else: the form to put under a kernel trace.  --backward times the BACKWARD pass
alone instead (one forward kept, its graph retained): the two kernels of backward="fused", the default
backward="recompute" in torch ops, and the composed route's own autograd.

    python tools/ubench_mask_attention.py [--n 16384] [--m 4096] [--density 0.01] [--heads 4] [--seconds 1]
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
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--form", default="renorm", choices=["none", "root", "renorm"])
    ap.add_argument("--route", default="both", choices=["both", "fused", "composed"])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="run this many calls of --route and exit")
    ap.add_argument("--backward", action="store_true", help="time the backward pass of fused / recompute / composed")
    a = ap.parse_args()
    torch.manual_seed(0)
    n, m, d, heads, dt = a.n, a.m, a.dim, a.heads, torch.bfloat16
    words = (m + 63) // 64
    bits = torch.rand((n, words * 64), device="cuda") < a.density
    bits[:, m:] = False
    mask = (bits.view(n, words, 64).to(torch.int64) << torch.arange(64, device="cuda")).sum(2)
    z = torch.randn((m, d), device="cuda").to(dt)
    s_src, s_nb, s_root = (torch.randn((r, heads), device="cuda") for r in (n, m, n))
    root = torch.randn((n, d), device="cuda").to(dt) if a.form != "none" else None
    s_root = s_root if a.form == "renorm" else None

    def fused(backward="recompute"):
        return ops.mask_attention(mask, z, s_src, s_nb, 1, n, m, heads=heads, root=root, s_root=s_root, backward=backward)

    def composed():
        ind, _val, _shape = Graph.adj_from_mask(mask, 1, n, m)
        src, cand = ind[:, 1].to(torch.int32), ind[:, 2].to(torch.int32)
        if a.form != "renorm":
            agg = ops.attention_aggregate("additive", s_src, s_nb, cand, n, v=z, heads=heads, indices=src)
            return agg if root is None else root + agg
        # renorm: the source's own row is one more candidate (the eye column)
        own = torch.arange(n, device="cuda", dtype=torch.int32)
        return ops.attention_aggregate("additive", s_src, torch.cat([s_nb, s_root]), torch.cat([cand, m + own]), n,
                                       v=torch.cat([z, root]), heads=heads, indices=torch.cat([src, own]))

    routes = {"fused": fused, "composed": composed}
    if a.backward:
        leaves = [t.requires_grad_(True) for t in (z, s_src, s_nb, root, s_root) if t is not None]
        outs = {"fused": fused("fused"), "recompute": fused(), "composed": composed()}
        grad = torch.randn((n, d), device="cuda").to(dt)
        routes = {k: (lambda o=o: torch.autograd.grad(o, leaves, grad, retain_graph=True)) for k, o in outs.items()}
    elif a.route != "both":
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
    out = {"shape": {"n": n, "m": m, "d": d, "heads": heads, "density": a.density, "nnz": int(bits.sum()), "form": a.form,
                     "dtype": "bf16"},
           "calls_per_window": calls, "windows": a.repeats,
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()},
           "peak_bytes_per_call": peak}
    if "fused" in ms and not a.backward:
        # pass 2 evaluates 64 numerators per live word and source, for every head and column tile of the head;
        # one v_mfma_f32_16x16x32 per run of 16 sources, chunk of 32 candidates and 16 columns
        dh = d // heads
        nt = 1
        while nt < 4 and 16 * nt < dh:
            nt *= 2
        col_tiles = (dh + 16 * nt - 1) // (16 * nt)
        runs = (n + 15) // 16
        pad = torch.zeros((runs * 16 - n, words), dtype=torch.int64, device="cuda")
        live_words = int((torch.cat([mask, pad]).view(runs, 16, words) != 0).any(1).sum())
        p_evals = live_words * 16 * 64 * heads * col_tiles
        bytes_needed = n * words * 8 + m * d * 2 + (n + m + (n if s_root is not None else 0)) * heads * 4 \
            + (n * d * 2 if root is not None else 0) + n * d * 2
        sec = out["ms"]["fused"]["median"] * 1e-3
        out["fused"] = {"p_evaluations": p_evals, "p_per_second": p_evals / sec, "mfma": 2 * live_words * heads * col_tiles * nt,
                        "bytes_needed": bytes_needed, "hbm_floor_ms": bytes_needed / HBM_BYTES_PER_S * 1e3}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
