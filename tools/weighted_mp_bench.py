#!/usr/bin/env python3
"""The fused edge-weighted aggregation against the composition it replaces, one GPU, one process.

Times, with device events and after warm-up, for fp32 and bf16 storage
  - fused:    ops.gather_segment_reduce / ops.gather_scatter ("add", edge_weight=w): one pass
  - composed: ops.gather -> torch multiply by w[:, None] -> ops.scatter_add, the ops as they were
              before the weighted form existed (five passes over an [E, D] block)
  - edge_dot: ops.edge_dot of the destination rows and the gathered rows of the same edges
on two shapes:
  - a SAGE block: 16 384 x 25 destinations with `count` 10 neighbours each, D = 128, a table of
    1 M rows (sorted destinations: no grouping needed)
  - a GCN-style block: --gcn-nodes nodes, --gcn-edges random edges with UNSORTED destination keys
    (both forms then sort the keys; the bytes below leave the sort out)
and prints ONE JSON line (also written to --out): the median milliseconds of every variant with
the spread over the windows, and the bytes each algorithm must move - for the fused op the index,
weight and row reads plus the output write - with the rate they imply.

Protocol: every variant is warmed up, then timed in windows of --iters calls between two events;
the variants alternate window by window (--repeats rounds); the median window is reported with
min and max.

    python tools/weighted_mp_bench.py [--out profiles/weighted_mp.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def time_variants(variants, iters, repeats, warmup):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            got[k].append(window_ms(fn, iters))
    return {k: {"ms": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
            for k, v in got.items()}


def algo_bytes(e, d, n_out, elt):
    """bytes the algorithm must move; elt = bytes per table / message element (the output has elt too)"""
    block = e * d * elt
    return {"fused": e * (4 + 4) + block + n_out * d * elt,
            "composed": (e * 4 + 2 * block) + (block + e * 4 + block) + (block + e * 4 + n_out * d * elt),
            "edge_dot": e * 8 + 2 * block + e * 4}


def bench_shape(ops, name, table, gi, dst, n_out, count, a, res):
    e, d = gi.numel(), table.shape[1]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    w = torch.rand((e, 1), generator=gen, device="cuda") + 0.5
    g_out = torch.randn((n_out, d), generator=gen, device="cuda")
    shape = {"e": e, "d": d, "n_out": n_out, "table_rows": table.shape[0], "sorted_keys": count is not None}
    for tag, x in (("fp32", table), ("bf16", table.to(torch.bfloat16))):
        wx = w.to(x.dtype)
        if count is not None:
            fused = lambda: ops.gather_segment_reduce("add", x, gi, n_out, count=count, edge_weight=w)
        else:
            fused = lambda: ops.gather_scatter("add", x, gi, dst, n_out, edge_weight=w)
        v = {"fused": fused,
             "composed": lambda: ops.scatter_add(ops.gather(x, gi) * wx, dst, n_out),
             "edge_dot": lambda: ops.edge_dot(g_out, dst, x, gi, out_dtype=torch.float32)}
        times = time_variants(v, a.iters, a.repeats, a.warmup)
        by = algo_bytes(e, d, n_out, x.element_size())
        by["edge_dot"] = e * 8 + e * d * 4 + e * d * x.element_size() + e * 4      # (the dst rows are fp32)
        for k, t in times.items():
            t["algo_bytes"] = by[k]
            t["algo_GBps"] = round(by[k] / (t["ms"] * 1e-3) / 1e9, 1)
            t["fraction_of_8TBps"] = round(by[k] / (t["ms"] * 1e-3) / 8e12, 4)
        shape[tag] = {"times": times,
                      "fused_over_composed_time": round(times["fused"]["ms"] / times["composed"]["ms"], 4),
                      "fused_over_composed_bytes": round(by["fused"] / by["composed"], 4)}
        del x, wx
    res["shapes"][name] = shape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-dst", type=int, default=16384 * 25)
    ap.add_argument("--count", type=int, default=10)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--table-rows", type=int, default=1_000_000)
    ap.add_argument("--gcn-nodes", type=int, default=500_000)
    ap.add_argument("--gcn-edges", type=int, default=4_000_000)
    a = ap.parse_args()
    from euler_amd import ops
    if not torch.cuda.is_available():
        sys.exit("weighted_mp_bench: needs a GPU (nothing here is measured on a CPU)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    res = {"tool": "weighted_mp_bench", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "repeats": a.repeats, "warmup": a.warmup, "shapes": {}}

    table = torch.randn((a.table_rows, a.dim), generator=gen, device="cuda")
    gi = torch.randint(0, a.table_rows, (a.n_dst * a.count,), generator=gen, device="cuda", dtype=torch.int32)
    dst = torch.arange(a.n_dst, device="cuda", dtype=torch.int32).repeat_interleave(a.count)
    bench_shape(ops, "sage_block", table, gi, dst, a.n_dst, a.count, a, res)
    del table, gi, dst

    x = torch.randn((a.gcn_nodes, a.dim), generator=gen, device="cuda")
    src = torch.randint(0, a.gcn_nodes, (a.gcn_edges,), generator=gen, device="cuda", dtype=torch.int32)
    dst = torch.randint(0, a.gcn_nodes, (a.gcn_edges,), generator=gen, device="cuda", dtype=torch.int32)
    bench_shape(ops, "gcn_block_unsorted", x, src, dst, a.gcn_nodes, None, a, res)

    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
