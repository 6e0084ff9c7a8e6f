#!/usr/bin/env python3
"""The GCN-normalised aggregation of a block: today's composition against gcn_norm + gcn_aggregate,
one GPU, one process, the same library.

Times, with device events and after warm-up, for fp32 and bf16 storage, forward and forward +
backward (gradient of x):
  - composed: exactly as examples/python/gcn_minibatch.py composes it - scatter_add of ones and
              ** -0.5 per side, a gather per side, an [E, 1] multiply, then the fused weighted
              reduce gather_scatter("add", x, src, dst, n, edge_weight=w)
  - fused:    ops.gcn_norm + ops.gcn_aggregate
  - norm:     ops.gcn_norm alone (the histogram and the table kernel)
  - reduce_norm / reduce_weighted (forward only): the two reduces alone - gcn_aggregate over precomputed
              tables, gather_scatter over a precomputed [E, 1] weight - and their `count` forms on the SAGE block
on the two shapes of DESIGN 4.10's table:
  - a SAGE block: 409 600 destinations x 10 neighbours (sorted destination keys), D = 128, 1 M sources
  - a GCN-style block: --gcn-nodes nodes, --gcn-edges random edges with UNSORTED destination keys
and prints ONE JSON line (also written to --out): the median milliseconds of every variant with the
min and max over the windows, fused / composed per row, and the bytes each algorithm must move
(indices, tables, rows and outputs; the sort of unsorted keys left out, as in 4.10).

Protocol: every variant is warmed up (--warmup calls), then timed in windows of --iters calls
between two events; the variants alternate window by window (--repeats rounds); the median window
is reported with min and max.

    python tools/gcn_norm_bench.py [--out profiles/gcn_norm.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from weighted_mp_bench import time_variants       # noqa: E402  (the protocol, shared)


def composed_weight(ops, dst, src, size):
    """norm_i * norm_j per edge, [E, 1], as gcn_minibatch.py builds it"""
    ones = torch.ones((dst.numel(), 1), device=dst.device)
    norm_i = ops.scatter_add(ones, dst, size[0]) ** -0.5
    norm_j = ops.scatter_add(ones, src, size[1]) ** -0.5
    return ops.gather(norm_i, dst) * ops.gather(norm_j, src)


def algo_bytes(e, d, n_dst, n_src, elt, backward):
    """bytes the algorithms must move in a forward pass (+ the gradient of x); elt = bytes per element
    of x and of the output; index and norm entries have 4"""
    block = e * d * elt
    reduce_w = e * (4 + 4 + 4) + block + n_dst * d * elt           # 4.10: indices, weight, rows, output
    # composed: per side scatter_add of ones (ones, keys; table out), ** -0.5 (in, out), gather (index, read,
    # write); then the [E, 1] multiply (two reads, one write)
    norm_a = 2 * (e * 8) + 3 * 4 * (n_dst + n_src) + 2 * (e * 12) + e * 12
    norm_b = e * 8 + 3 * 4 * (n_dst + n_src)                       # keys, counters written and read, tables
    reduce_n = e * (4 + 4 + 4) + n_dst * 4 + block + n_dst * d * elt   # the weight read is a table entry
    by = {"composed": norm_a + reduce_w, "fused": norm_b + reduce_n, "norm": norm_b}
    if backward:        # the same reduce with the roles swapped, over fp32 rows of the gradient
        back = e * 12 + e * d * 4 + n_src * d * 4
        by = {"composed": by["composed"] + back + e * 4 + (n_dst + 1) * d * 4, "fused": by["fused"] + back + n_src * 4}
    return by


def bench_shape(ops, name, x32, dst, src, size, count, a, res):
    e, d = src.numel(), x32.shape[1]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    g_out = torch.randn((size[0], d), generator=gen, device="cuda")
    ei = torch.stack([dst, src])
    shape = {"e": e, "d": d, "n_dst": size[0], "n_src": size[1],
             "sorted_keys": bool((dst[1:] >= dst[:-1]).all())}
    for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        x = x32.to(dt)
        xg = x.clone().requires_grad_(True)
        g = g_out.to(dt)

        def composed(t):
            return ops.gather_scatter("add", t, src, dst, size[0], edge_weight=composed_weight(ops, dst, src, size))

        def fused(t):
            return ops.gcn_aggregate(t, ei, size, ops.gcn_norm(ei, size))

        def with_backward(f):
            def run():
                xg.grad = None
                f(xg).backward(g)
            return run

        # the reduces alone, over precomputed tables / a precomputed [E, 1] weight (4.10's kernel)
        norm = ops.gcn_norm(ei, size)
        w = composed_weight(ops, dst, src, size)
        alone = {"reduce_norm": lambda: ops.gcn_aggregate(x, ei, size, norm),
                 "reduce_weighted": lambda: ops.gather_scatter("add", x, src, dst, size[0], edge_weight=w)}
        if count is not None:
            alone["reduce_norm_count"] = lambda: ops.gcn_aggregate(x, src, size, norm, count=count)
            alone["reduce_weighted_count"] = lambda: ops.gather_segment_reduce("add", x, src, size[0], count=count,
                                                                               edge_weight=w)
        rows = {"forward": dict({"composed": lambda: composed(x), "fused": lambda: fused(x),
                                 "norm": lambda: ops.gcn_norm(ei, size)}, **alone),
                "forward_backward": {"composed": with_backward(composed), "fused": with_backward(fused)}}
        out = {}
        for row, variants in rows.items():
            times = time_variants(variants, a.iters, a.repeats, a.warmup)
            by = algo_bytes(e, d, size[0], size[1], x.element_size(), row != "forward")
            for k, t in times.items():
                if k in by:
                    t["algo_bytes"] = by[k]
                    t["algo_GBps"] = round(by[k] / (t["ms"] * 1e-3) / 1e9, 1)
            c, f = times["composed"], times["fused"]
            out[row] = {"times": times, "fused_over_composed": round(f["ms"] / c["ms"], 4),
                        # the ratio's range over the windows; "faster by more than the spread" = max < 1
                        "fused_over_composed_min": round(f["min"] / c["max"], 4),
                        "fused_over_composed_max": round(f["max"] / c["min"], 4)}
        shape[tag] = out
        del x, xg, g
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
        sys.exit("gcn_norm_bench: needs a GPU (nothing here is measured on a CPU)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    res = {"tool": "gcn_norm_bench", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "repeats": a.repeats, "warmup": a.warmup, "shapes": {}}

    x = torch.randn((a.table_rows, a.dim), generator=gen, device="cuda")
    src = torch.randint(0, a.table_rows, (a.n_dst * a.count,), generator=gen, device="cuda", dtype=torch.int32)
    dst = torch.arange(a.n_dst, device="cuda", dtype=torch.int32).repeat_interleave(a.count)
    bench_shape(ops, "sage_block", x, dst, src, (a.n_dst, a.table_rows), a.count, a, res)
    del x, src, dst

    x = torch.randn((a.gcn_nodes, a.dim), generator=gen, device="cuda")
    src = torch.randint(0, a.gcn_nodes, (a.gcn_edges,), generator=gen, device="cuda", dtype=torch.int32)
    dst = torch.randint(0, a.gcn_nodes, (a.gcn_edges,), generator=gen, device="cuda", dtype=torch.int32)
    bench_shape(ops, "gcn_block_unsorted", x, dst, src, (a.gcn_nodes, a.gcn_nodes), None, a, res)

    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
