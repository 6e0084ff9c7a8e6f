#!/usr/bin/env python3
"""fp32 vs bf16 storage on the shapes of the hetero leg and the SAGE example, one GPU.

Times, with device events, for each shape
  - block aggregation (ops.gather_segment_reduce "mean", int64 ids, `count` per destination):
    count = 10 and 25, D = 128 and 256, n_dst = 256 000, a table of --table-rows rows
  - ops.scatter_mean with E = 2.56 M (10 sorted updates per destination), D = 128
  - Graph.get_dense_feature of 281 600 rows of a uniform 128-d table
the variants fp32, bf16 -> fp32 and bf16 -> bf16, and prints ONE JSON line (also written to
--out): per shape the median milliseconds of every variant, their ratios to fp32 and the byte
ratios the algorithm needs (computed from the shapes).

Protocol: every variant of a shape is warmed up, then timed in windows of --iters calls
between two events; the variants alternate window by window (--repeats rounds) and the
median window is reported with the spread (min, max).

--root DIR imports euler_amd from another checkout of this repository: a checkout that has no
16-bit ops (an earlier commit) yields the fp32 column alone, the number this commit's fp32
column must match.

    python tools/bench_half_mp.py [--out profiles/half_mp.json] [--root DIR]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def time_variants(variants, iters, repeats, warmup):
    """variants: {name: fn}; alternating windows; {name: {ms, min, max}}"""
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


def with_ratios(times, bytes_per_variant):
    out = {"times": times, "algo_bytes": bytes_per_variant}
    if "fp32" in times and len(times) > 1:
        out["time_ratio_to_fp32"] = {k: round(v["ms"] / times["fp32"]["ms"], 4) for k, v in times.items()}
        out["byte_ratio_to_fp32"] = {k: round(b / bytes_per_variant["fp32"], 4)
                                     for k, b in bytes_per_variant.items() if k in times}
    for k, v in times.items():
        v["algo_GBps"] = round(bytes_per_variant[k] / (v["ms"] * 1e-3) / 1e9, 1)
    return out


def feature_graph(euler_amd, n, dim, seed):
    rng = np.random.default_rng(seed)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    ones_f = np.ones(n, np.float32)
    val = rng.standard_normal(n * dim, dtype=np.float32)
    feats = (1, np.arange(n + 1, dtype=np.int64) * dim, np.full(n, dim, np.int32), val)
    return euler_amd.Graph.from_csr(ids, np.arange(n + 1, dtype=np.int64), np.ones(n, np.int32),
                                    ids.copy(), ones_f, ones_f.copy(), 1, features=feats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--root", default="")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-dst", type=int, default=256_000)
    ap.add_argument("--table-rows", type=int, default=1_000_000)
    ap.add_argument("--feature-nodes", type=int, default=500_000)
    ap.add_argument("--feature-rows", type=int, default=281_600)
    a = ap.parse_args()
    root = os.path.abspath(a.root) if a.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import euler_amd
    from euler_amd import _lib, ops
    if not torch.cuda.is_available():
        sys.exit("bench_half_mp: needs a GPU (nothing here is measured on a CPU)")
    half = hasattr(_lib, "BF16")
    bf16, f32 = torch.bfloat16, torch.float32
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    res = {"tool": "bench_half_mp", "device": torch.cuda.get_device_name(0), "package_root": os.path.basename(root),
           "has_16_bit_ops": half, "iters": a.iters, "repeats": a.repeats, "shapes": {}}
    n_dst = a.n_dst

    for d in (128, 256):
        table = torch.randn((a.table_rows, d), generator=gen, device="cuda")
        table16 = table.to(bf16)
        for count in (10, 25):
            ids = torch.randint(0, a.table_rows, (n_dst * count,), generator=gen, device="cuda", dtype=torch.int64)
            v = {"fp32": lambda: ops.gather_segment_reduce("mean", table, ids, n_dst, count=count)}
            if half:
                v["bf16_to_fp32"] = lambda: ops.gather_segment_reduce("mean", table16, ids, n_dst, count=count,
                                                                      out_dtype=f32)
                v["bf16_to_bf16"] = lambda: ops.gather_segment_reduce("mean", table16, ids, n_dst, count=count)
            idb = 8 * count                                       # the ids of a destination
            by = {"fp32": n_dst * (count * d * 4 + d * 4 + idb),
                  "bf16_to_fp32": n_dst * (count * d * 2 + d * 4 + idb),
                  "bf16_to_bf16": n_dst * (count * d * 2 + d * 2 + idb)}
            res["shapes"]["block_mean_count%d_d%d" % (count, d)] = with_ratios(
                time_variants(v, a.iters, a.repeats, a.warmup), by)
        del table, table16

    d, count = 128, 10
    e = n_dst * count
    upd = torch.randn((e, d), generator=gen, device="cuda")
    upd16 = upd.to(bf16)
    keys = torch.arange(n_dst, device="cuda", dtype=torch.int32).repeat_interleave(count)
    v = {"fp32": lambda: ops.scatter_mean(upd, keys, n_dst)}
    if half:
        v["bf16_to_fp32"] = lambda: ops.scatter_mean(upd16, keys, n_dst, out_dtype=f32)
        v["bf16_to_bf16"] = lambda: ops.scatter_mean(upd16, keys, n_dst)
    by = {"fp32": e * d * 4 + n_dst * d * 4 + e * 4, "bf16_to_fp32": e * d * 2 + n_dst * d * 4 + e * 4,
          "bf16_to_bf16": e * d * 2 + n_dst * d * 2 + e * 4}
    res["shapes"]["scatter_mean_e%d_d%d" % (e, d)] = with_ratios(time_variants(v, a.iters, a.repeats, a.warmup), by)
    del upd, upd16

    dim, rows = 128, a.feature_rows
    G = feature_graph(euler_amd, a.feature_nodes, dim, 11)
    q = torch.randint(1, a.feature_nodes + 1, (rows,), generator=gen, device="cuda", dtype=torch.int64)
    v = {"fp32": lambda: G.get_dense_feature(q, [0], [dim])}
    if half:
        G16 = feature_graph(euler_amd, a.feature_nodes, dim, 11)
        G16.set_dense_feature_dtype(bf16)
        v["bf16_to_fp32"] = lambda: G16.get_dense_feature(q, [0], [dim], out_dtype=f32)
        v["bf16_to_bf16"] = lambda: G16.get_dense_feature(q, [0], [dim])
    by = {"fp32": rows * (dim * 8 + 8), "bf16_to_fp32": rows * (dim * 6 + 8), "bf16_to_bf16": rows * (dim * 4 + 8)}
    res["shapes"]["get_dense_feature_rows%d_d%d" % (rows, dim)] = with_ratios(
        time_variants(v, a.iters, a.repeats, a.warmup), by)

    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
