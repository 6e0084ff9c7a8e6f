#!/usr/bin/env python3
"""fp32 vs bf16 vs fp8 (e4m3fn codes + per-column scale, ops.Fp8Rows) feature tables, one GPU.

Times, with device events, for each shape
  - block aggregation (ops.gather_segment_reduce "mean", int64 ids, `count` per destination):
    count = 10 and 25, D = 128 and 256, n_dst = 256 000, on a table of 1 M rows (the shapes of
    tools/bench_half_mp.py, for comparability) and on one of 8 M rows read at random - larger in
    every format than the L2 and the 256 MB Infinity Cache together
  - ops.gather of 281 600 rows of the 1 M-row, 128-d table
the variants fp32, bf16 -> fp32, fp8 -> fp32 and fp8 -> bf16 of one call, and prints ONE JSON line
(also written to --out): per shape the median milliseconds of every variant, their ratios to fp32
and to bf16 -> fp32, and beside every time ratio the byte ratio the algorithm needs (computed from
the shapes: the gathered rows, the output, the ids; the d scales of an fp8 table are noise).

Protocol (tools/bench_half_mp.py): every variant of a shape is warmed up, then timed in windows
of --iters calls between two events; the variants alternate window by window (--repeats rounds)
and the median window is reported with the spread (min, max).

--root DIR imports euler_amd from another checkout of this repository: one that has no Fp8Rows
(an earlier commit) yields the fp32 and bf16 columns alone, the numbers this commit's must match.

    python tools/bench_fp8_rows.py [--out profiles/fp8_rows.json] [--root DIR] [--big-rows 8000000]
"""
import argparse
import json
import os
import statistics
import sys

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
    out = {"times": times, "algo_bytes": {k: b for k, b in bytes_per_variant.items() if k in times}}
    for base in ("fp32", "bf16_to_fp32"):
        if base in times and len(times) > 1:
            out["time_ratio_to_" + base] = {k: round(v["ms"] / times[base]["ms"], 4) for k, v in times.items()}
            out["byte_ratio_to_" + base] = {k: round(bytes_per_variant[k] / bytes_per_variant[base], 4)
                                            for k in times}
    for k, v in times.items():
        v["algo_GBps"] = round(bytes_per_variant[k] / (v["ms"] * 1e-3) / 1e9, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--root", default="")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-dst", type=int, default=256_000)
    ap.add_argument("--table-rows", type=int, default=1_000_000)
    ap.add_argument("--big-rows", type=int, default=8_000_000, help="0: leave the large table out")
    ap.add_argument("--gather-rows", type=int, default=281_600)
    a = ap.parse_args()
    root = os.path.abspath(a.root) if a.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import euler_amd      # noqa: F401
    from euler_amd import ops
    if not torch.cuda.is_available():
        sys.exit("bench_fp8_rows: needs a GPU (nothing here is measured on a CPU)")
    fp8 = hasattr(ops, "Fp8Rows")
    bf16, f32 = torch.bfloat16, torch.float32
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    res = {"tool": "bench_fp8_rows", "device": torch.cuda.get_device_name(0), "package_root": os.path.basename(root),
           "has_fp8_rows": fp8, "iters": a.iters, "repeats": a.repeats, "shapes": {}}
    n_dst = a.n_dst

    def tables(rows, d):
        t = torch.randn((rows, d), generator=gen, device="cuda")
        return t, t.to(bf16), (ops.Fp8Rows.quantize(t) if fp8 else None)

    for rows in [a.table_rows] + ([a.big_rows] if a.big_rows else []):
        for d in (128, 256):
            t32, t16, t8 = tables(rows, d)
            for count in (10, 25):
                ids = torch.randint(0, rows, (n_dst * count,), generator=gen, device="cuda", dtype=torch.int64)
                v = {"fp32": lambda: ops.gather_segment_reduce("mean", t32, ids, n_dst, count=count),
                     "bf16_to_fp32": lambda: ops.gather_segment_reduce("mean", t16, ids, n_dst, count=count,
                                                                       out_dtype=f32)}
                if fp8:
                    v["fp8_to_fp32"] = lambda: ops.gather_segment_reduce("mean", t8, ids, n_dst, count=count)
                    v["fp8_to_bf16"] = lambda: ops.gather_segment_reduce("mean", t8, ids, n_dst, count=count,
                                                                         out_dtype=bf16)
                idb = 8 * count                                       # the ids of a destination
                by = {"fp32": n_dst * (count * d * 4 + d * 4 + idb),
                      "bf16_to_fp32": n_dst * (count * d * 2 + d * 4 + idb),
                      "fp8_to_fp32": n_dst * (count * d + d * 4 + idb),
                      "fp8_to_bf16": n_dst * (count * d + d * 2 + idb)}
                res["shapes"]["block_mean_rows%d_count%d_d%d" % (rows, count, d)] = with_ratios(
                    time_variants(v, a.iters, a.repeats, a.warmup), by)
            if rows == a.table_rows and d == 128:
                e = a.gather_rows
                idx = torch.randint(0, rows, (e,), generator=gen, device="cuda", dtype=torch.int32)
                v = {"fp32": lambda: ops.gather(t32, idx),
                     "bf16_to_fp32": lambda: ops.gather(t16, idx, out_dtype=f32)}
                if fp8:
                    v["fp8_to_fp32"] = lambda: ops.gather(t8, idx)
                    v["fp8_to_bf16"] = lambda: ops.gather(t8, idx, out_dtype=bf16)
                by = {"fp32": e * (d * 8 + 4), "bf16_to_fp32": e * (d * 6 + 4), "fp8_to_fp32": e * (d * 5 + 4),
                      "fp8_to_bf16": e * (d * 3 + 4)}
                res["shapes"]["gather_rows%d_d%d" % (e, d)] = with_ratios(
                    time_variants(v, a.iters, a.repeats, a.warmup), by)
            del t32, t16, t8
            torch.cuda.empty_cache()

    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
