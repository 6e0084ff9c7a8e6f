#!/usr/bin/env python3
"""Microbenchmark of ops.relation_conv(route="fused") (one MFMA pass, no [size, R, F] block) against
route="composed" (relation_reduce, then the torch GEMM) - on one GPU, same process, same inputs,
the two routes alternating, without gradients.

Configurations (a table of --rows rows, --dst destinations x 25 draws, types uniform at random, one
entry in 16 of type -1, count=25; those of tools/ubench_relation_reduce.py):
  a    R = 8,  F = dim = 128
  c    R = 8,  F = dim = 32
  r64  R = 64, F = dim = 128
each for --dtypes and --aggr.

After a warm-up the median of --repeats calls by device events.  Per route also the growth of
torch.cuda.max_memory_allocated over one call.  Algorithmic bytes from shapes: gather indices and
types (4 E each) + the rows of the valid updates + the weight + the output; the composed route
adds the block, written once and read once.  One JSON line per configuration and a last line with
all of them; --out also writes that to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"a": (8, 128), "c": (8, 32), "r64": (64, 128)}


def timed(torch, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3


def family(R, f, dim, esz):
    """which instantiations RelDenseMakePlan (csrc/mp_relation_dense.h) picks: all R matrices within 64 KB or not"""
    cols = 16
    while cols < dim:
        cols *= 2
    column = (f + 31) // 32 * 32 * esz
    column += 0 if column % 256 == 0 else 16
    return "resident" if R * cols * column <= 65536 else "phased"


def peak_growth(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    del out
    return grown


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dst", type=int, default=131072)
    ap.add_argument("--count", type=int, default=25)
    ap.add_argument("--configs", nargs="+", default=["a", "c", "r64"], choices=sorted(SHAPES))
    ap.add_argument("--dtypes", nargs="+", default=["bfloat16", "float32"])
    ap.add_argument("--aggr", nargs="+", default=["mean"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 20:
        ap.error("--repeats: at least 20 timed calls")

    import torch
    from euler_amd import ops
    if not torch.cuda.is_available():
        sys.exit("ubench_relation_conv: needs a GPU (no CPU path is timed)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    results = []
    for cfg in args.configs:
        R, d = SHAPES[cfg]
        size, e = args.dst, args.dst * args.count
        t = torch.randint(0, R, (e,), generator=gen, device="cuda", dtype=torch.int32)
        t[torch.rand(e, generator=gen, device="cuda") < 1.0 / 16] = -1
        gi = torch.randint(0, args.rows, (e,), generator=gen, device="cuda", dtype=torch.int32)
        n_valid = int((t >= 0).sum())
        base = torch.randn((args.rows, d), device="cuda", generator=gen)
        for name in args.dtypes:
            x = base.to(getattr(torch, name))
            w = (torch.randn((R, d, d), device="cuda", generator=gen) / d ** 0.5).to(x.dtype)
            esz = x.element_size()
            for aggr in args.aggr:
                with torch.no_grad():
                    call = {route: (lambda route=route: ops.relation_conv(x, w, gi, t, size, count=args.count, aggr=aggr,
                                                                          route=route)) for route in ("fused", "composed")}
                    diff = float((call["fused"]().float() - call["composed"]().float()).abs().max())
                    for _ in range(args.warmup):
                        call["fused"]()
                        call["composed"]()
                    torch.cuda.synchronize()
                    times = {"fused": [], "composed": []}
                    for _ in range(args.repeats):
                        for route in times:
                            times[route].append(timed(torch, call[route]))
                    peak = {route: peak_growth(torch, call[route]) for route in times}
                shared = 8 * e + n_valid * d * esz + R * d * d * esz + size * d * esz
                r = dict(config=cfg, aggr=aggr, dtype=name, destinations=size, updates=e, valid_updates=n_valid,
                         relations=R, f=d, dim=d, table_rows=args.rows, repeats=args.repeats, max_abs_difference=diff,
                         family=family(R, d, d, esz),
                         fused_s=statistics.median(times["fused"]), composed_s=statistics.median(times["composed"]),
                         fused_min_s=min(times["fused"]), fused_max_s=max(times["fused"]),
                         composed_min_s=min(times["composed"]), composed_max_s=max(times["composed"]),
                         fused_algorithmic_bytes=shared, composed_algorithmic_bytes=shared + 2 * size * R * d * esz,
                         fused_peak_bytes=peak["fused"], composed_peak_bytes=peak["composed"],
                         speedup=statistics.median(times["composed"]) / statistics.median(times["fused"]))
                print(json.dumps(r), flush=True)
                results.append(r)
            del x, w
        del base
    line = json.dumps(dict(tool="ubench_relation_conv", results=results))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
