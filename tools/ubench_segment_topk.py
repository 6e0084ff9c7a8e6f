#!/usr/bin/env python3
"""Microbenchmark of ops.gather_segment_topk (the fused per-column top-k of LGCN) against the
composition it replaces, built from existing ops only - ops.gather, a view [B, nb, d] and
torch.topk(dim=1) - on one GPU, in the same process, on the same inputs, the two forms alternating.

Shapes: --batch roots with nb sampled neighbours each, top k, d columns, a table of --rows rows;
the (nb, k) pairs of --shapes in --dtypes.  The gather indices are int64 ids for the fused op (read
in place) and their int32 cast, made outside the timed region, for the composition.
COLD ROWS: every call reads another of --id-sets random id sets, both forms walking the same sets
in the same order, and the default table (2M rows: 1 GB in fp32, 512 MB in bf16) is larger than the
256 MiB Infinity Cache, so a call does not find the rows of the call before it on the die; a row
can still be resident by chance (at most cache / table of them).
Timed: the forward alone (no_grad) and forward + backward of a fixed random output gradient down to
the dense table gradient.  After --warmup rounds every sample is the device-event time of --inner
back-to-back calls divided by --inner; --repeats samples per form, reported as median, min and max,
and the spread (max - min) / median.  The fused forward's algorithmic traffic, counted from shapes,
is (e d + size k d) sizeof with e = batch * nb; its rate is given over the median time.
One JSON line per configuration and a last line with all of them; --out also writes that to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(torch, fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--shapes", nargs="+", default=["10,3", "25,8"], help="nb,k pairs")
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--id-sets", type=int, default=16)
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 20:
        ap.error("--repeats: at least 20 timed samples")

    import torch
    from euler_amd import ops
    if not torch.cuda.is_available():
        sys.exit("ubench_segment_topk: needs a GPU (no CPU path is timed)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    b, d = args.batch, args.dim
    table32 = torch.randn((args.rows, d), generator=gen, device="cuda")
    results = []
    for shape in args.shapes:
        nb, k = (int(x) for x in shape.split(","))
        id_sets = [torch.randint(0, args.rows, (b * nb,), generator=gen, device="cuda") for _ in range(args.id_sets)]
        id_sets32 = [ids.to(torch.int32) for ids in id_sets]
        for name in args.dtypes:
            table = table32.to(getattr(torch, name)).requires_grad_()
            w = torch.randn((b, k, d), generator=gen, device="cuda").to(table.dtype)
            turn = {"fused": 0, "composed": 0}

            def fused():
                turn["fused"] += 1
                return ops.gather_segment_topk(table, id_sets[turn["fused"] % args.id_sets], b, k, count=nb)

            def composed():
                turn["composed"] += 1
                ids32 = id_sets32[turn["composed"] % args.id_sets]
                return torch.topk(ops.gather(table, ids32).view(b, nb, d), k, dim=1).values

            def step(forward):
                table.grad = None
                forward().backward(w)

            with torch.no_grad():
                same = bool(torch.equal(fused(), composed()))
            for _ in range(args.warmup):
                step(fused)
                step(composed)
            torch.cuda.synchronize()
            t = {key: [] for key in ("fused_fwd", "composed_fwd", "fused_fwd_bwd", "composed_fwd_bwd")}
            for _ in range(args.repeats):
                with torch.no_grad():
                    t["fused_fwd"].append(timed(torch, fused, args.inner))
                    t["composed_fwd"].append(timed(torch, composed, args.inner))
                t["fused_fwd_bwd"].append(timed(torch, lambda: step(fused), args.inner))
                t["composed_fwd_bwd"].append(timed(torch, lambda: step(composed), args.inner))
            nbytes = (b * nb * d + b * k * d) * table.element_size()
            r = dict(dtype=name, batch=b, nb=nb, k=k, dim=d, rows=args.rows, id_sets=args.id_sets,
                     table_bytes=table.numel() * table.element_size(), repeats=args.repeats, inner=args.inner,
                     values_equal=same)
            for key, v in t.items():
                med = statistics.median(v)
                r[key + "_s"], r[key + "_min_s"], r[key + "_max_s"] = med, min(v), max(v)
                r[key + "_spread"] = (max(v) - min(v)) / med
            r["fwd_speedup"] = r["composed_fwd_s"] / r["fused_fwd_s"]
            r["fwd_bwd_speedup"] = r["composed_fwd_bwd_s"] / r["fused_fwd_bwd_s"]
            # the fused forward beats the composition by more than the run-to-run spread of the two
            r["fwd_faster_beyond_spread"] = r["fused_fwd_max_s"] < r["composed_fwd_min_s"]
            r["fused_fwd_algorithmic_bytes"] = nbytes
            r["fused_fwd_bytes_per_s"] = nbytes / r["fused_fwd_s"]
            print(json.dumps(r), flush=True)
            results.append(r)
            table.grad = None
            del table
    line = json.dumps(dict(tool="ubench_segment_topk", results=results))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
