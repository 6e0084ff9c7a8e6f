#!/usr/bin/env python3
"""Microbenchmark of ops.skipgram_loss (the fused loss head of DeepWalk / LINE / unsupervised
GraphSAGE) against the composition it replaces - three embedding lookups, two batched matmuls,
softplus, a mean and the two sorts of mrr_score, as examples/python/deepwalk_train.py --composed
spells it - on one GPU, same process, same inputs, the two forms alternating.

Shapes: the reference's (run_deepwalk.py: batch 1024, walk_len 3, window 1 -> 4 pairs a node, so
B = 4096 pair rows; P = 1, K = 5) at d in --dims, and --large pair rows so that the kernels are not
launch-bound; two tables of --rows rows in --dtypes.  Timed: the forward alone (loss, rank and
logits), and forward + backward down to the sparse gradients of both tables.  After a warm-up
each sample is --inner back-to-back calls between two device events, divided by --inner; the
median of --repeats samples is reported.
Byte model of the fused forward, per pair row: (1 + P + K) * d * sizeof(element) - the table
rows alone; ids and outputs add 8 * (1 + P + K) + 4 * (P + K + 2).  Its rate is given as a
fraction of 8 TB/s.  One JSON line with every configuration; --out also writes it to a file."""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8e12


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
    ap.add_argument("--batches", type=int, nargs="+", default=[4096], help="pair rows of the reference's shape")
    ap.add_argument("--large", type=int, default=262144, help="pair rows of the shape that is not launch-bound")
    ap.add_argument("--negs", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 20:
        ap.error("--repeats: at least 20 timed samples")

    import torch
    from euler_amd import ops
    if not torch.cuda.is_available():
        sys.exit("ubench_skipgram: needs a GPU (no CPU path is timed)")
    spec = importlib.util.spec_from_file_location(
        "deepwalk_train", os.path.join(ROOT, "examples", "python", "deepwalk_train.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    p, k = 1, args.negs
    results = []
    for d in args.dims:
        t32 = torch.randn((args.rows, d), generator=gen, device="cuda") * d ** -0.5
        c32 = torch.randn((args.rows, d), generator=gen, device="cuda") * d ** -0.5
        for name in args.dtypes:
            target = torch.nn.Parameter(t32.to(getattr(torch, name)))
            context = torch.nn.Parameter(c32.to(getattr(torch, name)))
            element = target.element_size()
            for b in args.batches + [args.large]:
                ids = lambda shape: torch.randint(0, args.rows, shape, generator=gen, device="cuda")    # noqa: E731
                src, pos, neg = ids((b,)), ids((b, p)), ids((b, k))

                def fused():
                    return example.loss_of(target, context, src, pos, neg)

                def composed():
                    return example.loss_of(target, context, src, pos, neg, composed=True)

                def step(forward):
                    target.grad = context.grad = None
                    forward()[0].backward()

                with torch.no_grad():
                    lf, rf, xf = fused()
                    lc, rc, xc = composed()
                    loss_diff = abs(float(lf) - float(lc))
                    logit_diff = float((xf - xc).abs().max())
                    rank_mismatch = int((rf.long() != rc.long()).sum())     # (ties and last-bit differences of the logits)
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
                med = {key: statistics.median(v) for key, v in t.items()}
                row_bytes = (1 + p + k) * d * element
                results.append(dict(
                    dtype=name, pair_rows=b, positives=p, negs=k, dim=d, table_rows=args.rows, repeats=args.repeats,
                    inner=args.inner, fused_fwd_s=med["fused_fwd"], composed_fwd_s=med["composed_fwd"],
                    fwd_speedup=med["composed_fwd"] / med["fused_fwd"],
                    fused_fwd_bwd_s=med["fused_fwd_bwd"], composed_fwd_bwd_s=med["composed_fwd_bwd"],
                    fwd_bwd_speedup=med["composed_fwd_bwd"] / med["fused_fwd_bwd"],
                    fused_fwd_min_s=min(t["fused_fwd"]), fused_fwd_max_s=max(t["fused_fwd"]),
                    composed_fwd_min_s=min(t["composed_fwd"]), composed_fwd_max_s=max(t["composed_fwd"]),
                    byte_model_per_row=row_bytes, byte_model="(1 + P + K) * d * sizeof(element) per pair row",
                    fused_fwd_model_bytes=b * row_bytes,
                    fused_fwd_model_bytes_per_s=b * row_bytes / med["fused_fwd"],
                    fused_fwd_fraction_of_8TBps=b * row_bytes / med["fused_fwd"] / PEAK_BYTES_PER_S,
                    abs_loss_difference=loss_diff, max_abs_logit_difference=logit_diff, rank_mismatches=rank_mismatch))
                print("done: %s d=%d B=%d" % (name, d, b), file=sys.stderr, flush=True)
            target.grad = context.grad = None
            del target, context
        del t32, c32
    line = json.dumps(dict(tool="ubench_skipgram", results=results))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
