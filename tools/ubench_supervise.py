#!/usr/bin/env python3
"""Microbenchmark of ops.supervise_loss (the fused loss head of the supervised models) against the
composition it replaces, on one GPU, same process, same inputs, the two forms alternating.

Shapes: B = --batch logit rows with C in --classes columns, fp32 logits and hard labels.
  loss + f1   fused: ops.supervise_loss with a metrics.Streaming("f1").  composed: what
              examples/python/graphsage_train.py --composed spells - binary_cross_entropy_with_logits,
              sigmoid, floor(p + 0.5) and the masked sums of tp / fp / fn, kept on the device (no
              host read; only calls that exist without the fused head).  Forward alone, and forward
              + backward down to the gradient of the logits.
  loss + auc  fused: the same call with a metrics.Streaming("auc") of --thresholds thresholds.
              composed: tf.metrics.auc's formulation - every prediction compared with every
              threshold, a [T, B * C] block, and four masked sums per threshold.  If the device
              refuses that block the fact is recorded instead of a time.
  histograms  the fused loss + auc call on uniform predictions (logits ~ N(0, 3)) and on
              concentrated ones (N(0, 0.01): every prediction in a few buckets, the contended case
              of a trained model) - for this library and, with --alt-lib, for a build with the
              other histogram strategy (make OUT=... EXTRA=-DEULER_GPU_SV_HIST_LDS=0: one 64-bit
              integer atomic per element straight to memory instead of a histogram in LDS per
              block), timed by a child process with EULER_GPU_LIB_PATH set.
After a warm-up each sample is --inner back-to-back calls between two device events, divided by
--inner; the median of --repeats samples is reported.  One JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import subprocess
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


def median_of(torch, fns, warmup, repeats, inner):
    """the forms alternate inside every repeat -> {name: (median, min, max)}"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(timed(torch, fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def composed_f1(torch, logits, labels, counts):
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels)
    with torch.no_grad():
        pred = torch.floor(torch.sigmoid(logits) + 0.5)
        lab, prd = labels != 0, pred != 0
        counts += torch.stack([(lab & prd).sum(), (~lab & prd).sum(), (lab & ~prd).sum()])
    return loss


def composed_auc(torch, logits, labels, thr, acc):
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels)
    with torch.no_grad():
        p = torch.sigmoid(logits).reshape(1, -1)
        lab = (labels != 0).reshape(1, -1)
        over = p > thr.reshape(-1, 1)                                   # [T, B * C]
        acc[0] += (over & lab).sum(1)
        acc[1] += (over & ~lab).sum(1)
        acc[2] += (~over & lab).sum(1)
        acc[3] += (~over & ~lab).sum(1)
    return loss


def histogram_times(torch, args):
    """the fused loss + auc forward on uniform and on concentrated predictions, per C"""
    from euler_amd import metrics, ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    out = []
    for c in args.classes:
        row = dict(classes=c)
        for name, scale in (("uniform", 3.0), ("concentrated", 0.01)):
            x = torch.randn((args.batch, c), generator=gen, device="cuda") * scale
            z = (torch.rand((args.batch, c), generator=gen, device="cuda") < 0.3).float()
            m = metrics.Streaming("auc", args.thresholds)
            with torch.no_grad():
                med = median_of(torch, {"t": lambda: ops.supervise_loss(x, z, metric=m)}, args.warmup, args.repeats,
                                args.inner)["t"]
            row[name + "_s"], row[name + "_min_s"], row[name + "_max_s"] = med
            row[name + "_hist_sum"] = int(m.hist.sum())
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--classes", type=int, nargs="+", default=[1, 41, 121])
    ap.add_argument("--thresholds", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--alt-lib", default=None, help="a libeuler_gpu.so built with the other histogram strategy")
    ap.add_argument("--names", nargs=2, default=["this library", "--alt-lib"],
                    help="what to call the histogram strategy of this library and of --alt-lib in the output")
    ap.add_argument("--histograms-only", action="store_true", help="(the child process of --alt-lib)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 20:
        ap.error("--repeats: at least 20 timed samples")

    import torch
    from euler_amd import _lib, metrics, ops
    if not torch.cuda.is_available():
        sys.exit("ubench_supervise: needs a GPU (no CPU path is timed)")
    if args.histograms_only:
        print(json.dumps(dict(lib=_lib.LIB_PATH, histograms=histogram_times(torch, args))))
        return
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    results = []
    for c in args.classes:
        x = (torch.randn((args.batch, c), generator=gen, device="cuda") * 3).requires_grad_()
        z = (torch.rand((args.batch, c), generator=gen, device="cuda") < 0.3).float()
        f1, auc = metrics.Streaming("f1"), metrics.Streaming("auc", args.thresholds)
        counts = torch.zeros(3, dtype=torch.int64, device="cuda")

        def step(forward):
            x.grad = None
            forward().backward()

        fused = lambda: ops.supervise_loss(x, z, metric=f1)                          # noqa: E731
        composed = lambda: composed_f1(torch, x, z, counts)                          # noqa: E731
        with torch.no_grad():
            loss_diff = abs(float(fused()) - float(composed()))
        count_diff = int((f1.counts[:3] - counts).abs().sum())
        fwd = {}
        with torch.no_grad():
            fwd = median_of(torch, {"fused": fused, "composed": composed}, args.warmup, args.repeats, args.inner)
        both = median_of(torch, {"fused": lambda: step(fused), "composed": lambda: step(composed)}, args.warmup,
                         args.repeats, args.inner)
        row = dict(batch=args.batch, classes=c, repeats=args.repeats, inner=args.inner,
                   f1_fused_fwd_s=fwd["fused"][0], f1_composed_fwd_s=fwd["composed"][0],
                   f1_fwd_speedup=fwd["composed"][0] / fwd["fused"][0],
                   f1_fused_fwd_min_s=fwd["fused"][1], f1_fused_fwd_max_s=fwd["fused"][2],
                   f1_composed_fwd_min_s=fwd["composed"][1], f1_composed_fwd_max_s=fwd["composed"][2],
                   f1_fused_fwd_bwd_s=both["fused"][0], f1_composed_fwd_bwd_s=both["composed"][0],
                   f1_fwd_bwd_speedup=both["composed"][0] / both["fused"][0],
                   abs_loss_difference=loss_diff, count_mismatches=count_diff)
        # loss + auc
        fused_auc = lambda: ops.supervise_loss(x, z, metric=auc)                     # noqa: E731
        with torch.no_grad():
            row["auc_fused_fwd_s"] = median_of(torch, {"t": fused_auc}, args.warmup, args.repeats, args.inner)["t"][0]
        row["auc_thresholds"] = args.thresholds
        row["auc_composed_block_bytes"] = args.thresholds * args.batch * c
        try:
            thr = torch.linspace(0, 1, args.thresholds, device="cuda")
            acc = torch.zeros((4, args.thresholds), dtype=torch.int64, device="cuda")
            with torch.no_grad():
                t = median_of(torch, {"t": lambda: composed_auc(torch, x, z, thr, acc)}, 1, args.repeats, 1)["t"]
            row["auc_composed_fwd_s"], row["auc_fwd_speedup"] = t[0], t[0] / row["auc_fused_fwd_s"]
        except RuntimeError as err:                                       # (torch.OutOfMemoryError is one)
            row["auc_composed_fwd_s"] = None
            row["auc_composed_refused"] = str(err).splitlines()[0][:200]
            torch.cuda.empty_cache()
        results.append(row)
        print("done: C=%d" % c, file=sys.stderr, flush=True)
    doc = dict(tool="ubench_supervise", results=results,
               histograms=[dict(lib=args.names[0], rows=histogram_times(torch, args))])
    if args.alt_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--histograms-only", "--batch", str(args.batch),
               "--thresholds", str(args.thresholds), "--repeats", str(args.repeats), "--inner", str(args.inner),
               "--seed", str(args.seed), "--classes"] + [str(c) for c in args.classes]
        r = subprocess.run(cmd, env=dict(os.environ, EULER_GPU_LIB_PATH=os.path.abspath(args.alt_lib)),
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit("ubench_supervise: the --alt-lib run failed:\n" + r.stderr[-2000:])
        doc["histograms"].append(dict(lib=args.names[1], rows=json.loads(r.stdout.strip().splitlines()[-1])["histograms"]))
    line = json.dumps(doc)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
