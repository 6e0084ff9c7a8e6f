#!/usr/bin/env python3
"""Microbenchmark of ops.triple_score_matrix (triple scoring with TransR's per-relation matrix
projection fused in) against the torch composition it replaces - composed_score of
examples/python/transr_minibatch.py, the example's --composed path, which is the reference's
formulation: on one GPU, same process, same inputs, the two forms alternating.

Shapes (--shapes): "reference" - run_transR.py's defaults, B = 128, K = 1, de = dr = 100, FB15k's
14 951 entities and 1 345 relations, relation ids uniform; "large" - B = 65 536, K = 5, the same
dims and tables, relation ids Zipf-distributed (p ~ 1 / rank).  --batch / --negs / --dims override.
Timed: the forward alone, and forward + backward of sum(pos) + sum(neg) down to the dense
gradients of all three tables.  After a warm-up the median of --repeats calls by device events;
the peak allocation of one forward + backward of each form is read from the caching allocator.
Operations of the fused form counted from shapes: 2 de dr (2 + K) per triple forward.
One JSON line per configuration and a last line with all of them; --out also writes that to a file."""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"reference": dict(batch=128, negs=1, zipf=False), "large": dict(batch=65536, negs=5, zipf=True)}


def timed(torch, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3


def load_example():
    spec = importlib.util.spec_from_file_location(
        "transr_minibatch", os.path.join(ROOT, "examples", "python", "transr_minibatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["reference", "large"], choices=sorted(SHAPES))
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--negs", type=int, default=None)
    ap.add_argument("--dims", type=int, nargs=2, default=[100, 100], metavar=("DE", "DR"))
    ap.add_argument("--ent-rows", type=int, default=14951)
    ap.add_argument("--rel-rows", type=int, default=1345)
    ap.add_argument("--dtypes", nargs="+", default=["float32"])
    ap.add_argument("--kinds", nargs="+", default=["trans_l1"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fused-only", action="store_true", help="time the fused form alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 20 and not args.fused_only:
        ap.error("--repeats: at least 20 timed calls")

    import torch
    if not torch.cuda.is_available():
        sys.exit("ubench_triple_score_matrix: needs a GPU (no CPU path is timed)")
    example = load_example()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    de, dr = args.dims
    results = []
    for shape in args.shapes:
        b = args.batch or SHAPES[shape]["batch"]
        k = args.negs if args.negs is not None else SHAPES[shape]["negs"]
        ids = lambda hi, size: torch.randint(0, hi, size, generator=gen, device="cuda")      # noqa: E731
        src, dst, neg = ids(args.ent_rows, (b,)), ids(args.ent_rows, (b,)), ids(args.ent_rows, (b, k))
        if SHAPES[shape]["zipf"]:
            p = 1.0 / torch.arange(1, args.rel_rows + 1, device="cuda", dtype=torch.float64)
            rel_id = torch.multinomial(p, b, replacement=True, generator=gen)
        else:
            rel_id = ids(args.rel_rows, (b,))
        for name in args.dtypes:
            tables = example.make_tables(args.ent_rows, args.rel_rows, de, dr, gen=gen, dtype=getattr(torch, name))
            for kind in args.kinds:
                def fused():
                    return example.energies(tables, src, rel_id, dst, neg, kind, sparse_grad=False)

                def composed():
                    return example.composed_score(tables, src, rel_id, dst, neg, kind, sparse=False)

                def step(forward):
                    for t in tables.values():
                        t.grad = None
                    pos, out = forward()
                    (pos.sum() + out.sum()).backward()

                def peak(forward):
                    for t in tables.values():
                        t.grad = None
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    step(forward)
                    torch.cuda.synchronize()
                    return torch.cuda.max_memory_allocated() - before

                forms = (("fused", fused),) if args.fused_only else (("fused", fused), ("composed", composed))
                max_diff = None
                if not args.fused_only:
                    with torch.no_grad():
                        pf, nf = fused()
                        pc, nc = composed()
                        max_diff = max(float((pf - pc).abs().max()), float((nf - nc).abs().max()))
                        del pf, nf, pc, nc
                for _ in range(args.warmup):
                    for _, form in forms:
                        step(form)
                torch.cuda.synchronize()
                t = {"%s_%s" % (n, w): [] for n, _ in forms for w in ("fwd", "fwd_bwd")}
                for _ in range(args.repeats):
                    for n, form in forms:
                        with torch.no_grad():
                            t[n + "_fwd"].append(timed(torch, form))
                        t[n + "_fwd_bwd"].append(timed(torch, lambda: step(form)))
                med = {key: statistics.median(v) for key, v in t.items()}
                flops = 2.0 * de * dr * (2 + k) * b
                r = dict(shape=shape, kind=kind, dtype=name, batch=b, negs=k, ent_dim=de, rel_dim=dr,
                         ent_rows=args.ent_rows, rel_rows=args.rel_rows, repeats=args.repeats,
                         relations_used=int(torch.unique(rel_id).numel()),
                         fused_fwd_projection_flops=flops, fused_fwd_flops_per_s=flops / med["fused_fwd"],
                         max_abs_score_difference=max_diff)
                for key, v in t.items():
                    r[key + "_s"], r[key + "_min_s"], r[key + "_max_s"] = med[key], min(v), max(v)
                for n, form in forms:
                    r[n + "_peak_alloc_bytes"] = peak(form)
                if not args.fused_only:
                    r["fwd_speedup"] = med["composed_fwd"] / med["fused_fwd"]
                    r["fwd_bwd_speedup"] = med["composed_fwd_bwd"] / med["fused_fwd_bwd"]
                    r["peak_alloc_ratio"] = r["composed_peak_alloc_bytes"] / max(r["fused_peak_alloc_bytes"], 1)
                print(json.dumps(r), flush=True)
                results.append(r)
            for t in tables.values():
                t.grad = None
            del tables
            torch.cuda.empty_cache()
    line = json.dumps(dict(tool="ubench_triple_score_matrix", results=results))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
