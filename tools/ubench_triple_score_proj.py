#!/usr/bin/env python3
"""Microbenchmark of ops.triple_score_proj (triple scoring with the TransH / TransD projection
fused in) against the torch composition it replaces - composed_score of
examples/python/transh_transd_minibatch.py, the example's --composed path: on one GPU, same
process, same inputs, the two forms alternating.

Shapes: --batch triples, --negs negatives, d in --dims, entity tables of --ent-rows rows and
relation tables of --rel-rows rows, in --dtypes; --projs and --kinds with corrupt = both.
Timed: the forward alone, and forward + backward of sum(pos) + sum(neg) down to the dense
gradients of every table.  After a warm-up the median of --repeats calls by device events.
Bytes of the fused forward counted from shapes, per triple - hyperplane:
(5 + K) d sizeof + 8 (3 + K) + 4 (1 + 2 K) (h, t, the K negatives, r, w); transfer:
(8 + 2 K) d sizeof + 8 (3 + K) + 4 (1 + 2 K) (an ent and an ent_transfer row per entity, r, rho);
their rate is given as a fraction of 8 TB/s.
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

PEAK_BYTES_PER_S = 8e12


def timed(torch, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3


def load_example():
    spec = importlib.util.spec_from_file_location(
        "transh_transd_minibatch", os.path.join(ROOT, "examples", "python", "transh_transd_minibatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--negs", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--ent-rows", type=int, default=2_000_000)
    ap.add_argument("--rel-rows", type=int, default=1024)
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--projs", nargs="+", default=["hyperplane", "transfer"])
    ap.add_argument("--kinds", nargs="+", default=["trans_l1"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 20:
        ap.error("--repeats: at least 20 timed calls")

    import torch
    if not torch.cuda.is_available():
        sys.exit("ubench_triple_score_proj: needs a GPU (no CPU path is timed)")
    example = load_example()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    b, k = args.batch, args.negs
    ids = lambda hi, shape: torch.randint(0, hi, shape, generator=gen, device="cuda")      # noqa: E731
    src, dst, rel_id, neg = ids(args.ent_rows, (b,)), ids(args.ent_rows, (b,)), ids(args.rel_rows, (b,)), \
        ids(args.ent_rows, (b, k))
    results = []
    for d in args.dims:
        for proj in args.projs:
            for name in args.dtypes:
                tables = example.make_tables(proj, args.ent_rows, args.rel_rows, d, gen=gen, dtype=getattr(torch, name))
                element = tables["ent"].element_size()
                for kind in args.kinds:
                    def fused():
                        return example.energies(proj, tables, src, rel_id, dst, neg, kind, sparse_grad=False)

                    def composed():
                        return example.composed_score(proj, tables, src, rel_id, dst, neg, kind, sparse=False)

                    def step(forward):
                        for t in tables.values():
                            t.grad = None
                        pos, out = forward()
                        (pos.sum() + out.sum()).backward()

                    with torch.no_grad():
                        pf, nf = fused()
                        pc, nc = composed()
                        max_diff = max(float((pf - pc).abs().max()), float((nf - nc).abs().max()))
                    for _ in range(args.warmup):
                        step(fused)
                        step(composed)
                    torch.cuda.synchronize()
                    t = {key: [] for key in ("fused_fwd", "composed_fwd", "fused_fwd_bwd", "composed_fwd_bwd")}
                    for _ in range(args.repeats):
                        with torch.no_grad():
                            t["fused_fwd"].append(timed(torch, fused))
                            t["composed_fwd"].append(timed(torch, composed))
                        t["fused_fwd_bwd"].append(timed(torch, lambda: step(fused)))
                        t["composed_fwd_bwd"].append(timed(torch, lambda: step(composed)))
                    med = {key: statistics.median(v) for key, v in t.items()}
                    rows = (5 + k) if proj == "hyperplane" else (8 + 2 * k)
                    nbytes = b * (rows * d * element + 8 * (3 + k) + 4 * (1 + 2 * k))
                    r = dict(proj=proj, kind=kind, dtype=name, batch=b, negs=k, dim=d, ent_rows=args.ent_rows,
                             rel_rows=args.rel_rows, repeats=args.repeats,
                             fused_fwd_s=med["fused_fwd"], composed_fwd_s=med["composed_fwd"],
                             fwd_speedup=med["composed_fwd"] / med["fused_fwd"],
                             fused_fwd_bwd_s=med["fused_fwd_bwd"], composed_fwd_bwd_s=med["composed_fwd_bwd"],
                             fwd_bwd_speedup=med["composed_fwd_bwd"] / med["fused_fwd_bwd"],
                             fused_fwd_min_s=min(t["fused_fwd"]), fused_fwd_max_s=max(t["fused_fwd"]),
                             composed_fwd_min_s=min(t["composed_fwd"]), composed_fwd_max_s=max(t["composed_fwd"]),
                             fused_fwd_algorithmic_bytes=nbytes,
                             fused_fwd_bytes_per_s=nbytes / med["fused_fwd"],
                             fused_fwd_fraction_of_8TBps=nbytes / med["fused_fwd"] / PEAK_BYTES_PER_S,
                             max_abs_score_difference=max_diff)
                    print(json.dumps(r), flush=True)
                    results.append(r)
                for t in tables.values():
                    t.grad = None
                del tables
                torch.cuda.empty_cache()
    line = json.dumps(dict(tool="ubench_triple_score_proj", results=results))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
