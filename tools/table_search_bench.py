#!/usr/bin/env python3
"""Times ops.table_topk and ops.table_rank against the composition they replace - `queries @
table.T` in row chunks whose [Q, rows] fp32 block fits 1 GiB, torch.topk (or a comparison and a
sum) per chunk, the chunks merged: composed_topk / composed_rank of
examples/python/embedding_search.py - on one GPU, same process, same inputs, the two forms
alternating.

Shapes: metric ip, d = 128, k = 10, a table of --rows (10M) rows in bf16 and fp32, fp32 queries,
Q in {25, 1024}.  After a warm-up of every form each sample is one call between two device events;
the median, the least and the largest of --repeats samples are reported.

Models (computed from the shapes, nothing measured):
  bytes of one sweep      N * d * sizeof(element); its rate against the 6.0 TB/s an in-order HBM
                          sweep reaches on this chip is `sweep_fraction` - the figure
                          that matters at Q = 25, where one sweep serves every query.
  VALU lane-operations    2 * d * Q * N (a separately rounded multiply and add per column and pair);
                          against 157.3e12 / 2 a second (the vector fp32 peak counts a fused
                          multiply-add as two) that is `valu_fraction` - the figure at Q = 1024.
One JSON line with every configuration; --out also writes it to a file."""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SWEEP_BYTES_PER_S = 6.0e12
VALU_OPS_PER_S = 157.3e12 / 2


def timed(torch, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--queries", type=int, nargs="+", default=[25, 1024])
    ap.add_argument("--dtypes", nargs="+", default=["bfloat16", "float32"])
    ap.add_argument("--metric", default="ip")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-composed", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from euler_amd import ops
    if not torch.cuda.is_available():
        sys.exit("table_search_bench: needs a GPU (no CPU path is timed)")
    spec = importlib.util.spec_from_file_location(
        "embedding_search", os.path.join(ROOT, "examples", "python", "embedding_search.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    n, d, k = args.rows, args.dim, args.k
    t32 = torch.randn((n, d), generator=gen, device="cuda") * d ** -0.5
    results = []
    for name in args.dtypes:
        table = t32.to(getattr(torch, name))
        for q in args.queries:
            queries = torch.randn((q, d), generator=gen, device="cuda") * d ** -0.5
            target = torch.randint(0, n, (q,), generator=gen, device="cuda")
            forms = {"topk": lambda: ops.table_topk(table, queries, k, metric=args.metric),
                     "rank": lambda: ops.table_rank(table, queries, target, metric=args.metric)}
            if not args.no_composed:
                forms["composed_topk"] = lambda: example.composed_topk(table, queries, k, metric=args.metric)
                forms["composed_rank"] = lambda: example.composed_rank(table, queries, target, metric=args.metric)
            for _ in range(args.warmup):
                for fn in forms.values():
                    fn()
            torch.cuda.synchronize()
            t = {key: [] for key in forms}
            for _ in range(args.repeats):
                for key, fn in forms.items():
                    t[key].append(timed(torch, fn))
            row = dict(dtype=name, rows=n, dim=d, k=k, queries=q, metric=args.metric, repeats=args.repeats,
                       sweep_bytes=n * d * table.element_size(), valu_lane_ops=2 * d * q * n)
            for key, v in t.items():
                row[key + "_s"], row[key + "_min_s"], row[key + "_max_s"] = statistics.median(v), min(v), max(v)
            for key in ("topk", "rank"):
                row[key + "_sweep_fraction"] = row["sweep_bytes"] / row[key + "_s"] / SWEEP_BYTES_PER_S
                row[key + "_valu_fraction"] = row["valu_lane_ops"] / row[key + "_s"] / VALU_OPS_PER_S
            if not args.no_composed:
                row["topk_speedup"] = row["composed_topk_s"] / row["topk_s"]
                row["rank_speedup"] = row["composed_rank_s"] / row["rank_s"]
                rows_f, rows_c = forms["topk"]()[1], forms["composed_topk"]()[1]
                row["rows_equal_fraction"] = float((rows_f == rows_c).float().mean())
                row["rank_equal_fraction"] = float((forms["rank"]() == forms["composed_rank"]()).float().mean())
            results.append(row)
            print("done: %s Q=%d" % (name, q), file=sys.stderr, flush=True)
        del table
    line = json.dumps(dict(tool="table_search_bench", results=results))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
