#!/usr/bin/env python3
"""Microbenchmark of Graph.sparse_feature_embedding (the fused ShallowEncoder lookup) against the
composition it replaces: get_sparse_feature -> row offsets -> gather_segment_reduce("mean",
seg_ptr=), on one GPU, same process, same inputs.

Workload (defaults): a synthetic graph of 10 M nodes with one uint64 slot, entry lists of
geometric length (mean 8, capped at 64) drawn in [0, V), V = 10 M table rows; 1 M queried nodes;
dim 16 and 64; fp32 and bf16 tables; combiner mean.  Warm-up, then the median of --repeats timed
calls by device events, the two forms alternating.

Bytes of the fused kernel counted from shapes: node ids (8 n) + entry ids (8 nnz) + table rows
(nnz * dim * element) + output (n * dim * element).  One JSON line per configuration and a last
line with all of them; --out also writes that to a file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_graph(EA, n_nodes, n_rows, mean_len, cap, seed):
    """ids 1 .. n, one out-edge each (to the next node); one uint64 slot per node"""
    rng = np.random.default_rng(seed)
    ids = np.arange(1, n_nodes + 1, dtype=np.uint64)
    lens = np.minimum(rng.geometric(1.0 / mean_len, n_nodes), cap).astype(np.int64)
    ptr = np.zeros(n_nodes + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    val = rng.integers(0, n_rows, int(ptr[-1]), dtype=np.int64).astype(np.uint64)
    G = EA.Graph.from_csr(ids, np.arange(n_nodes + 1, dtype=np.int64), np.ones(n_nodes, np.int32),
                          np.roll(ids, -1), np.ones(n_nodes, np.float32), np.ones(n_nodes, np.float32),
                          1, sparse_features=(1, ptr, lens.astype(np.int32), val))
    return G, lens


def group_lanes(dim, element, aligned=True):
    """the lane group the launcher picks (sparse_embed.h: SeGroupLanes)"""
    per = 16 // element
    chunks = dim // per if aligned and dim % per == 0 else dim
    g = 1
    while g < 64 and g < chunks:
        g <<= 1
    return g


def timed(torch, fn, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--mean-len", type=float, default=8.0)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--dims", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--combiner", default="mean")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 20:
        ap.error("--repeats: at least 20 timed calls")

    import torch
    import euler_amd as EA
    from euler_amd import ops
    if not torch.cuda.is_available():
        sys.exit("ubench_sparse_embedding: needs a GPU (no CPU path is timed)")

    G, lens = build_graph(EA, args.nodes, args.rows, args.mean_len, args.cap, args.seed)
    rng = np.random.default_rng(args.seed + 1)
    q_np = rng.integers(1, args.nodes + 1, args.queries, dtype=np.int64)
    q = torch.as_tensor(q_np).cuda()
    n = q.numel()
    nnz = int(lens[q_np - 1].sum())
    results = []
    for dim in args.dims:
        base = torch.randn((args.rows, dim), device="cuda")
        for name in args.dtypes:
            dt = getattr(torch, name)
            table = base.to(dt)
            element = table.element_size()

            def fused():
                return G.sparse_feature_embedding(q, [0], [table], args.combiner)[0]

            def composed():
                (ind, val, _), = G.get_sparse_feature(q, [0], [0])
                off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
                off[1:] = torch.cumsum(torch.bincount(ind[:, 0], minlength=n), 0)
                return ops.gather_segment_reduce(args.combiner if args.combiner != "sqrtn" else "add",
                                                 table, val, n, seg_ptr=off)

            # same result up to the composition's mean = sum / (count + 1e-7)
            a, b = fused().float(), composed().float()
            worst = float((a - b).abs().max())
            scale = float(b.abs().max())
            for _ in range(args.warmup):
                fused()
                composed()
            torch.cuda.synchronize()
            tf, tc = [], []
            for _ in range(args.repeats):
                tf.append(timed(torch, fused, 1))
                tc.append(timed(torch, composed, 1))
            bytes_fused = 8 * n + 8 * nnz + nnz * dim * element + n * dim * element
            r = dict(dim=dim, dtype=name, combiner=args.combiner, queries=n, entries=nnz,
                     table_rows=args.rows, group_lanes=group_lanes(dim, element),
                     fused_s=statistics.median(tf), composed_s=statistics.median(tc),
                     fused_min_s=min(tf), fused_max_s=max(tf), composed_min_s=min(tc),
                     composed_max_s=max(tc), repeats=args.repeats,
                     fused_algorithmic_bytes=bytes_fused,
                     fused_bytes_per_s=bytes_fused / statistics.median(tf),
                     speedup=statistics.median(tc) / statistics.median(tf),
                     largest_difference=worst, largest_value=scale)
            print(json.dumps(r), flush=True)
            results.append(r)
            del table
        del base
    line = json.dumps(dict(tool="ubench_sparse_embedding", results=results))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    G.close()


if __name__ == "__main__":
    main()
