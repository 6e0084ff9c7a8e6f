#!/usr/bin/env python3
"""Microbenchmark of ops.relation_reduce (the fused per-relation aggregation of an RGCN layer)
against the composition it replaces: the keys dst * R + type built in torch, then
ops.gather_scatter - on one GPU, same process, same inputs, the two forms alternating.

Configurations (a table of --rows rows):
  a  sampled block: --dst destinations x 25 draws, R = 8, D = 128; types uniform at random (the
     keys are unsorted), one entry in 16 has type -1; the fused call takes count=25
  b  full-neighbour block: geometric segment lengths (mean 16, capped at 256), types
     non-decreasing inside a destination (the keys are sorted), R = 8 and R = 64, D = 128; the
     fused call takes the block's scatter keys (indices=), as RelationDataFlow gives them
  c  configuration a with D = 32
each in fp32 and bf16, for --ops (mean_rel: the composition is ONE gather_scatter("mean");
mean: its add, then the division by the destination's count in torch).

After a warm-up the median of --repeats calls by device events; wall time (call + wait) too, since
the composition waits on the host.  Bytes of the fused call counted from shapes: gather indices
and types (4 E each, + 4 E keys in b) + the rows of the valid updates + the output.  One JSON line
per configuration and a last line with all of them; --out also writes that to a file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(torch, fn):
    """-> (device seconds by events, wall seconds until the result is there)"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3, time.perf_counter() - t0


def sampled_block(torch, gen, size, count, R):
    e = size * count
    t = torch.randint(0, R, (e,), generator=gen, device="cuda", dtype=torch.int32)
    t[torch.rand(e, generator=gen, device="cuda") < 1.0 / 16] = -1
    dst = torch.arange(size, device="cuda", dtype=torch.int32).repeat_interleave(count)
    return dict(e=e, types=t, dst=dst, kw={"count": count}, key_bytes=0)


def full_block(torch, gen, size, R, mean_len=16.0, cap=256):
    u = torch.rand(size, generator=gen, device="cuda", dtype=torch.float64)
    lens = torch.clamp(torch.floor(torch.log1p(-u) / torch.log1p(torch.tensor(-1.0 / mean_len))) + 1, max=cap).long()
    dst = torch.arange(size, device="cuda").repeat_interleave(lens)
    e = int(dst.numel())
    t = torch.randint(0, R, (e,), generator=gen, device="cuda")
    t = (torch.sort(dst * R + t).values % R).to(torch.int32)        # non-decreasing inside a destination
    dst = dst.to(torch.int32)
    return dict(e=e, types=t, dst=dst, kw={"indices": dst}, key_bytes=4 * e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dst", type=int, default=131072)
    ap.add_argument("--configs", nargs="+", default=["a", "b8", "b64", "c"])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--ops", nargs="+", default=["mean_rel", "mean"])
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
        sys.exit("ubench_relation_reduce: needs a GPU (no CPU path is timed)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    shapes = {"a": ("sampled", 8, 128), "b8": ("full", 8, 128), "b64": ("full", 64, 128), "c": ("sampled", 8, 32)}
    results = []
    tables = {}
    for cfg in args.configs:
        kind, R, dim = shapes[cfg]
        size = args.dst
        blk = sampled_block(torch, gen, size, 25, R) if kind == "sampled" else full_block(torch, gen, size, R)
        e, t, dst, kw = blk["e"], blk["types"], blk["dst"], blk["kw"]
        gi = torch.randint(0, args.rows, (e,), generator=gen, device="cuda", dtype=torch.int32)
        n_valid = int((t >= 0).sum())
        if dim not in tables:
            tables.clear()
            tables[dim] = torch.randn((args.rows, dim), device="cuda")
        for name in args.dtypes:
            table = tables[dim].to(getattr(torch, name))
            element = table.element_size()
            for op in args.ops:
                def fused():
                    return ops.relation_reduce(op, table, gi, t, R, size, **kw)

                def composed():
                    valid = (t >= 0) & (t < R)
                    key = torch.where(valid, dst * R + t, torch.full_like(t, -1))
                    if op == "mean_rel":
                        return ops.gather_scatter("mean", table, gi, key, size * R).view(size, R, dim)
                    s = ops.gather_scatter("add", table, gi, key, size * R, out_dtype=torch.float32)
                    n = torch.zeros(size, dtype=torch.float32, device="cuda").index_add_(0, dst.long(), valid.float())
                    return (s.view(size, R, dim) / (n + 1e-7).view(size, 1, 1)).to(table.dtype)

                same = bool(torch.equal(fused(), composed()))
                for _ in range(args.warmup):
                    fused()
                    composed()
                torch.cuda.synchronize()
                tf, tc, wf, wc = [], [], [], []
                for _ in range(args.repeats):
                    d, w = timed(torch, fused)
                    tf.append(d)
                    wf.append(w)
                    d, w = timed(torch, composed)
                    tc.append(d)
                    wc.append(w)
                nbytes = 8 * e + blk["key_bytes"] + n_valid * dim * element + size * R * dim * element
                r = dict(config=cfg, kind=kind, op=op, dtype=name, destinations=size, updates=e,
                         valid_updates=n_valid, relations=R, dim=dim, table_rows=args.rows,
                         fused_s=statistics.median(tf), composed_s=statistics.median(tc),
                         fused_min_s=min(tf), fused_max_s=max(tf), composed_min_s=min(tc), composed_max_s=max(tc),
                         fused_wall_s=statistics.median(wf), composed_wall_s=statistics.median(wc),
                         repeats=args.repeats, fused_algorithmic_bytes=nbytes,
                         fused_bytes_per_s=nbytes / statistics.median(tf),
                         speedup=statistics.median(tc) / statistics.median(tf), same_bits=same)
                print(json.dumps(r), flush=True)
                results.append(r)
            del table
    line = json.dumps(dict(tool="ubench_relation_reduce", results=results))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
