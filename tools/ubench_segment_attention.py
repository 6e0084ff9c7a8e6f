#!/usr/bin/env python3
"""The fused attention_aggregate against the three-op composition, one GPU, one process.

Times, with device events and after warm-up, forward and forward + backward of
  - fused:    ops.attention_aggregate (euler_gpu_segment_attention and its _grad)
  - composed: ops.edge_dot (dot) or two ops.gather, an add and a leaky_relu (additive), then
              ops.edge_softmax, then ops.gather_segment_reduce("add", ..., edge_weight=alpha) -
              existing code, with its own autograd
on
  - a sampled block: --n-dst destinations x --count updates of a table of --n-src rows, D = --dim,
    H in {1, 8}, fp32 and bf16: dot with v=None (AGNN: one table), dot with v != k, additive (GAT)
  - a pooled batch: --graphs graphs with power-law sizes through seg_ptr, every node once:
    dot with v=None (Set2Set) and additive without q (AttentionPool)
and prints ONE JSON line (also written to --out): the median milliseconds of every variant with the
min and max over the windows, the algorithmic bytes of the fused forward (every gathered row once a
table, the gather indices, q and out) and the fraction of 8 TB/s they imply.

Protocol: every variant is warmed up, then timed in windows of --iters calls between two events;
the variants alternate window by window (--repeats rounds); the median window is reported.

    python tools/ubench_segment_attention.py [--out profiles/segment_attention.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def time_variants(variants, iters, repeats, warmup):
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


def fwd_bwd(f, tensors, g):
    def run():
        leaves = [None if t is None else t.detach().requires_grad_(True) for t in tensors]
        f(*leaves).backward(g)
    return run


def make_fns(ops, kind, heads, gi, dst, size, form, scale, slope):
    def fused(q, k, v):
        return ops.attention_aggregate(kind, q, k, gi, size, v=v, heads=heads, scale=scale, negative_slope=slope,
                                       out_dtype=torch.float32, **form)

    def composed(q, k, v):
        if kind == "dot":
            logits = ops.edge_dot(q, dst, k, gi, heads=heads, out_dtype=torch.float32) * scale
        else:
            s = ops.gather(k, gi, out_dtype=torch.float32)
            if q is not None:
                s = s + ops.gather(q, dst, out_dtype=torch.float32)
            logits = torch.nn.functional.leaky_relu(s, slope)
        alpha = ops.edge_softmax(logits, **dict(form, size=size))
        return ops.gather_segment_reduce("add", k if v is None else v, gi, size, edge_weight=alpha,
                                         out_dtype=torch.float32, **form)
    return fused, composed


def bench_row(ops, name, kind, heads, q, k, v, gi, dst, size, form, a, res):
    fused, composed = make_fns(ops, kind, heads, gi, dst, size, form, 0.37, 0.2)
    dv = (k if v is None else v).shape[1]
    g = torch.randn((size, dv), device="cuda")
    t = (q, k, v)
    variants = {"fused_fwd": lambda: fused(*t), "composed_fwd": lambda: composed(*t),
                "fused_fwd_bwd": fwd_bwd(fused, t, g), "composed_fwd_bwd": fwd_bwd(composed, t, g)}
    times = time_variants(variants, a.iters, a.repeats, a.warmup)
    e, elt = gi.numel(), k.element_size()
    algo = e * k.shape[1] * elt + (0 if v is None else e * dv * elt) + e * gi.element_size() + \
        (0 if q is None else size * q.shape[1] * elt) + size * dv * 4
    times["fused_fwd"]["algo_bytes"] = algo
    times["fused_fwd"]["fraction_of_8TBps"] = round(algo / (times["fused_fwd"]["ms"] * 1e-3) / 8e12, 4)
    res["rows"][name] = {"e": e, "size": size, "heads": heads, "d": k.shape[1], "dv": dv,
                         "dtype": str(k.dtype)[6:], "times": times,
                         "fused_over_composed_fwd": round(times["fused_fwd"]["ms"] / times["composed_fwd"]["ms"], 4),
                         "fused_over_composed_fwd_bwd":
                             round(times["fused_fwd_bwd"]["ms"] / times["composed_fwd_bwd"]["ms"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-dst", type=int, default=16384 * 25)
    ap.add_argument("--count", type=int, default=10)
    ap.add_argument("--n-src", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=1 << 20, help="nodes of the pooled batch")
    a = ap.parse_args()
    from euler_amd import ops
    if not torch.cuda.is_available():
        sys.exit("ubench_segment_attention: needs a GPU (nothing here is measured on a CPU)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    res = {"tool": "ubench_segment_attention", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "repeats": a.repeats, "warmup": a.warmup, "rows": {}}
    size, e, d = a.n_dst, a.n_dst * a.count, a.dim
    gi = torch.randint(0, a.n_src, (e,), generator=gen, device="cuda", dtype=torch.int32)
    dst = torch.arange(size, device="cuda", dtype=torch.int32).repeat_interleave(a.count)
    form = {"count": a.count}
    for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        k = (torch.randn((a.n_src, d), generator=gen, device="cuda") * 0.3).to(dt)
        v = torch.randn((a.n_src, d), generator=gen, device="cuda").to(dt)
        q = (torch.randn((size, d), generator=gen, device="cuda") * 0.3).to(dt)
        for heads in (1, 8):
            sk = torch.randn((a.n_src, heads), generator=gen, device="cuda").to(dt)
            sq = torch.randn((size, heads), generator=gen, device="cuda").to(dt)
            bench_row(ops, "block_dot_shared_H%d_%s" % (heads, tag), "dot", heads, q, k, None, gi, dst, size, form, a, res)
            bench_row(ops, "block_dot_two_tables_H%d_%s" % (heads, tag), "dot", heads, q, k, v, gi, dst, size, form, a, res)
            bench_row(ops, "block_additive_H%d_%s" % (heads, tag), "additive", heads, sq, sk, v, gi, dst, size, form, a, res)
        del k, v, q
    # the pooled batch: power-law graph sizes, every node once, in graph order
    rng = np.random.default_rng(5)
    lens = rng.pareto(1.3, a.graphs) + 0.2
    lens = np.maximum(np.floor(lens * a.nodes / lens.sum()).astype(np.int64), 1)
    n = int(lens.sum())
    sp = torch.as_tensor(np.concatenate([[0], np.cumsum(lens)]), device="cuda")
    nodes = torch.arange(n, device="cuda", dtype=torch.int32)
    graph = torch.repeat_interleave(torch.arange(a.graphs, device="cuda", dtype=torch.int32),
                                    torch.as_tensor(lens, device="cuda"))
    res["pool"] = {"nodes": n, "largest": int(lens.max()), "longer_than_32": int((lens > 32).sum())}
    for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        x = torch.randn((n, d), generator=gen, device="cuda").to(dt)
        qg = (torch.randn((a.graphs, d), generator=gen, device="cuda") * 0.3).to(dt)
        gate = torch.randn((n, 1), generator=gen, device="cuda").to(dt)
        bench_row(ops, "pool_set2set_%s" % tag, "dot", 1, qg, x, None, nodes, graph, a.graphs, {"seg_ptr": sp}, a, res)
        bench_row(ops, "pool_attention_%s" % tag, "additive", 1, None, gate, x, nodes, graph, a.graphs,
                  {"seg_ptr": sp}, a, res)
        del x, qg, gate
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
