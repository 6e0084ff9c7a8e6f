#!/usr/bin/env python3
"""The fused edge_softmax against the scatter_softmax composition, one GPU, one process.

Times, with device events and after warm-up, forward and forward + backward of
  - fused:    ops.edge_softmax (one read and one write of the [E, H] logits; its own gradient kernel)
  - composed: ops.scatter_softmax, unchanged: scatter_max, gather, subtract, torch.exp, scatter_add,
              gather, divide - and their autograd
on
  - a sampled block: --n-dst destinations x --count updates, H in {1, 8}, fp32 and bf16, given as
    sorted keys, as unsorted keys (a shuffle; both sides then sort) and as `count` (the
    composition has no such form: it gets the sorted keys)
  - a power-law seg_ptr block of the same E (with a hub of --hub updates; the composition gets
    the sorted keys)
and prints ONE JSON line (also written to --out): the median milliseconds of every variant with the
spread over the windows, the algorithmic bytes of the fused op (logits + keys + output) and the
fraction of 8 TB/s they imply.

Protocol: every variant is warmed up, then timed in windows of --iters calls between two events;
the variants alternate window by window (--repeats rounds); the median window is reported.

    python tools/edge_softmax_bench.py [--out profiles/edge_softmax.json]
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


def fwd_bwd(f, x, g):
    def run():
        xr = x.detach().requires_grad_(True)
        f(xr).backward(g)
    return run


def bench_row(ops, name, x, g, fused_kw, keys, size, key_bytes, a, res):
    fused = lambda t: ops.edge_softmax(t, **fused_kw)
    composed = lambda t: ops.scatter_softmax(t, keys, size)
    v = {"fused_fwd": lambda: fused(x), "composed_fwd": lambda: composed(x),
         "fused_fwd_bwd": fwd_bwd(fused, x, g), "composed_fwd_bwd": fwd_bwd(composed, x, g)}
    times = time_variants(v, a.iters, a.repeats, a.warmup)
    elt = x.element_size()
    by = {"fused_fwd": x.numel() * elt * 2 + key_bytes,
          "fused_fwd_bwd": x.numel() * elt * 2 + key_bytes + x.numel() * (4 + elt + elt) + key_bytes}
    if x.dtype != torch.float32:       # (training keeps an fp32 output: written once more, read by the backward)
        by["fused_fwd_bwd"] = x.numel() * (elt + 4 + 4 + elt) + key_bytes + x.numel() * (4 + elt + elt) + key_bytes
    for k in by:
        times[k]["algo_bytes"] = by[k]
        times[k]["fraction_of_8TBps"] = round(by[k] / (times[k]["ms"] * 1e-3) / 8e12, 4)
    res["rows"][name] = {"e": x.shape[0], "heads": x.shape[1], "size": size, "dtype": str(x.dtype)[6:],
                         "times": times,
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
    ap.add_argument("--hub", type=int, default=100_000)
    a = ap.parse_args()
    from euler_amd import ops
    if not torch.cuda.is_available():
        sys.exit("edge_softmax_bench: needs a GPU (nothing here is measured on a CPU)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    res = {"tool": "edge_softmax_bench", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "repeats": a.repeats, "warmup": a.warmup, "rows": {}}
    size, e = a.n_dst, a.n_dst * a.count
    keys = torch.arange(size, device="cuda", dtype=torch.int32).repeat_interleave(a.count)
    shuffle = torch.randperm(e, generator=gen, device="cuda")
    keys_u = keys[shuffle].contiguous()
    # power law: Pareto lengths scaled to the same E, one hub, a fifth of the destinations empty
    rng = np.random.default_rng(5)
    lens = rng.pareto(1.3, size) + 0.2
    lens[rng.random(size) < 0.2] = 0
    lens = np.floor(lens * (e - a.hub) / lens.sum()).astype(np.int64)
    lens[size // 2] += e - lens.sum()
    sp = torch.as_tensor(np.concatenate([[0], np.cumsum(lens)]), device="cuda")
    keys_p = torch.repeat_interleave(torch.arange(size, device="cuda", dtype=torch.int32),
                                     torch.as_tensor(lens, device="cuda"))
    res["power_law"] = {"longest": int(lens.max()), "empty": int((lens == 0).sum()),
                        "longer_than_32": int((lens > 32).sum())}
    for heads in (1, 8):
        for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            x = (torch.randn((e, heads), generator=gen, device="cuda") * 3).to(dt)
            g = torch.randn((e, heads), generator=gen, device="cuda").to(dt)
            rows = (("sorted_keys", {"indices": keys, "size": size}, keys, e * 4),
                    ("unsorted_keys", {"indices": keys_u, "size": size}, keys_u, e * 4),
                    ("count", {"count": a.count, "size": size}, keys, 0),
                    ("power_law_seg_ptr", {"seg_ptr": sp, "size": size}, keys_p, (size + 1) * 8))
            for name, kw, ck, kb in rows:
                bench_row(ops, "%s_H%d_%s" % (name, heads, tag), x, g, kw, ck, size, kb, a, res)
            del x, g
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
