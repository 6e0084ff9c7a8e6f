#!/usr/bin/env python3
"""Microbenchmark of ops.triple_score (the fused energies of TransE / DistMult) against the
composition it replaces, built only from ops.gather, torch element-wise ops and - through
gather's gradient - ops.scatter_add: on one GPU, same process, same inputs, the two forms
alternating.

Shapes: --batch triples, --negs negatives, d in --dims, an entity table of --ent-rows rows and a
relation table of --rel-rows rows, in --dtypes; --kinds with corrupt = both and normalize on.
Timed: the forward alone, and forward + backward of sum(pos) + sum(neg) down to the dense
gradients of both tables.  After a warm-up the median of --repeats calls by device events.
Bytes of the fused forward counted from shapes, per triple:
(3 + K) d sizeof + 8 (3 + K) + 4 (1 + 2 K); their rate is given as a fraction of 8 TB/s.
One JSON line per configuration and a last line with all of them; --out also writes that to a file."""
import argparse
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


def composed_score(torch, ops, ent, rel, src, rel_id, dst, neg, kind):
    """calculate_energy as the reference spells it: gather, l2_normalize, tile, score, concat"""
    b, k = neg.shape

    def rows(table, ids):
        return ops.gather(table, ids.reshape(-1).to(torch.int32), out_dtype=torch.float32)

    def norm(x):
        return x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=1e-12))

    def score(a, r, c):
        if kind == "distmult":
            return (a * r * c).sum(-1)
        e = a + r - c
        return -(e.abs().sum(-1) if kind == "trans_l1" else torch.linalg.vector_norm(e, dim=-1))

    looked_up = norm(rows(ent, torch.cat([src, dst, neg.reshape(-1)])))          # one gather, one scatter_add back
    h, t, n = looked_up[:b].reshape(b, 1, -1), looked_up[b:2 * b].reshape(b, 1, -1), looked_up[2 * b:].reshape(b, k, -1)
    r = norm(rows(rel, rel_id)).reshape(b, 1, -1)
    hh, rr, tt = h.expand(-1, k, -1), r.expand(-1, k, -1), t.expand(-1, k, -1)
    return score(h, r, t).reshape(-1), torch.cat([score(n, rr, tt), score(hh, rr, n)], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--negs", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--ent-rows", type=int, default=2_000_000)
    ap.add_argument("--rel-rows", type=int, default=1024)
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--kinds", nargs="+", default=["trans_l1", "distmult"])
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
        sys.exit("ubench_triple_score: needs a GPU (no CPU path is timed)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    b, k = args.batch, args.negs
    ids = lambda hi, shape: torch.randint(0, hi, shape, generator=gen, device="cuda")      # noqa: E731
    src, dst, rel_id, neg = ids(args.ent_rows, (b,)), ids(args.ent_rows, (b,)), ids(args.rel_rows, (b,)), \
        ids(args.ent_rows, (b, k))
    results = []
    for d in args.dims:
        ent32 = torch.randn((args.ent_rows, d), generator=gen, device="cuda")
        rel32 = torch.randn((args.rel_rows, d), generator=gen, device="cuda")
        for name in args.dtypes:
            ent = ent32.to(getattr(torch, name)).requires_grad_()
            rel = rel32.to(getattr(torch, name)).requires_grad_()
            element = ent.element_size()
            for kind in args.kinds:
                def fused():
                    return ops.triple_score(ent, rel, src, rel_id, dst, neg, kind=kind)

                def composed():
                    return composed_score(torch, ops, ent, rel, src, rel_id, dst, neg, kind)

                def step(forward):
                    ent.grad = rel.grad = None
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
                nbytes = b * ((3 + k) * d * element + 8 * (3 + k) + 4 * (1 + 2 * k))
                r = dict(kind=kind, dtype=name, batch=b, negs=k, dim=d, ent_rows=args.ent_rows,
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
            ent.grad = rel.grad = None
            del ent, rel
        del ent32, rel32
    line = json.dumps(dict(tool="ubench_triple_score", results=results))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
