#!/usr/bin/env python
"""One optimiser step of euler_amd.optim.SparseAdam (one fused call per table: keys, sort, step)
against torch.optim.SparseAdam (coalesce, sparse_mask, a dozen element-wise launches) on the SAME
sparse gradient tensors.

  --shape deepwalk   the step of examples/python/deepwalk_train.py at its defaults: 200 000 nodes,
                     d = 128, batch 1024, walks of 3, 5 negatives; the gradients of target and
                     context are what skipgram_loss(..., sparse_grad=True) hands to the optimiser
  --shape hub        one table of 200 000 rows, d = 128, and an uncoalesced gradient of 65 536
                     occurrences, half of them on 16 hub rows

Both optimisers run in one process and alternate: a repeat is `--steps` steps of one between two
device events, then of the other; the first repeat is warm-up and is dropped.  Printed: one JSON
line with the median time of a step over the repeats, its min - max spread, and fused / torch.

Run each shape as its own command under its own time limit and stop at the first failure:
  timeout -k 10 300 python tools/bench_sparse_optim.py --shape deepwalk && \\
  timeout -k 10 300 python tools/bench_sparse_optim.py --shape hub"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples", "python"))
import euler_amd                                   # noqa: E402
from euler_amd import euler_ops, optim             # noqa: E402


def deepwalk_gradients(nodes, dim, batch):
    """[(table, sparse gradient)] of one deepwalk_train.py step on its synthetic graph"""
    import deepwalk_train as ex
    G = euler_amd.Graph.synthetic(euler_amd.synth_params(1, nodes, 10 * nodes, weighted=True))
    G.set_node_sampler()
    euler_ops.set_default_graph(G)
    G.set_seed(42)
    target, context = ex.make_tables(nodes, dim)
    src, pos, negs = ex.sample_step(batch, nodes)
    loss, _, _ = ex.loss_of(target, context, src, pos, negs)
    loss.backward()
    return [(target.detach(), target.grad), (context.detach(), context.grad)]


def hub_gradients(rows, dim, e, hubs):
    gen = torch.Generator(device="cuda").manual_seed(0)
    ids = torch.randint(0, rows, (e,), device="cuda", generator=gen)
    ids[::2] = torch.randint(0, hubs, (e // 2,), device="cuda", generator=gen)
    values = torch.randn((e, dim), device="cuda", generator=gen) * 0.01
    table = torch.randn((rows, dim), device="cuda", generator=gen) * dim ** -0.5
    return [(table, torch.sparse_coo_tensor(ids.reshape(1, -1), values, (rows, dim)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="deepwalk", choices=["deepwalk", "hub"])
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--occurrences", type=int, default=65536)
    ap.add_argument("--hubs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--lr", type=float, default=0.01)
    a = ap.parse_args()
    pairs = deepwalk_gradients(a.nodes, a.dim, a.batch) if a.shape == "deepwalk" else \
        hub_gradients(a.nodes, a.dim, a.occurrences, a.hubs)

    def make(cls):
        params = []
        for table, grad in pairs:
            p = torch.nn.Parameter(table.clone())
            p.grad = grad                               # the same gradient tensors for both
            params.append(p)
        return cls(params, lr=a.lr)

    opts = {"fused": make(optim.SparseAdam), "torch": make(torch.optim.SparseAdam)}
    times = {k: [] for k in opts}
    for rep in range(a.repeats + 1):
        for name, opt in opts.items():
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            for _ in range(a.steps):
                opt.step()
            end.record()
            end.synchronize()
            if rep:                                     # (repeat 0: warm-up)
                times[name].append(begin.elapsed_time(end) / a.steps)
    out = {"shape": a.shape, "rows": a.nodes + (2 if a.shape == "deepwalk" else 0), "d": a.dim,
           "occurrences": [int(g._values().shape[0]) for _, g in pairs], "steps": a.steps, "repeats": a.repeats}
    for name, ts in times.items():
        out[name + "_ms"] = round(statistics.median(ts), 4)
        out[name + "_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
    out["fused_over_torch"] = round(out["fused_ms"] / out["torch_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
