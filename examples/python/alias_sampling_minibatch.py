#!/usr/bin/env python3
"""The two neighbour draws side by side on a graph of heavy-tailed (Pareto) weights.

The default draw of sample_neighbor / sample_fanout inverts the row's running sums exactly as the
reference does ("exact").  `method="alias"` draws from the same distribution through one alias table
per (row, edge-type group): one 32-byte entry per draw, whatever the degree and the weights - other
neighbours for the same seed, 32 bytes per edge of tables, none of the exact mode's search indexes.
Pareto weights are the kind the exact mode's weight-bucket index declines for its lean kernels
(DESIGN 4.1), so its draws walk the pivot levels here.

    python examples/python/alias_sampling_minibatch.py [--nodes 200000] [--degree 32] [--batch 4096]

Prints, per mode: device_bytes after the mode's first call, the empirical against the exact
probability of a hub row's heaviest and lightest edge, and the time per 2-hop [25, 10] step (device
events, after warm-up).  One graph per mode, so that the bytes are each mode's own.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402

HUB_DEGREE = 2000


def pareto_csr(nodes, degree, seed=7):
    """ids 1 .. nodes, one edge type; node 1 is a hub of HUB_DEGREE distinct neighbours"""
    rng = np.random.default_rng(seed)
    deg = np.full(nodes, degree, np.int64)
    deg[0] = min(HUB_DEGREE, nodes - 1)
    row_ptr = np.zeros(nodes + 1, np.int64)
    row_ptr[1:] = np.cumsum(deg)
    E = int(row_ptr[-1])
    nbr = rng.integers(1, nodes + 1, E).astype(np.uint64)
    nbr[:deg[0]] = np.arange(2, 2 + deg[0], dtype=np.uint64)
    w = ((rng.pareto(0.7, E) + 1) * 0.5).astype(np.float32)
    prefix = np.zeros(E, np.float32)
    total = np.zeros(nodes, np.float32)
    # running f32 sums per row (Node::Init); rows of one length at a time
    for d in np.unique(deg):
        rows = np.nonzero(deg == d)[0]
        idx = row_ptr[rows][:, None] + np.arange(d)[None, :]
        c = np.cumsum(w[idx], axis=1, dtype=np.float32)
        prefix[idx] = c
        total[rows] = c[:, -1]
    return dict(row_id=np.arange(1, nodes + 1, dtype=np.uint64), row_ptr=row_ptr, type_end=deg.astype(np.int32),
                nbr=nbr, prefix_w=prefix, type_prefix=total, n_edge_types=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    csr = pareto_csr(a.nodes, a.degree)
    hub = csr["prefix_w"][:int(csr["row_ptr"][1])].astype(np.float64)
    p = np.diff(np.concatenate([[0.0], hub])) / hub[-1]                  # the exact model of the hub row
    heavy, light = int(np.argmax(p)), int(np.argmin(p))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    roots = torch.randint(1, a.nodes + 1, (8, a.batch), generator=gen, device="cuda")
    hub_root = torch.ones(1, dtype=torch.int64, device="cuda")
    for method in ("exact", "alias"):
        G = euler_amd.Graph.from_csr(**csr)
        G.set_seed(2024)
        G.set_neighbor_method(method)               # every later call of this graph draws this way
        base = G.device_bytes
        G.sample_fanout(roots[0], [[0], [0]], [25, 10], call_id=0)
        torch.cuda.synchronize()
        print("%-5s device_bytes %d after the first call (+%d over the flat arrays)" % (method, G.device_bytes,
                                                                                       G.device_bytes - base))
        draws = 0
        hits = np.zeros(2, np.int64)
        for c in range(64):
            ids = G.sample_neighbor(hub_root, [0], 16384, call_id=1000 + c)[0]
            hits += [int((ids == 2 + heavy).sum()), int((ids == 2 + light).sum())]
            draws += ids.numel()
        print("      hub row, %d draws: heaviest edge %.6f (exact %.6f), lightest edge %.3e (exact %.3e)"
              % (draws, hits[0] / draws, p[heavy], hits[1] / draws, p[light]))
        for i in range(8):                          # warm-up
            G.sample_fanout(roots[i], [[0], [0]], [25, 10], call_id=2 * i)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(a.steps):
            G.sample_fanout(roots[i % 8], [[0], [0]], [25, 10], call_id=100 + 2 * i)
        stop.record()
        torch.cuda.synchronize()
        print("      %.4f ms per [25, 10] step of %d roots" % (start.elapsed_time(stop) / a.steps, a.batch))
        G.close()


if __name__ == "__main__":
    main()
