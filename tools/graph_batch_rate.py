#!/usr/bin/env python3
"""Graph-label path rates: label-index build for 1 000 000 graphs, graph_batch per
minibatch end to end, and the whole-graph block against the SparseGetAdj mask route for the same
batch, alternated in one process.  Shapes: MUTAG-like (128 of 188 graphs x 18 nodes) and
REDDIT-like (512 of 2 000 graphs x 430 nodes, about 500 edges each).  Writes
profiles/graph_batch_rate.json.

    python tools/graph_batch_rate.py [--reps 10] [--out profiles/graph_batch_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402


def multigraph(n_graphs, nodes, edges_per_graph, seed):
    """Graph g = ids [g * nodes + 1, (g + 1) * nodes]; one edge type; every edge inside its graph."""
    rng = np.random.default_rng(seed)
    n = n_graphs * nodes
    # every node 1+ edges, some one more, so that a graph has about edges_per_graph of them
    per = max(edges_per_graph // nodes, 1)
    extra = max(edges_per_graph - per * nodes, 0) / nodes
    deg = per + (rng.random(n) < extra).astype(np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    src = np.repeat(np.arange(n), deg)
    nbr = ((src // nodes) * nodes + rng.integers(0, nodes, len(src)) + 1).astype(np.uint64)
    w = (np.arange(len(src)) - np.repeat(row_ptr[:-1], deg) + 1).astype(np.float32)
    te = deg.astype(np.int32).reshape(n, 1)
    g = euler_amd.Graph.from_csr(np.arange(1, n + 1, dtype=np.uint64), row_ptr, te, nbr, w,
                                 te.astype(np.float32), 1)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    labels = [str(x) for x in (np.arange(n) // nodes).tolist()]
    return g, ids, labels, len(src)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def shape_leg(name, n_graphs, nodes, edges, batch, reps, out):
    g, ids, labels, E = multigraph(n_graphs, nodes, edges, 1)
    g.set_graph_labels(ids, labels)
    g.set_seed(3)
    for _ in range(2):
        g.graph_batch(batch, [0])
    t_batch = timed(lambda: g.graph_batch(batch, [0]), reps)
    _, n_id, _, ei = g.graph_batch(batch, [0])
    N = n_id.numel()
    res = {"graphs": n_graphs, "nodes_per_graph": nodes, "edges_per_graph": E // n_graphs,
           "batch_graphs": batch, "batch_nodes": N, "block_edges": int(ei.shape[1]) - N,
           "graph_batch_ms": t_batch * 1e3}
    # block vs. the SparseGetAdj route, alternated
    tb, tm = [], []
    for _ in range(reps):
        tb.append(timed(lambda: g.whole_graph_block(n_id, [0]), 1))
        tm.append(timed(lambda: g.sparse_get_adj(n_id, n_id, [0]), 1))
    res["block_ms"] = float(np.median(tb)) * 1e3
    res["sparse_get_adj_ms"] = float(np.median(tm)) * 1e3
    # algorithmic bytes of the block: ids in, row records + neighbour ids of the listed edges,
    # one table probe (16 B) per listed edge, the (j, c) keys sorted (about 8 passes x 16 B), out
    listed_edges = N * E // (n_graphs * nodes)
    algo = N * 8 + N * 16 + listed_edges * (8 + 16) + res["block_edges"] * (8 * 16 + 16)
    res["block_algorithmic_bytes"] = int(algo)
    res["block_share_of_8TBps"] = algo / (res["block_ms"] * 1e-3) / 8e12
    out[name] = res
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_batch_rate.json"))
    ap.add_argument("--build-graphs", type=int, default=1_000_000)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    shape_leg("mutag_like", 188, 18, 40, 128, a.reps, out)
    shape_leg("reddit_like", 2000, 430, 500, 512, a.reps, out)
    g, ids, labels, _ = multigraph(a.build_graphs, 10, 10, 2)
    b0 = g.device_bytes
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        g.set_graph_labels(ids, labels)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    n_lab, nbytes = g.label_index_info()
    out["index_build"] = {"graphs": a.build_graphs, "labelled_nodes": n_lab, "seconds": min(ts),
                          "index_bytes": nbytes, "bytes_per_node": nbytes / n_lab,
                          "device_bytes_added": g.device_bytes - b0}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
