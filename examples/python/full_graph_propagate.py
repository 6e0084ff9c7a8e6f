#!/usr/bin/env python3
"""Propagation over the FULL neighbour lists of every node, read straight from the graph's rows.

SGCN's one-off S^K X (sgcn_conv.py), APPNP's power iteration (appnp_conv.py:54-60), a GCN layer over
full neighbours and the embeddings of all nodes after training reduce a table over each node's
stored neighbour list.  One call a hop, with no list of the edges and no host wait:

    norm = (G.neighbor_norm(nodes, et, self_loop=True), G.neighbor_norm(table_ids, et, self_loop=True))
    x = G.neighbor_aggregate("add", x, nodes, et, weight="norm", norm=norm, self_loop=True)       # S x
    h = G.neighbor_aggregate("add", h, nodes, et, weight="norm", norm=norm, self_loop=True,
                             root=h0, alpha=0.1)                                  # an APPNP step

The table is indexed by node id; the script queries the ids 0 .. n (id 0 is no node: only its own
row), so every hop's result is the next hop's table.

    python examples/python/full_graph_propagate.py [--nodes N] [--edges E] [--dim D] [--hops K]
        [--dtype fp32|bf16|fp16] [--weight norm|edge|none] [--composed] [--chunk NODES] [--repeats R]

--composed runs, beside the fused calls, the composition of the existing ops - get_full_neighbor
(two calls and a host wait) over chunks of --chunk nodes, the self ids appended, ops.gcn_aggregate /
ops.gather_segment_reduce - asserts that both give the same bits, and prints both times (hipEvents,
one warm-up, the median of --repeats runs) with the bytes the fused call has to move.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402

ALPHA = 0.1
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def hop(G, x, nodes, et, weight, norm, root, composed, chunk):
    """one hop over all `nodes`: x [rows, D] -> [len(nodes), D]"""
    kw = dict(weight=weight, self_loop=True, alpha=None if root is None else ALPHA)
    if not composed:
        return G.neighbor_aggregate("add", x, nodes, et, norm=norm, root=root, **kw)
    parts = []
    for b in range(0, nodes.numel(), chunk):
        s = slice(b, b + chunk)
        parts.append(G.neighbor_aggregate_composed(
            "add", x, nodes[s], et, norm=None if norm is None else (norm[0][s], norm[1]),
            root=None if root is None else root[s], **kw))
    return torch.cat(parts)


def propagate(G, x0, nodes, et, weight, norm, hops, composed=False, chunk=1 << 20):
    """-> (S^K X, the APPNP iterate after K steps)"""
    s = h = x0
    for _ in range(hops):
        s = hop(G, s, nodes, et, weight, norm, None, composed, chunk)
        h = hop(G, h, nodes, et, weight, norm, x0, composed, chunk)
    return s, h


def timed(fn, repeats):
    """median milliseconds of fn() by hipEvents after one warm-up, and every run's time"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return sorted(times)[len(times) // 2], times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--edges", type=int, default=200000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--hops", type=int, default=2)
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="fp32")
    ap.add_argument("--weight", choices=["norm", "edge", "none"], default="norm")
    ap.add_argument("--composed", action="store_true")
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    weight = None if a.weight == "none" else a.weight
    G = euler_amd.Graph.synthetic(euler_amd.synth_params(7, a.nodes, a.edges, weighted=True))
    et = [0]
    nodes = torch.arange(a.nodes + 1, device="cuda")           # the ids 0 .. n = the table's rows
    gen = torch.Generator(device="cuda").manual_seed(1)
    x0 = (torch.rand((a.nodes + 1, a.dim), device="cuda", generator=gen) - 0.5).to(DTYPES[a.dtype])
    x0[0] = 0
    norm = None
    if weight == "norm":
        nd = G.neighbor_norm(nodes, et, self_loop=True)
        norm = (nd, nd)                                        # the queried ids are the table's rows
    s, h = propagate(G, x0, nodes, et, weight, norm, a.hops)
    torch.cuda.synchronize()
    print("S^%d X and %d APPNP steps over %d nodes / %d listed edges (fused, %s, weight %s): |S^K X| = %.6f, "
          "|H_K| = %.6f" % (a.hops, a.hops, a.nodes, int(G.neighbor_degree(nodes, et).sum()), a.dtype, a.weight,
                            float(s.float().abs().sum()), float(h.float().abs().sum())))
    if not a.composed:
        return
    cs, ch = propagate(G, x0, nodes, et, weight, norm, a.hops, composed=True, chunk=a.chunk)
    assert torch.equal(s.view(torch.uint8), cs.view(torch.uint8)), "S^K X: fused and composed differ"
    assert torch.equal(h.view(torch.uint8), ch.view(torch.uint8)), "APPNP: fused and composed differ"
    print("fused and composed results are bit-identical")
    # one hop of each form, timed
    listed = int(G.neighbor_degree(nodes, et, self_loop=True).sum())
    t_f, all_f = timed(lambda: hop(G, x0, nodes, et, weight, norm, None, False, a.chunk), a.repeats)
    t_c, all_c = timed(lambda: hop(G, x0, nodes, et, weight, norm, None, True, a.chunk), a.repeats)
    esize = x0.element_size()
    # per update: the id (8) and, weighted, the running sums (edge: 4 + 4 cached; norm: a table entry 4)
    # next to the table row; per node: its id, its row record and its output row
    per_update = a.dim * esize + 8 + (4 if weight else 0)
    gbytes = (listed * per_update + (a.nodes + 1) * (8 + 24 + a.dim * esize)) / 1e9
    print("one hop, fused:    %9.3f ms  (%s)  %.1f GB/s by algorithmic bytes (%.3f GB)"
          % (t_f, " ".join("%.3f" % t for t in all_f), gbytes / (t_f * 1e-3), gbytes))
    print("one hop, composed: %9.3f ms  (%s)" % (t_c, " ".join("%.3f" % t for t in all_c)))
    # the hub's tail: the node with the longest list is one wave-slot's loop
    deg = G.neighbor_degree(nodes, et, self_loop=True)
    hub = nodes[int(deg.argmax())].reshape(1)
    hub_norm = None if norm is None else (norm[0][int(deg.argmax())].reshape(1), norm[1])
    t_h, _ = timed(lambda: hop(G, x0, hub, et, weight, hub_norm, None, False, a.chunk), a.repeats)
    print("the longest list (%d entries) alone: %.3f ms = %.1f %% of the fused hop"
          % (int(deg.max()), t_h, 100.0 * t_h / t_f))


if __name__ == "__main__":
    main()
