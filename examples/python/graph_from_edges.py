#!/usr/bin/env python3
"""A graph straight from an edge list on the device: Graph.from_edges.

What OGB, PyG and most pipelines hand over is `edge_index` [2, E], optionally an edge type and a
weight per edge, and a feature matrix - already tensors.  from_edges turns them into the graph on the
device: rows, the reference's grouping by edge type, Node::Init's sequential fp32 sums, the id map,
the search index and the node sampler, with no host pass over the edges and no converted files.

    python examples/python/graph_from_edges.py [--nodes 20000] [--edges 200000] [--batch 512]

In this order:
  1. a random typed, weighted edge_index and an [N, 64] feature tensor, on the device;
  2. G = Graph.from_edges(edge_index, ..., undirected=True);
  3. one GraphSAGE minibatch on G: sage_blocks -> get_dense_feature -> gather_segment_reduce;
  4. the same minibatch on the twin Graph.from_csr makes from a numpy layout of the same edges
     (what a user had to write before), asserted equal bit for bit.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402
from euler_amd import ops                          # noqa: E402


def csr_on_the_host(src, dst, typ, w, n_nodes, n_types):
    """The reference's layout of an edge list, restated on the host: rows 1 .. n_nodes, entries grouped
    by type in input order, running fp32 sums added one after the other (cumsum adds in order)."""
    key = (src - 1) * n_types + typ
    order = np.argsort(key, kind="stable")
    seg = np.searchsorted(key[order], np.arange(n_nodes * n_types + 1))
    nbr, w = dst[order].astype(np.uint64), w[order].astype(np.float32)
    row_ptr = seg[::n_types].astype(np.int64)
    type_end = (seg[1:].reshape(n_nodes, n_types) - row_ptr[:-1, None]).astype(np.int32)
    prefix = np.zeros(len(w), np.float32)
    type_prefix = np.zeros((n_nodes, n_types), np.float32)
    for r in range(n_nodes):
        prefix[row_ptr[r]:row_ptr[r + 1]] = np.cumsum(w[row_ptr[r]:row_ptr[r + 1]], dtype=np.float32)
        run = np.float32(0)
        for t in range(n_types):
            group = w[seg[r * n_types + t]:seg[r * n_types + t + 1]]
            run = run + (np.cumsum(group, dtype=np.float32)[-1] if len(group) else np.float32(0))
            type_prefix[r, t] = run
    return row_ptr, type_end, nbr, prefix, type_prefix


def minibatch(G, roots, fanouts, dim):
    """one GraphSAGE input: the sampled blocks, the outermost layer's features, a mean per block"""
    n_types = G.num_edge_types
    blocks, counts = G.sage_blocks(roots, [list(range(n_types))] * len(fanouts), fanouts, add_self_loops=False,
                                   call_id=0)
    x = G.get_dense_feature(blocks[-1][0], [0], [dim])[0]
    for h in reversed(range(len(fanouts))):
        n_id, _, edge_src, edge_dst, _ = blocks[h]
        # without self loops a block is `fanout` consecutive edges per node of layer h: edge_src names
        # that node, edge_dst a row of n_id - the layer the features (then the aggregates) were fetched for
        assert x.shape[0] == n_id.numel() and int(edge_dst.max()) < n_id.numel()
        assert torch.equal(edge_src, torch.arange(counts[h], device=edge_src.device).repeat_interleave(fanouts[h]))
        x = ops.gather_segment_reduce("mean", x, edge_dst.to(torch.int32), counts[h], count=fanouts[h])
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--edges", type=int, default=200000)
    ap.add_argument("--types", type=int, default=2)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--dim", type=int, default=64)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    edge_index = torch.randint(1, a.nodes + 1, (2, a.edges), device="cuda", generator=gen)
    edge_type = torch.randint(0, a.types, (a.edges,), device="cuda", generator=gen, dtype=torch.int32)
    weight = torch.rand(a.edges, device="cuda", generator=gen) * 4 + 0.5
    feat = torch.randn(a.nodes, a.dim, device="cuda", generator=gen)
    nodes = torch.arange(1, a.nodes + 1, device="cuda")

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    G = euler_amd.Graph.from_edges(edge_index, edge_type=edge_type, weight=weight, n_edge_types=a.types,
                                   nodes=nodes, features=[feat], undirected=True)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0

    t0 = time.perf_counter()
    ei = edge_index.cpu().numpy()
    src, dst = np.concatenate([ei[0], ei[1]]), np.concatenate([ei[1], ei[0]])      # undirected
    typ = np.tile(edge_type.cpu().numpy(), 2).astype(np.int64)
    w = np.tile(weight.cpu().numpy(), 2)
    row_ptr, type_end, nbr, prefix, type_prefix = csr_on_the_host(src, dst, typ, w, a.nodes, a.types)
    fval = feat.cpu().numpy().reshape(-1)
    twin = euler_amd.Graph.from_csr(np.arange(1, a.nodes + 1, dtype=np.uint64), row_ptr, type_end, nbr, prefix,
                                    type_prefix, a.types,
                                    features=(1, np.arange(a.nodes + 1, dtype=np.int64) * a.dim,
                                              np.full(a.nodes, a.dim, np.int32), fval))
    t_host = time.perf_counter() - t0

    roots = torch.randint(1, a.nodes + 1, (a.batch,), device="cuda", generator=gen)
    G.set_seed(42)
    twin.set_seed(42)
    x = minibatch(G, roots, [5, 3], a.dim)
    y = minibatch(twin, roots, [5, 3], a.dim)
    assert G.num_edges == twin.num_edges == 2 * a.edges
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "from_edges and from_csr disagree"
    print("%d nodes, %d edges given, %d stored (undirected), %d edge types" % (a.nodes, a.edges, G.num_edges, a.types))
    print("from_edges: %.1f ms on the device; the host layout + from_csr: %.1f ms (wall clock, one run each, first-call costs included)"
          % (t_dev * 1e3, t_host * 1e3))
    print("one GraphSAGE minibatch of %d roots: %d x %d aggregated rows, bit-equal on both graphs"
          % (a.batch, x.shape[0], x.shape[1]))


if __name__ == "__main__":
    main()
