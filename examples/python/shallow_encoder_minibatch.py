#!/usr/bin/env python3
"""ShallowEncoder on the tf_euler operator surface, end to end on one MI355X: node ids plus one
sparse (uint64) feature to embeddings, a hop-1 mean aggregation, and one training step.

What tf_euler/python/utils/encoders.py:146-170 does per node in the reference -
get_sparse_feature, then tf.nn.embedding_lookup_sparse(table, sp, None, combiner) - is ONE call
here, with no SparseTensor in between and no host wait:

    emb, = G.sparse_feature_embedding(nodes, [0], [table], "mean", default_values=[V - 1],
                                      sparse_grad=True)

The table's gradient arrives as a torch.sparse_coo_tensor over the rows the batch read, which is
what torch.optim.SparseAdam consumes: a table of 10^7 rows never sees a dense gradient.

    python examples/python/shallow_encoder_minibatch.py [--nodes 2000] [--batch 64] [--dim 16]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import euler_amd                                   # noqa: E402
from euler_amd import ops, optim                   # noqa: E402
from fused_optimizer_check import moved_only_looked_up_rows          # noqa: E402


def ring_graph(n, vocab, seed):
    """ids 1 .. n, each with edges to the next two nodes; one uint64 slot of 0 .. 12 values in
    [0, vocab - 1) per node (row vocab - 1 of the table is kept for nodes without values)"""
    rng = np.random.default_rng(seed)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    nbr = np.stack([np.roll(ids, -1), np.roll(ids, -2)], 1).reshape(-1)
    lens = rng.integers(0, 13, n)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    values = rng.integers(0, vocab - 1, int(ptr[-1]), dtype=np.int64).astype(np.uint64)
    return euler_amd.Graph.from_csr(
        ids, np.arange(0, 2 * n + 1, 2, dtype=np.int64), np.full(n, 2, np.int32), nbr,
        np.tile(np.array([1, 2], np.float32), n), np.full(n, 2, np.float32), 1,
        sparse_features=(1, ptr, lens.astype(np.int32), values))


def encode(G, nodes, id_table, feat_table):
    """ShallowEncoder with use_id and one sparse feature, combiner "add" over the two parts"""
    by_id = ops.gather(id_table, nodes.reshape(-1))                     # ids 1 .. n; row 0 = default node
    by_feature, = G.sparse_feature_embedding(nodes, [0], [feat_table], "mean",
                                             default_values=[feat_table.shape[0] - 1], sparse_grad=True)
    return by_id + by_feature


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--fanout", type=int, default=5)
    ap.add_argument("--fused-optimizer", action="store_true",
                    help="euler_amd.optim.SparseAdam - one fused kernel per table - instead of torch.optim.SparseAdam")
    a = ap.parse_args()
    torch.manual_seed(0)
    G = ring_graph(a.nodes, a.vocab, 1)
    G.set_seed(42)
    id_table = (torch.randn(a.nodes + 1, a.dim, device="cuda") * 0.1).requires_grad_(True)
    feat_table = (torch.randn(a.vocab, a.dim, device="cuda") * 0.1).requires_grad_(True)
    opt_sparse = (optim.SparseAdam if a.fused_optimizer else torch.optim.SparseAdam)([feat_table], lr=0.01)
    opt_dense = torch.optim.SGD([id_table], lr=0.01)

    roots = torch.randint(1, a.nodes + 1, (a.batch,), device="cuda")
    nbrs, _, _ = G.sample_neighbor(roots, [0], a.fanout, default_node=0)
    # hop 1 of GraphSAGE's mean aggregator over the encoder's rows: self + mean of the neighbours
    h_self = encode(G, roots, id_table, feat_table)
    h_nbr = encode(G, nbrs.reshape(-1), id_table, feat_table)
    dst = torch.arange(a.batch, device="cuda", dtype=torch.int32).repeat_interleave(a.fanout)
    h = h_self + ops.scatter_mean(h_nbr, dst, a.batch)
    loss = (h * h).mean()
    before = feat_table.detach().clone()
    opt_sparse.zero_grad()
    opt_dense.zero_grad()
    loss.backward()
    assert feat_table.grad.is_sparse
    rows_read = feat_table.grad.coalesce().indices().shape[1]
    opt_sparse.step()
    opt_dense.step()
    torch.cuda.synchronize()
    moved = int((feat_table.detach() != before).any(dim=1).sum())
    if a.fused_optimizer:
        print("fused optimizer: %d rows moved, all of them looked up" % moved_only_looked_up_rows([feat_table], [before]))
    print("ShallowEncoder step: %d roots x fanout %d, dim %d, loss %.6f; sparse gradient over %d of %d "
          "table rows, %d rows updated by SparseAdam"
          % (a.batch, a.fanout, a.dim, float(loss.detach()), rows_read, a.vocab, moved))
    G.close()


if __name__ == "__main__":
    main()
