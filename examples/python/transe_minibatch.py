#!/usr/bin/env python3
"""Knowledge-graph embedding (TransE l1 / l2, DistMult), one optimiser step on one MI355X.

What examples/TransX/transX.py and examples/distmult/distmult.py do per batch in the reference:

    sample_edge(B)            -> (src, dst, type): the type column is the relation id
    sample_node(B * K)        -> the negatives, reshaped [B, K]
    calculate_energy          -> look up, l2-normalise, tile the true triple K times, score the
                                 true triple and the 2 K corrupted ones (front and tail)
    margin loss, MRR          -> transE.py:52-65, transX.py:81-86

The input pipeline is Graph.sample_edge / Graph.sample_node; calculate_energy is ONE kernel,
ops.triple_score, which reads 3 + K table rows per triple and writes 1 + 2 K floats - the torch
composition (--composed) builds about a dozen [B, K, d] intermediates for the same numbers.  The
tables' gradients come back as sparse tensors over the rows that were looked up, for SparseAdam.

    python examples/python/transe_minibatch.py [--kind trans_l1|trans_l2|distmult] [--composed]
                                               [--batch 64] [--negs 5] [--dim 32] [--data DIR]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import euler_amd                                   # noqa: E402
from euler_amd import ops, optim                   # noqa: E402
from fused_optimizer_check import moved_only_looked_up_rows          # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "fixture_dat")


def sample_batch(G, batch, negs):
    """-> src, rel_id, dst [B] and neg [B, K], all int64 on the device, no host wait"""
    e = G.sample_edge(batch)
    return e[:, 0], e[:, 2], e[:, 1], G.sample_node(batch * negs).reshape(batch, negs)


def composed_score(ent, rel, src, rel_id, dst, neg, kind, normalize=True):
    """calculate_energy with corrupt = 'both' as the reference spells it, in plain torch: the
    lookups (sparse gradients, as the fused op's), norm_emb, the tile, the scores, the concat"""
    emb = torch.nn.functional.embedding

    def norm(x):
        if not normalize:
            return x
        return x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=1e-12))

    def score(a, r, c):
        if kind == "distmult":
            return (a * r * c).sum(-1)
        e = a + r - c
        return -(e.abs().sum(-1) if kind == "trans_l1" else torch.linalg.vector_norm(e, dim=-1))

    k = neg.shape[1]
    h, t, n = (norm(emb(i, ent, sparse=True).float()) for i in (src.reshape(-1, 1), dst.reshape(-1, 1), neg))
    r = norm(emb(rel_id.reshape(-1, 1), rel, sparse=True).float())
    hh, rr, tt = h.expand(-1, k, -1), r.expand(-1, k, -1), t.expand(-1, k, -1)
    return score(h, r, t).reshape(-1), torch.cat([score(n, rr, tt), score(hh, rr, n)], -1)


def energies(ent, rel, src, rel_id, dst, neg, kind, composed=False):
    if composed:
        return composed_score(ent, rel, src, rel_id, dst, neg, kind)
    return ops.triple_score(ent, rel, src, rel_id, dst, neg, kind=kind, corrupt="both", sparse_grad=True)


def margin_loss(pos, neg, margin=1.0):
    """transE.py:52-65: mean over the batch of max(margin + mean_k neg - pos, 0)"""
    return torch.clamp(margin + neg.mean(-1) - pos, min=0).mean()


def mrr(pos, neg):
    """transX.py:81-86: the true triple is the last of [neg | pos]; ties rank it behind"""
    rank = (neg >= pos.reshape(-1, 1)).sum(-1)
    return (1.0 / (rank + 1).float()).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="trans_l1", choices=["trans_l1", "trans_l2", "distmult"])
    ap.add_argument("--composed", action="store_true", help="the torch composition instead of ops.triple_score")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--negs", type=int, default=5)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--fused-optimizer", action="store_true",
                    help="euler_amd.optim.SparseAdam - one fused kernel per table - instead of torch.optim.SparseAdam")
    ap.add_argument("--data", default=FIXTURE, help="a graph directory (euler.meta + .dat); default: the fixture graph")
    a = ap.parse_args()
    torch.manual_seed(0)
    G = euler_amd.Graph.load(a.data, edges=True)
    G.set_seed(7)
    n_ent, n_rel = G.id_range()[0] + 1, G.num_edge_types          # row = node id / edge type
    ent = torch.nn.Parameter(torch.randn((n_ent, a.dim), device="cuda"))
    rel = torch.nn.Parameter(torch.randn((n_rel, a.dim), device="cuda"))
    opt = (optim.SparseAdam if a.fused_optimizer else torch.optim.SparseAdam)([ent, rel], lr=0.01)
    src, rel_id, dst, neg = sample_batch(G, a.batch, a.negs)
    pos, scores = energies(ent, rel, src, rel_id, dst, neg, a.kind, a.composed)
    loss = margin_loss(pos, scores, a.margin)
    opt.zero_grad()
    loss.backward()
    before = [ent.detach().clone(), rel.detach().clone()] if a.fused_optimizer else None
    opt.step()
    if a.fused_optimizer:
        print("fused optimizer: %d rows moved, all of them looked up" % moved_only_looked_up_rows([ent, rel], before))
    rows = int(ent.grad.coalesce().indices().numel())
    print("%s (%s): loss %.6f  mrr %.4f  rows updated %d of %d"
          % (a.kind, "composed" if a.composed else "fused", float(loss), float(mrr(pos.detach(), scores.detach())),
             rows, n_ent))
    assert torch.isfinite(loss) and rows > 0
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
