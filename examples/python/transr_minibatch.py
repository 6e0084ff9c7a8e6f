#!/usr/bin/env python3
"""Knowledge-graph embedding with a per-relation matrix (TransR), one optimiser step on one MI355X.

What examples/TransX/transR.py does per batch in the reference:

    sample_edge(B)            -> (src, dst, type): the type column is the relation id
    sample_node(B * K)        -> the negatives, reshaped [B, K]
    generate_embedding        -> look up the entity and relation rows and ONE [de * dr] matrix per
                                 triple, tile that matrix over the K negatives, run a batched
                                 [1, de] x [de, dr] product per entity row, l2-normalise
    calculate_scores          -> the true triple and the 2 K corrupted ones (front and tail)
    margin loss               -> transR.py:70-83, against the mean of the negative scores

The input pipeline is Graph.sample_edge / Graph.sample_node; generate_embedding and
calculate_scores are ops.triple_score_matrix, which works on the triples grouped by relation and
never builds a matrix per triple - the torch composition (--composed) builds the [B, de * dr]
lookup and its [B, K, de * dr] tile for the same numbers.  The three tables' gradients come back
as sparse tensors over the rows / relations that were looked up, for SparseAdam.

    python examples/python/transr_minibatch.py [--kind trans_l1|trans_l2] [--composed]
        [--batch 64] [--negs 5] [--ent-dim 32] [--rel-dim 24] [--data DIR]
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


def make_tables(n_ent, n_rel, ent_dim, rel_dim, gen=None, dtype=torch.float32):
    """the model's tables as a dict of Parameters: ent [n_ent, de], rel [n_rel, dr] and
    matrix [n_rel, de * dr]"""
    shapes = (("ent", (n_ent, ent_dim)), ("rel", (n_rel, rel_dim)), ("matrix", (n_rel, ent_dim * rel_dim)))
    return {name: torch.nn.Parameter(torch.randn(shape, device="cuda", generator=gen).to(dtype))
            for name, shape in shapes}


def composed_score(tables, src, rel_id, dst, neg, kind, sparse=True):
    """generate_embedding and calculate_scores with corrupt = 'both' as the reference spells them,
    in plain torch: the lookups (sparse: with sparse gradients, as the fused op's here), one
    [de, dr] matrix per triple, its tile over the negatives, bmm, l2_normalize with the 1e-12
    clamp, the norms, the concat"""
    emb = torch.nn.functional.embedding
    b, k = neg.shape
    de, dr = tables["ent"].shape[1], tables["rel"].shape[1]

    def look(name, ids):
        return emb(ids, tables[name], sparse=sparse).float()

    def l2n(x):
        return x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=1e-12))

    def project(x, m):                                            # x [B, n, de], m [B, n, de * dr]
        n = x.shape[1]
        y = torch.bmm(x.reshape(b * n, 1, de), m.reshape(b * n, de, dr))
        return l2n(y.reshape(b, n, dr))

    def score(a, r, c):
        return -torch.linalg.vector_norm(a + r - c, ord=1 if kind == "trans_l1" else 2, dim=-1)

    m = look("matrix", rel_id.reshape(-1, 1))                     # [B, 1, de * dr]
    h, t = project(look("ent", src.reshape(-1, 1)), m), project(look("ent", dst.reshape(-1, 1)), m)
    n = project(look("ent", neg), m.repeat(1, k, 1))              # tf.tile(..., [1, num_negs, 1])
    r = l2n(look("rel", rel_id.reshape(-1, 1)))
    hh, rr, tt = h.expand(-1, k, -1), r.expand(-1, k, -1), t.expand(-1, k, -1)
    return score(h, r, t).reshape(-1), torch.cat([score(n, rr, tt), score(hh, rr, n)], -1)


def energies(tables, src, rel_id, dst, neg, kind, composed=False, sparse_grad=True):
    if composed:
        return composed_score(tables, src, rel_id, dst, neg, kind, sparse=sparse_grad)
    return ops.triple_score_matrix(tables["ent"], tables["rel"], tables["matrix"], src, rel_id, dst, neg, kind=kind,
                                   corrupt="both", sparse_grad=sparse_grad)


def margin_loss(pos, neg, margin=1.0):
    """transR.py:70-83: mean over the batch of max(margin + mean_k neg - pos, 0)"""
    return torch.clamp(margin + neg.mean(-1) - pos, min=0).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="trans_l1", choices=["trans_l1", "trans_l2"])
    ap.add_argument("--composed", action="store_true", help="the torch composition instead of ops.triple_score_matrix")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--negs", type=int, default=5)
    ap.add_argument("--ent-dim", type=int, default=32)
    ap.add_argument("--rel-dim", type=int, default=24)
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--fused-optimizer", action="store_true",
                    help="euler_amd.optim.SparseAdam - one fused kernel per table - instead of torch.optim.SparseAdam")
    ap.add_argument("--data", default=FIXTURE, help="a graph directory (euler.meta + .dat); default: the fixture graph")
    a = ap.parse_args()
    torch.manual_seed(0)
    G = euler_amd.Graph.load(a.data, edges=True)
    G.set_seed(7)
    n_ent, n_rel = G.id_range()[0] + 1, G.num_edge_types          # row = node id / edge type
    tables = make_tables(n_ent, n_rel, a.ent_dim, a.rel_dim)
    opt = (optim.SparseAdam if a.fused_optimizer else torch.optim.SparseAdam)(list(tables.values()), lr=0.01)
    src, rel_id, dst, neg = sample_batch(G, a.batch, a.negs)
    pos, scores = energies(tables, src, rel_id, dst, neg, a.kind, a.composed)
    loss = margin_loss(pos, scores, a.margin)
    opt.zero_grad()
    loss.backward()
    before = [t.detach().clone() for t in tables.values()] if a.fused_optimizer else None
    opt.step()
    if a.fused_optimizer:
        print("fused optimizer: %d rows moved, all of them looked up"
              % moved_only_looked_up_rows(list(tables.values()), before))
    rows = int(tables["ent"].grad.coalesce().indices().numel())
    mats = int(tables["matrix"].grad.coalesce().indices().numel())
    print("transr %s (%s): loss %.6f  rows updated %d of %d, matrices %d of %d"
          % (a.kind, "composed" if a.composed else "fused", float(loss), rows, n_ent, mats, n_rel))
    assert torch.isfinite(loss) and rows > 0 and mats > 0
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
