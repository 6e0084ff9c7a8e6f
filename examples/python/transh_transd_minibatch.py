#!/usr/bin/env python3
"""Knowledge-graph embedding with a projection (TransH, TransD), one optimiser step on one MI355X.

What examples/TransX/transH.py and transD.py do per batch in the reference:

    sample_edge(B)            -> (src, dst, type): the type column is the relation id
    sample_node(B * K)        -> the negatives, reshaped [B, K]
    generate_embedding        -> look up the entity and relation rows and the rows of the extra
                                 tables (TransH: the hyperplane's normal per relation; TransD: a
                                 transfer row per entity and per relation), tile the relation's
                                 rows over the K negatives, project every entity row
    calculate_scores          -> the true triple and the 2 K corrupted ones (front and tail)
    margin loss               -> transH.py:68-80

The input pipeline is Graph.sample_edge / Graph.sample_node; generate_embedding and
calculate_scores are ONE kernel, ops.triple_score_proj - the torch composition (--composed)
builds the tiled and projected [B, K, d] blocks for the same numbers.  The tables' gradients come
back as sparse tensors over the rows that were looked up, for SparseAdam.

    python examples/python/transh_transd_minibatch.py [--proj hyperplane|transfer]
        [--kind trans_l1|trans_l2] [--composed] [--batch 64] [--negs 5] [--dim 32] [--data DIR]
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


def make_tables(proj, n_ent, n_rel, dim, gen=None, dtype=torch.float32):
    """the model's tables as a dict of Parameters: ent, rel and hyper (TransH) or ent_transfer,
    rel_transfer (TransD)"""
    names = {"hyperplane": (("ent", n_ent), ("rel", n_rel), ("hyper", n_rel)),
             "transfer": (("ent", n_ent), ("rel", n_rel), ("ent_transfer", n_ent), ("rel_transfer", n_rel))}[proj]
    return {name: torch.nn.Parameter(torch.randn((rows, dim), device="cuda", generator=gen).to(dtype))
            for name, rows in names}


def composed_score(proj, tables, src, rel_id, dst, neg, kind, sparse=True):
    """generate_embedding and calculate_scores with corrupt = 'both' as the reference spells them,
    in plain torch: the lookups (sparse: with sparse gradients, as the fused op's here), the tile
    of the relation's rows over the negatives, the projection, l2_normalize, the scores, the concat"""
    emb = torch.nn.functional.embedding
    k = neg.shape[1]

    def look(name, ids):
        return emb(ids, tables[name], sparse=sparse).float()

    def l2n(x):
        return x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=1e-12))

    def score(a, r, c):
        e = a + r - c
        return -(e.abs().sum(-1) if kind == "trans_l1" else torch.linalg.vector_norm(e, dim=-1))

    rid = rel_id.reshape(-1, 1)
    if proj == "hyperplane":
        hyper = look("hyper", rid)                                # [B, 1, d]

        def project(ids, aux):
            x, w = look("ent", ids), l2n(aux)
            return x - (x * w).sum(-1, keepdim=True) * w
        aux = hyper
    else:
        aux = look("rel_transfer", rid)

        def project(ids, aux):
            x = look("ent", ids)
            return l2n(x + (x * look("ent_transfer", ids)).sum(-1, keepdim=True) * aux)
    h, t = project(src.reshape(-1, 1), aux), project(dst.reshape(-1, 1), aux)
    n = project(neg, aux.repeat(1, k, 1))                         # tf.tile(..., [1, num_negs, 1])
    r = l2n(look("rel", rid))
    hh, rr, tt = h.expand(-1, k, -1), r.expand(-1, k, -1), t.expand(-1, k, -1)
    return score(h, r, t).reshape(-1), torch.cat([score(n, rr, tt), score(hh, rr, n)], -1)


def energies(proj, tables, src, rel_id, dst, neg, kind, composed=False, sparse_grad=True):
    if composed:
        return composed_score(proj, tables, src, rel_id, dst, neg, kind)
    extra = {name: t for name, t in tables.items() if name not in ("ent", "rel")}
    return ops.triple_score_proj(tables["ent"], tables["rel"], src, rel_id, dst, neg, proj=proj, kind=kind,
                                 corrupt="both", sparse_grad=sparse_grad, **extra)


def margin_loss(pos, neg, margin=1.0):
    """transH.py:68-80: mean over the batch of max(margin + mean_k neg - pos, 0)"""
    return torch.clamp(margin + neg.mean(-1) - pos, min=0).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proj", default="hyperplane", choices=["hyperplane", "transfer"],
                    help="hyperplane: TransH; transfer: TransD")
    ap.add_argument("--kind", default="trans_l1", choices=["trans_l1", "trans_l2"])
    ap.add_argument("--composed", action="store_true", help="the torch composition instead of ops.triple_score_proj")
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
    tables = make_tables(a.proj, n_ent, n_rel, a.dim)
    opt = (optim.SparseAdam if a.fused_optimizer else torch.optim.SparseAdam)(list(tables.values()), lr=0.01)
    src, rel_id, dst, neg = sample_batch(G, a.batch, a.negs)
    pos, scores = energies(a.proj, tables, src, rel_id, dst, neg, a.kind, a.composed)
    loss = margin_loss(pos, scores, a.margin)
    opt.zero_grad()
    loss.backward()
    before = [t.detach().clone() for t in tables.values()] if a.fused_optimizer else None
    opt.step()
    if a.fused_optimizer:
        print("fused optimizer: %d rows moved, all of them looked up"
              % moved_only_looked_up_rows(list(tables.values()), before))
    rows = int(tables["ent"].grad.coalesce().indices().numel())
    print("%s %s (%s): loss %.6f  rows updated %d of %d"
          % (a.proj, a.kind, "composed" if a.composed else "fused", float(loss), rows, n_ent))
    assert torch.isfinite(loss) and rows > 0
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
