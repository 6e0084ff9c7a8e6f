#!/usr/bin/env python3
"""DeepWalk / node2vec / LINE training steps, end to end on one MI355X.

What the reference's unsupervised solution (tf_euler/python/solution/base_unsupervise.py) does per
step for examples/deepwalk and examples/line:

    to_sample                 -> (src, pos, negs): random_walk -> gen_pair -> sample_node
                                 (deepwalk_minibatch.py next to this file, unchanged)
    target / context lookup   -> three embedding lookups over [N, 1 + K, d] blocks
    PosNegLogits              -> two batched matmuls (solution/logits.py:30-34)
    xent_loss                 -> sigmoid cross-entropy, one mean (solution/losses.py:27-33)
    mrr_score                 -> two top_k sorts (utils/metrics.py:51-61)

Everything below to_sample is ONE op here, ops.skipgram_loss: 1 + P + K table rows read per pair
row, the loss and the rank of the positive written, the tables' gradients returned as sparse
tensors over the rows that were looked up, for SparseAdam.  --composed runs the lookup + bmm +
softplus formulation in plain torch instead, for comparison.  The two tables are
[max_id + 2, dim]: random_walk fills a walk that cannot go on with default_node = max_id + 1,
which has a row of its own as in the reference.  --order 1 shares one table between target and
context (LINE's first order, examples/line/line.py:52-53).  --fused-optimizer steps with
euler_amd.optim.SparseAdam (one fused call per table) instead of torch.optim.SparseAdam.

    python examples/python/deepwalk_train.py [--data DIR] [--batch 1024] [--steps 20] [--dim 128]
                                             [--composed] [--order 1|2] [--fused-optimizer]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import euler_amd                                   # noqa: E402
from euler_amd import euler_ops, ops, optim        # noqa: E402
from deepwalk_minibatch import to_sample           # noqa: E402
from fused_optimizer_check import moved_only_looked_up_rows          # noqa: E402


def composed_loss(target, context, src, pos, negs):
    """UnsuperviseSolution.__call__ (base_unsupervise.py:63-73) in plain torch: the three lookups
    (sparse gradients, as the fused op's), PosNegLogits' two matmuls, xent_loss, and the rank of
    mrr_score by its two sorts.  -> (loss, rank [N] int64, logits [N, P + K])"""
    emb = torch.nn.functional.embedding
    e = emb(src.reshape(-1, 1), target, sparse=True).float()                # [N, 1, d]
    e_pos = emb(pos, context, sparse=True).float()                          # [N, P, d]
    e_negs = emb(negs, context, sparse=True).float()                        # [N, K, d]
    logits = torch.matmul(e, e_pos.transpose(1, 2))                         # [N, 1, P]
    neg_logits = torch.matmul(e, e_negs.transpose(1, 2))                    # [N, 1, K]
    true_xent = torch.nn.functional.softplus(-logits)                       # labels = 1
    negative_xent = torch.nn.functional.softplus(neg_logits)                # labels = 0
    loss = torch.cat([true_xent.reshape(-1), negative_xent.reshape(-1)]).mean()
    with torch.no_grad():
        all_logits = torch.cat([neg_logits, logits], 2)
        order = torch.sort(all_logits, dim=2, descending=True, stable=True).indices     # top_k(all, size)
        ranks = torch.sort(order, dim=2, stable=True).indices                            # top_k(-indices, size)
        rank = ranks[:, 0, -1]
    return loss, rank, torch.cat([logits, neg_logits], 2).reshape(src.numel(), -1).detach()


def loss_of(target, context, src, pos, negs, composed=False):
    """-> (loss, rank, logits) of one minibatch, by the fused op or by the composition"""
    if composed:
        return composed_loss(target, context, src, pos, negs)
    return ops.skipgram_loss(target, context, src, pos, negs, sparse_grad=True, return_logits=True)


def make_tables(max_id, dim, order=2, dtype=torch.float32, seed=0):
    """target and context [max_id + 2, dim]; order 1: one table for both (LINE's first order)"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    make = lambda: torch.nn.Parameter(                                      # noqa: E731
        (torch.randn((max_id + 2, dim), generator=gen, device="cuda") * dim ** -0.5).to(dtype))
    target = make()
    return target, (target if order == 1 else make())


def sample_step(batch, max_id, walk_len=3, num_negs=5, p=1.0, q=1.0):
    inputs = euler_ops.sample_node(batch, 0)                   # the source nodes of the step
    return to_sample(inputs, 0, [0], max_id, walk_len, p, q, 1, 1, num_negs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default="")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--walk-len", type=int, default=3)          # run_deepwalk.py:34
    ap.add_argument("--num-negs", type=int, default=5)          # run_deepwalk.py:39
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--order", type=int, default=2, choices=[1, 2])
    ap.add_argument("--composed", action="store_true", help="the torch composition instead of ops.skipgram_loss")
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--fused-optimizer", action="store_true",
                    help="euler_amd.optim.SparseAdam - one fused kernel per table - instead of torch.optim.SparseAdam")
    a = ap.parse_args()
    if a.data:
        euler_ops.initialize_graph({"mode": "local", "data_path": a.data})       # euler_ops/base.py
        G = euler_ops.get_default_graph()
        max_id = int(G.id_range()[0])
    else:
        G = euler_amd.Graph.synthetic(euler_amd.synth_params(1, a.nodes, 10 * a.nodes, weighted=True))
        G.set_node_sampler()                       # unit weights, one node type, row order
        euler_ops.set_default_graph(G)
        max_id = a.nodes
    G.set_seed(42)
    target, context = make_tables(max_id, a.dim, a.order)
    params = [target] if context is target else [target, context]
    opt = (optim.SparseAdam if a.fused_optimizer else torch.optim.SparseAdam)(params, lr=a.lr)
    mode = "composed" if a.composed else "fused"
    for step in range(a.steps):
        src, pos, negs = sample_step(a.batch, max_id, a.walk_len, a.num_negs)
        loss, rank, _ = loss_of(target, context, src, pos, negs, a.composed)
        opt.zero_grad()
        loss.backward()
        before = [p.detach().clone() for p in params] if a.fused_optimizer and step == 0 else None
        opt.step()
        if before is not None:
            print("fused optimizer: %d rows moved, all of them looked up" % moved_only_looked_up_rows(params, before))
        print("step %d (%s, order %d): loss %.6f  mrr %.4f  pairs %d"
              % (step, mode, a.order, float(loss), float(ops.rank_metric("mrr", rank)), src.numel()))
        assert torch.isfinite(loss)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
