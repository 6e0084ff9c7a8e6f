#!/usr/bin/env python3
"""Supervised GraphSAGE training steps, end to end on one MI355X.

What the reference's SuperviseModel (tf_euler/python/mp_utils/base.py:24-47) does per step for
examples/graphsage:

    SageDataFlow              -> Graph.sage_blocks: the sampled blocks of every hop, one enqueue
    get_dense_feature         -> the input features of the outermost layer
    SAGEConv per block        -> gather_segment_reduce("mean") over the block's fanout + two matmuls
    out_fc                    -> one matmul, logits [B, label_dim]
    get_dense_feature         -> the labels, a [B, label_dim] block
    sigmoid, sigmoid_cross_entropy_with_logits, reduce_mean, floor(p + 0.5), the masked sums of
    tf.metrics.true_positives / false_positives / false_negatives, a host read for the f1

Everything below out_fc is ONE op here, Graph.supervise_loss: the labels are read straight from
the graph's feature table, the loss comes back as a 0-d tensor and a metrics.Streaming("f1")
object collects tp / fp / fn on the device.  --composed trains through the plain-torch head
instead: the label fetch, binary_cross_entropy_with_logits and the masked sums.  Either way
every step runs BOTH heads on the same logits and asserts that they agree: the integer counts
exactly, the loss within the bound derived in DESIGN 4.23 on both sides of the float64 value.

    python examples/python/graphsage_train.py [--data DIR] [--batch 64] [--steps 20] [--composed]

--data: a directory written by euler/tools (euler.meta + Node/*.dat; float feature --feature-fid
= the input features, --label-fid = the labels); default: the fixture graph of tests/golden, whose
float slot 1 holds values above 1 - soft labels, so its loss has no floor and falls below zero.
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from euler_amd import euler_ops, metrics, ops      # noqa: E402
from euler_amd.dataflow import SageDataFlow        # noqa: E402

U = 2.0 ** -24
E_SP = 2.7970                                      # ulps of the fp32 softplus, measured
SP_BELOW = math.log1p(math.exp(-86.0))
REL_TERM = (1 + E_SP * 2 * U) * (1 + U) - 1


def make_model(in_dim, hidden, label_dim, layers=2, seed=0):
    """per layer (w_self, w_neigh), then out_fc (no bias, base.py:30)"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    dims = [in_dim] + [hidden] * layers
    make = lambda i, o: torch.nn.Parameter(torch.randn((i, o), generator=gen, device="cuda") * i ** -0.5)   # noqa: E731
    return [make(dims[k // 2], dims[k // 2 + 1]) for k in range(2 * layers)] + [make(hidden, label_dim)]


def logits_of(G, flow, params, src, feature_fid, in_dim, fanouts):
    """the blocks of src -> logits [B, label_dim]"""
    df = flow(src)                                   # blocks from the outermost hop inwards
    x = G.get_dense_feature(df[0].n_id, [feature_fid], [in_dim], out_dtype=torch.float32)[0]
    for k, blk in enumerate(df):                     # (no self loops: `count` sampled edges per destination)
        fanout = fanouts[len(fanouts) - 1 - k]
        neigh = ops.gather_segment_reduce("mean", x, blk.edge_index[1].to(torch.int32), blk.size[0], count=fanout)
        x = torch.relu(x[blk.res_n_id] @ params[2 * k] + neigh @ params[2 * k + 1])
    return x @ params[-1]


def fused_head(G, src, logits, label_fid, label_dim, metric):
    return G.supervise_loss(src, logits, label_fid, label_dim, metric=metric)


def composed_head(G, src, logits, label_fid, label_dim):
    """SuperviseModel.__call__ after out_fc in plain torch -> (loss, int64 [tp, fp, fn, correct, total])"""
    label = G.get_dense_feature(src, [label_fid], [label_dim], out_dtype=torch.float32)[0]
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, label)
    with torch.no_grad():
        pred = torch.floor(torch.sigmoid(logits) + 0.5)
        lab, prd = label != 0, pred != 0
        counts = torch.stack([(lab & prd).sum(), (~lab & prd).sum(), (lab & ~prd).sum(), (label == pred).sum(),
                              torch.tensor(label.numel(), device=label.device)])
    return loss, counts


def loss64_and_bound(logits, label):
    """the float64 loss of the same fp32 logits and the bound of the fused fp32 loss's error
    (the softplus' measured ulps, half an ulp each for the product and the add of a
    soft label, C - 1 + ceil(B / 256) + 8 additions, the count and the division)"""
    x, z = logits.detach().double(), label.double()
    b, c = x.shape
    a = torch.clamp(x, min=0) - x * z
    big_l = torch.log1p(torch.exp(-x.abs()))
    soft = (z != 0) & (z != 1)
    da = torch.where(soft, U * (x * z).abs() * (1 + U) + U * a.abs(), torch.zeros_like(a))
    err = da + REL_TERM * (a.abs() + da + big_l) + SP_BELOW
    n = c + -(-b // 256) + 9
    gam = n * U / (1 - n * U)
    return float((a + big_l).sum() / (b * c)), float((err.sum() + gam * (a.abs() + big_l + err).sum()) / (b * c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=os.path.join(ROOT, "tests", "golden", "fixture_dat"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--fanouts", type=int, nargs=2, default=[3, 2])
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--feature-fid", type=int, default=0)
    ap.add_argument("--feature-dim", type=int, default=2)
    ap.add_argument("--label-fid", type=int, default=1)
    ap.add_argument("--label-dim", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--composed", action="store_true", help="train through the plain-torch head")
    a = ap.parse_args()
    euler_ops.initialize_graph({"mode": "local", "data_path": a.data})            # euler_ops/base.py
    G = euler_ops.get_default_graph()
    max_id = int(G.id_range()[0])
    G.set_seed(42)
    flow = SageDataFlow(G, a.fanouts, [[0], [0]], add_self_loops=False, max_id=max_id)
    params = make_model(a.feature_dim, a.hidden, a.label_dim)
    opt = torch.optim.Adam(params, lr=a.lr)
    f1 = metrics.get("f1")()
    mode = "composed" if a.composed else "fused"
    totals = torch.zeros(5, dtype=torch.int64, device="cuda")
    first = last = None
    for step in range(a.steps):
        src = euler_ops.sample_node(a.batch, 0)
        logits = logits_of(G, flow, params, src, a.feature_fid, a.feature_dim, a.fanouts)
        before = f1.counts.clone() if f1.counts is not None else torch.zeros_like(totals)
        if a.composed:
            loss, counts = composed_head(G, src, logits, a.label_fid, a.label_dim)
            with torch.no_grad():
                other = fused_head(G, src, logits, a.label_fid, a.label_dim, f1)
        else:
            loss = fused_head(G, src, logits, a.label_fid, a.label_dim, f1)
            with torch.no_grad():
                other, counts = composed_head(G, src, logits, a.label_fid, a.label_dim)
        opt.zero_grad()
        loss.backward()
        opt.step()
        # the two heads on the same logits: the counts exactly, the loss within the bound
        fused, comp = (float(other), float(loss.detach())) if a.composed else (float(loss.detach()), float(other))
        label = G.get_dense_feature(src, [a.label_fid], [a.label_dim], out_dtype=torch.float32)[0]
        loss64, bound = loss64_and_bound(logits, label)
        assert torch.equal(f1.counts - before, counts), (step, (f1.counts - before).tolist(), counts.tolist())
        assert abs(fused - loss64) <= bound and abs(fused - comp) <= 2 * bound, (step, fused, comp, loss64, bound)
        totals += counts
        assert torch.equal(totals, f1.counts)                                      # streaming: the sum over the steps
        value = float(loss.detach())
        first, last = (value if first is None else first), value
        print("step %d (%s): loss %.6f  f1 %.4f  |fused - composed| %.3g (bound %.3g)"
              % (step, mode, value, float(f1.value()), abs(fused - comp), 2 * bound))
        assert math.isfinite(value)
    torch.cuda.synchronize()
    if a.steps > 1:
        assert last < first, "the loss did not fall: %.6f -> %.6f" % (first, last)


if __name__ == "__main__":
    main()
