#!/usr/bin/env python3
"""Two-layer ScalableSage ("scalable GCN" training) with in-place embedding stores on one MI355X.

ScalableSageEncoder (tf_euler/python/utils/encoders.py:629-748) does not sample L hops.  It
samples ONE hop and reads the deeper layer's neighbour embeddings from a per-layer store: a
non-trainable table with a row per node that is kept in HBM across steps, plus a gradient store
of the same shape.  Per step (encoders.py:675-748):

    sample_fanout(inputs, [edge_type], [fanout])      -> node [B], neighbor [B * fanout]
    layer 0   aggregator(features(node), features(neighbor))                    -> h1
    layer 1   aggregator(h1, embedding_lookup(store, neighbor))                 -> h2, the loss
    _update_store      embedding_update(store, node, h1)
    _update_gradient   embedding_add(gradient_store, neighbor, d loss / d looked-up rows)
    _optimize_store    g = embedding_lookup(gradient_store, node), cleared afterwards;
                       store_loss = reduce_sum(h1 * g), i.e. h1.backward(gradient=g)

The three store operations are ops.embedding_update / embedding_add / embedding_take: in place,
in input order, the same bits on every run, and - through count=fanout - without the
[B * fanout, d] block of per-occurrence gradient rows.  --composed runs the same step with
index_put_ / index_add_ on materialised blocks as well, prints ms per step for both and checks on
a batch of distinct ids that the two agree: exactly for update and take, and for add within
gamma(2) * (|old| + |row|) (index_add_ promises no order; a 16-bit store adds the roundings of the
composed path, see add_bound).

The stores here are [max_id + 1, d]: the store operations leave out an id outside [0, rows), so
the default_node = max_id + 1 fills of the sampler drop out of update and add by themselves, where
the reference sizes its stores [max_id + 2, d] and spends the last row as a dump.  The buffers
below still hold one more row, which the store operations never see and which therefore stays
+0: ops.gather_segment_reduce reads an id past its table from the table's last row, and that row
makes a fill contribute nothing to the forward mean.

    python examples/python/scalable_sage_minibatch.py [--data DIR] [--nodes 2000000] [--batch 1024]
        [--fanout 10] [--dim 128] [--store-dtype {fp32,bf16}] [--steps 20] [--composed] [--time-ops]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402
from euler_amd import ops                          # noqa: E402

U32, U_STORE = 2.0 ** -24, {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


class State(object):
    """the graph, the input features, the two stores and the aggregators' weights"""

    def __init__(self, G, max_id, feat, in_dim, dim, classes, fanout, store_dtype, seed=1):
        self.G, self.max_id, self.feat, self.fanout = G, max_id, feat, fanout
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed)
        rows = max_id + 1
        # encoders.py:657-672: uniform(0, store_init_maxval) and zeros; + the row the ops never see
        self.store_buf = torch.zeros((rows + 1, dim), device="cuda", dtype=store_dtype)
        self.store_buf[:rows] = (torch.rand((rows, dim), device="cuda", generator=gen) * 0.05).to(store_dtype)
        self.grad_buf = torch.zeros((rows + 1, dim), device="cuda", dtype=store_dtype)
        self.store, self.grad_store = self.store_buf[:rows], self.grad_buf[:rows]      # what the store ops get
        w = lambda i, o: torch.nn.Parameter(torch.randn((i, o), device="cuda", generator=gen) / i ** 0.5)  # noqa: E731
        self.params = [w(in_dim, dim), w(in_dim, dim), w(dim, dim), w(dim, dim), w(dim, classes)]
        self.opt = torch.optim.Adam(self.params, lr=0.01)
        self.classes = classes


def store_ops(store, grad_store, node, neighbor, h1, leaf_grad, fanout, composed):
    """_update_store, _update_gradient and the lookup-and-clear of _optimize_store (encoders.py:713-748),
    under no_grad -> g [B, d] fp32.  leaf_grad: fused [B, d] (of the mean), composed [B * fanout, d]."""
    with torch.no_grad():
        if not composed:
            ops.embedding_update(store, node, h1)
            ops.embedding_add(grad_store, neighbor, leaf_grad / fanout, count=fanout)
            return ops.embedding_take(grad_store, node, clear=True, out_dtype=torch.float32)
        store.index_put_((node,), h1.to(store.dtype))
        grad_store.index_add_(0, neighbor, leaf_grad.to(grad_store.dtype))
        g = grad_store[node].float()
        grad_store.index_put_((node,), torch.zeros_like(g, dtype=grad_store.dtype))
        return g


def step(s, inputs, composed=False):
    """one training step, ScalableSageEncoder.call line by line (mean aggregator, concat=False)"""
    b, fanout = inputs.numel(), s.fanout
    # encoders.py:679-681
    ids = s.G.sample_fanout(inputs, [[0]], [fanout], default_node=s.max_id + 1)[0]
    node, neighbor = ids[0], ids[1]
    w_self0, w_neigh0, w_self1, w_neigh1, w_out = s.params
    # encoders.py:682, layer 0 from the features: get_dense_feature + the fused mean over the fanout
    if s.feat is None:
        x_node = s.G.get_dense_feature(node, [0], [w_self0.shape[0]])[0]
        x_neigh = ops.gather_segment_reduce("mean", s.G.get_dense_feature(neighbor, [0], [w_self0.shape[0]])[0],
                                            torch.arange(b * fanout, device="cuda", dtype=torch.int32), b, count=fanout)
    else:
        x_node = s.feat[node]
        x_neigh = ops.gather_segment_reduce("mean", s.feat, neighbor, b, count=fanout)
    h1 = torch.relu(x_node @ w_self0 + x_neigh @ w_neigh0)                  # encoders.py:692, layer 0
    # encoders.py:696-698: the neighbours' layer-1 input comes from the store, as a detached leaf
    if composed:
        rows = s.store_buf[torch.clamp(neighbor, 0, s.max_id + 1)].float().requires_grad_()
        n1 = rows.reshape(b, fanout, -1).mean(1)
    else:
        rows = ops.gather_segment_reduce("mean", s.store_buf, neighbor, b, count=fanout,
                                         out_dtype=torch.float32).detach().requires_grad_()
        n1 = rows
    h2 = torch.relu(h1 @ w_self1 + n1 @ w_neigh1)                           # encoders.py:692, layer 1
    loss = torch.nn.functional.cross_entropy(h2 @ w_out, node % s.classes)
    s.opt.zero_grad()
    loss.backward(retain_graph=True)
    live = (neighbor >= 0) & (neighbor <= s.max_id)
    nb = neighbor if not composed else torch.where(live, neighbor, torch.full_like(neighbor, s.max_id + 1))
    g = store_ops(s.store if not composed else s.store_buf, s.grad_store if not composed else s.grad_buf,
                  node, nb, h1.detach(), rows.grad, fanout, composed)
    if composed:
        s.store_buf[-1].zero_()                                             # the dump row of the composed path
        s.grad_buf[-1].zero_()
    h1.backward(gradient=g)                                                 # encoders.py:744: sum(h1 * g)
    s.opt.step()
    return loss.detach(), neighbor


def add_bound(old, row, dtype):
    """|fused - composed| of one add per element: gamma(2) * S with S = |old| + |row| for the two
    fp32 forms; a 16-bit store adds what the composed path rounds - the row to storage (u_s |row|)
    and each side's result to storage (2 u_s S (1 + u_s))"""
    s = old.double().abs() + row.double().abs()
    us = U_STORE[dtype]
    return (2 * U32 / (1 - 2 * U32)) * s + us * row.double().abs() + 2 * us * s * (1 + us)


def compare(store, grad_store, b, fanout, seed=3):
    """fused against composed store operations on DISTINCT ids (index_put_ / index_add_ are then
    well defined), from the same seeded rows; the rows touched are put back afterwards.
    -> worst |diff| / bound of add"""
    rows, d = store.shape
    assert b * fanout <= rows
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    perm = torch.randperm(rows, device="cuda", generator=gen)
    node, neighbor = perm[:b].contiguous(), perm[:b * fanout].contiguous()  # the nodes are neighbours too
    h1 = torch.randn((b, d), device="cuda", generator=gen)
    grad_mean = torch.randn((b, d), device="cuda", generator=gen)
    per_row = (grad_mean / fanout).repeat_interleave(fanout, 0)             # what autograd hands the composed path
    old_store, old_grad = store[node].clone(), grad_store[neighbor].clone()
    seeded = torch.randn((b * fanout, d), device="cuda", generator=gen).to(grad_store.dtype)
    got = {}
    with torch.no_grad():
        for composed in (False, True):
            store.index_put_((node,), old_store)
            grad_store.index_put_((neighbor,), seeded)
            if composed:
                store.index_put_((node,), h1.to(store.dtype))
                grad_store.index_add_(0, neighbor, per_row.to(grad_store.dtype))
            else:
                ops.embedding_update(store, node, h1)
                ops.embedding_add(grad_store, neighbor, grad_mean / fanout, count=fanout)
            added = grad_store[neighbor].clone()
            if composed:
                g = grad_store[node].float()
                grad_store.index_put_((node,), torch.zeros_like(g, dtype=grad_store.dtype))
            else:
                g = ops.embedding_take(grad_store, node, clear=True, out_dtype=torch.float32)
            got[composed] = (store[node].clone(), added, g, grad_store[neighbor].clone())
        store.index_put_((node,), old_store)
        grad_store.index_put_((neighbor,), old_grad)
    assert torch.equal(got[False][0], got[True][0]), "update: fused and composed differ"
    for composed in (False, True):                                          # take: the row the add left, then +0
        _, added, g, after = got[composed]
        assert torch.equal(g, added[:b].float()), "take did not return the row as it was"
        assert not bool(after[:b].any()) and torch.equal(after[b:], added[b:]), "clear touched the wrong rows"
    err = (got[False][1].double() - got[True][1].double()).abs()
    bound = add_bound(seeded, per_row, grad_store.dtype)
    assert bool((err <= bound).all()), "add: fused and composed differ by more than the bound"
    return float((err / bound.clamp(min=1e-300)).max())


def time_ops(s, b, fanout, reps=20):
    """ms of each store operation alone (device time between two events, after a warm-up)"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    inputs = torch.randint(1, s.max_id + 1, (b,), device="cuda", generator=gen)
    ids = s.G.sample_fanout(inputs, [[0]], [fanout], default_node=s.max_id + 1)[0]
    node, neighbor = ids[0], ids[1]
    d = s.store.shape[1]
    h1, gm = torch.randn((b, d), device="cuda"), torch.randn((b, d), device="cuda")
    calls = {"update": lambda: ops.embedding_update(s.store, node, h1),
             "add": lambda: ops.embedding_add(s.grad_store, neighbor, gm, count=fanout),
             "take+clear": lambda: ops.embedding_take(s.grad_store, node, clear=True)}
    out = {}
    for name, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out[name] = t0.elapsed_time(t1) / reps
    longest = int(torch.unique(neighbor, return_counts=True)[1].max())
    return out, longest


def make_state(a, store_dtype):
    if a.data:
        G = euler_amd.Graph.load(a.data)
        max_id, feat = int(G.id_range()[0]), None
        in_dim = a.in_dim
    else:
        G = euler_amd.Graph.synthetic(euler_amd.synth_params(1, a.nodes, 10 * a.nodes, weighted=True))
        max_id, in_dim = a.nodes, a.in_dim
        feat = torch.randn((max_id + 2, in_dim), device="cuda")             # row = node id
    G.set_seed(42)
    s = State(G, max_id, feat, in_dim, a.dim, a.classes, a.fanout, store_dtype)
    return s


def run(a, store_dtype, composed):
    s = make_state(a, store_dtype)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    draw = lambda: torch.randint(1, s.max_id + 1, (a.batch,), device="cuda", generator=gen)   # noqa: E731
    for _ in range(3):
        loss, neighbor = step(s, draw(), composed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss, neighbor = step(s, draw(), composed)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    assert bool(torch.isfinite(loss))
    return s, ms, float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default="", help="a graph directory (euler.meta + .dat); default: a synthetic graph")
    ap.add_argument("--nodes", type=int, default=2_000_000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--fanout", type=int, default=10)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--in-dim", type=int, default=32)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--store-dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--composed", action="store_true", help="also run the index_put_ / index_add_ step and compare")
    ap.add_argument("--time-ops", action="store_true", help="also time each store operation alone")
    a = ap.parse_args()
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[a.store_dtype]
    s, ms, loss = run(a, dt, False)
    print("fused    stores (%s): %.3f ms per step, loss %.4f  [batch %d, fanout %d, d %d, %d rows]"
          % (a.store_dtype, ms, loss, a.batch, a.fanout, a.dim, s.store.shape[0]))
    if a.time_ops:
        t, longest = time_ops(s, a.batch, a.fanout)
        print("store ops alone: " + ", ".join("%s %.3f ms" % kv for kv in t.items())
              + "; longest segment %d" % longest)
    if a.composed:
        worst = compare(s.store, s.grad_store, min(a.batch, s.store.shape[0] // a.fanout), a.fanout)
        print("fused == composed on distinct ids: update and take exactly, add within %.3f of its bound" % worst)
        del s
        torch.cuda.empty_cache()
        s, ms, loss = run(a, dt, True)
        print("composed stores (%s): %.3f ms per step, loss %.4f" % (a.store_dtype, ms, loss))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
