#!/usr/bin/env python3
"""The layer-0 aggregation of a sampled block over the input features stored in 8 bits.

The input feature table of a GNN is constant and the largest thing gathered, and its rows need
no gradient, so it can be stored as OCP e4m3fn codes with one fp32 scale per column
(ops.Fp8Rows): a quarter of the fp32 bytes per gathered row, half of the bf16 ones.

    T8 = G.fp8_dense_feature(0, dim)                   # id-indexed, two chunked passes, once
    nbrs, _, _ = G.sample_fanout(roots, [[0]], [count], default_node=-1)
    agg = ops.gather_segment_reduce("mean", T8, nbrs[1], roots.numel(), count=count)   # ids read in place

runs beside the same block mean over the fp32 and the bf16 table.  The contract is exact - the
fp8 op has the bits of the fp32 op on T8.dequantize() - and is asserted here; what the 8 bits cost
is the quantisation of the table itself, printed as the relative error of the aggregate against
the fp32 table's.

    python examples/python/fp8_features_minibatch.py [--nodes 20000] [--dim 128] [--batch 512] [--count 10]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402
from euler_amd import ops                          # noqa: E402


def feature_graph(n, dim, seed):
    """n nodes (ids 1 .. n) with eight random neighbours of weight 1 each and a dim-d feature slot
    whose columns have different magnitudes"""
    rng = np.random.default_rng(seed)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    deg = 8
    nbr = rng.integers(1, n + 1, n * deg).astype(np.uint64)
    w = np.tile(np.arange(1, deg + 1, dtype=np.float32), n)          # prefix weights of a row
    val = (rng.standard_normal((n, dim)) * np.exp2(rng.integers(-4, 5, dim))).astype(np.float32)
    feats = (1, np.arange(n + 1, dtype=np.int64) * dim, np.full(n, dim, np.int32), val.reshape(-1))
    return euler_amd.Graph.from_csr(ids, np.arange(n + 1, dtype=np.int64) * deg, np.full(n, deg, np.int32), nbr, w,
                                    np.full(n, float(deg), np.float32), 1, features=feats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--count", type=int, default=10)
    a = ap.parse_args()
    G = feature_graph(a.nodes, a.dim, 1)
    G.set_seed(42)
    max_id = int(G.id_range()[0])
    all_ids = torch.arange(max_id + 1, dtype=torch.int64, device="cuda")
    T32 = G.get_dense_feature(all_ids, [0], [a.dim])[0]             # id-indexed fp32 table
    T16 = T32.to(torch.bfloat16)
    T8 = G.fp8_dense_feature(0, a.dim, chunk_rows=4096)
    assert tuple(T8.shape) == tuple(T32.shape) and T8.q.dtype == torch.uint8

    roots = torch.randint(1, a.nodes + 1, (a.batch,), dtype=torch.int64, device="cuda")
    nbrs, _, _ = G.sample_fanout(roots, [[0]], [a.count], default_node=-1)
    n = roots.numel()
    agg32 = ops.gather_segment_reduce("mean", T32, nbrs[1], n, count=a.count)
    agg16 = ops.gather_segment_reduce("mean", T16, nbrs[1], n, count=a.count, out_dtype=torch.float32)
    agg8 = ops.gather_segment_reduce("mean", T8, nbrs[1], n, count=a.count)
    # the bit contract: the fp32 op on the dequantised table
    want = ops.gather_segment_reduce("mean", T8.dequantize(), nbrs[1], n, count=a.count)
    assert torch.equal(agg8.view(torch.int32), want.view(torch.int32)), "the fp8 op is not the fp32 op on dequantize()"
    agg8_16 = ops.gather_segment_reduce("mean", T8, nbrs[1], n, count=a.count, out_dtype=torch.bfloat16)
    assert torch.equal(agg8_16.view(torch.int16), want.to(torch.bfloat16).view(torch.int16))
    torch.cuda.synchronize()

    def rel(x):
        return float((x - agg32).norm() / agg32.norm())
    print("block mean of %d roots x %d neighbours, D = %d: bytes per gathered row fp32 %d / bf16 %d / fp8 %d"
          % (n, a.count, a.dim, a.dim * 4, a.dim * 2, a.dim))
    print("relative error of the aggregate against the fp32 table: bf16 %.3e, fp8 %.3e (bit contract holds)"
          % (rel(agg16), rel(agg8)))


if __name__ == "__main__":
    main()
