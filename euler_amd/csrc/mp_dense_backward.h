// The fused backward of aggregate_dense (mp_dense.h) - the gradients of the mean aggregator family
// of the reference: MeanAggregator / GCNAggregator (tf_euler/python/utils/aggregators.py:25-72),
// SAGEConv / GraphConv and GINConv - on the matrix units of gfx950.  This file states the contract and
// holds the plans; the host entry, the kernels (aggregate_dense_backward_kernels.hip) and a host-only
// program can all include it.
//
// WHAT IS COMPUTED.  The forward's arguments keep their meaning.  grad [size, cols] (cols = F, or
// Fs + F for concat) is fp32 or of the table's dtype.  Per destination r, A[r], Zn = A W + b and
// Zs = root Ws as the forward forms them; Gn, Gs the halves of grad (both all of it for add, the
// column ranges [Fs, Fs + F) and [0, Fs) for concat):
//     dZn = Gn where Zn > 0, else +0 (act none: Gn)          dZs likewise from Zs
//     d_bias = sum_r dZn[r]      d_weight = A^T dZn          d_root_weight = root^T dZs
//     dA = dZn W^T               dA'[r] = dA[r] / den[r]     (mean: DenseDenominator; add: 1)
//     d_root = dZs Ws^T (add, concat)  |  root_scale dA' (fold; no scale: dA')
//     d_table[g[p]] += dA'[dst(p)]  for every p whose index is inside the table (RANGE RULE)
// The last line is the grouped in-place add of embed_store.h over d_agg = dA' (fp32 [size, d]), which
// the entry writes: occurrences in increasing p in fp32, one rounding.
//
// ARITHMETIC.  A and both Z are recomputed by the forward's own fragment code (mp_dense_frag.h) under
// the forward's plan: the fold, the division, the one narrowing and the K order are the forward's, so
// the mask is the forward's bit for bit.  The derivative at Z == 0 and at NaN is 0 (z > 0 ? 1 : 0).
// dZ is narrowed once to the table's dtype (exact when grad has it; fp32 stays) and is an MFMA operand
// from then on.  Every product accumulates in fp32 on the matrix units in an order fixed by the
// shapes alone:
//   dA, d_root:  over f in the K chunks of 32 in increasing f, as the forward runs over k;
//   d_weight, d_root_weight, d_bias:  size is cut into SLABS by DenseBwdSlabRows(size); a slab is
//     accumulated in steps of 32 destinations in increasing r (d_bias as the products of a row of ones
//     with dZn, in the same steps) into an fp32 partial; the partials are added in increasing slab
//     from +0, one rounding per add.
// The division by den is one correctly rounded fp32 division, the multiply by root_scale one rounded
// fp32 multiply; each gradient is rounded once to its parameter's dtype (d_bias: the bias's).
// No float atomics, no host wait (seg_ptr is read on the device only), the same bits on every run, on
// every stream and for count or the equivalent seg_ptr.
// LIMITS.  Those of the forward, and 1 <= d, ds <= kDenseBwdMaxK, 1 <= F, Fs <= kDenseBwdMaxF: within
// them every W of every kernel is staged once per pass (no lockstep K tiling) in the 64 KB of mp_dense.h.
//
// THE KERNELS (all cap their grid and loop beyond the cap).
// 1. DenseBwdZKernel, destination-major: the forward's tiling, fold and MFMA stage, W^T in LDS, two
//    accumulator sets.  Its epilogue reads grad in the accumulator layout, applies the masks and stores
//    dZn [size, F] and dZs [size, Fs] in the table's dtype; on its first F pass it also stores the
//    narrowed A [size, d] straight from the A fragments (16 bytes per lane and chunk where d % 8 == 0).
//    act none needs no Z: the MFMA stage and the staging of W are skipped.
// 2. DenseBwdRowsKernel, destination-major, once per path: out[r] = X[r] W^T with X = dZ.  The A
//    fragment of 16 destinations x 32 f is a 16-byte load of a dZ row - the layout kernel 1 stored is the
//    operand layout, so the accumulator-to-operand turn costs no LDS: dZ has to reach memory for kernel 3
//    anyway and is read back from L2.  B is W in its NATURAL [k][f] layout, f contiguous: column k of
//    the fragment is a row of W, staged in LDS with the forward's column stride and swizzle (the plan
//    is DenseMakePlan with the roles of K and F exchanged).  The accumulators hold 16 NT columns of d;
//    more d are further passes.  Epilogue: the division (den from the lane's own four destinations),
//    d_agg in fp32, d_root in the table's dtype.
// 3. DenseBwdWeightKernel, once per path: out[k][f] = sum_r X[r][k] Y[r][f], X = A | root, Y = dZ.
//    A workgroup of 4 waves owns a (slab, 64 k, 64 f) job; wave w owns k fragment w and four f
//    fragments.  Per step of 32 destinations the workgroup loads 32 x 64 of X and of Y (16-byte loads
//    where the row stride allows) and writes them TRANSPOSED into LDS - T[column][r], r contiguous,
//    stride 32 elements + 16 bytes - so both operand fragments are 16-byte LDS reads of 8 consecutive
//    r; the next step's loads are issued before the MFMAs of this one.  LDS: 10 KB (fp32 18 KB).
//    The partial goes to the fp32 workspace; DenseBwdSumKernel adds the slabs and rounds once.
#pragma once

#include <stdint.h>

#include "mp_dense.h"

namespace euler_gpu {

constexpr int kDenseBwdMaxK = 256;           // d, ds: kernel 1 in fp32 still stages 32 columns of both paths at once
constexpr int kDenseBwdMaxF = 512;           // F, Fs: kernel 2 in fp32 stages 32 rows of W, 512 f each, in the 64 KB
constexpr int kDenseBwdTile = 64;            // k and f of a weight-kernel job
constexpr int kDenseBwdStep = 32;            // destinations per step of the weight kernel
constexpr int kDenseBwdMinSlabRows = 1024;
constexpr int kDenseBwdMaxSlabs = 256;
constexpr int kDenseBwdMaxBlocks = 512;      // of the weight kernel

// destinations per slab of the weight kernel: a multiple of 32, from `size` alone
inline int64_t DenseBwdSlabRows(int64_t size) {
  int64_t rows = (size + kDenseBwdMaxSlabs - 1) / kDenseBwdMaxSlabs;
  rows = (rows + kDenseBwdStep - 1) / kDenseBwdStep * kDenseBwdStep;
  return rows < kDenseBwdMinSlabRows ? kDenseBwdMinSlabRows : rows;
}

inline int64_t DenseBwdSlabs(int64_t size) {
  const int64_t rows = DenseBwdSlabRows(size);
  return (size + rows - 1) / rows;
}

// fp32 elements of the workspace: the partials of one path at a time, the bias row after the weight's
inline int64_t DenseBwdWorkspaceFloats(int64_t size, int64_t d, int64_t f, int64_t ds, int64_t fs) {
  const int64_t n = d * f + f, s = ds * fs;
  return DenseBwdSlabs(size) * (n > s ? n : s);
}

// bytes between the columns of a transposed tile of the weight kernel
inline int32_t DenseBwdTileStride(bool f32) { return kDenseBwdStep * (f32 ? 4 : 2) + 16; }

// the plan of DenseBwdRowsKernel over a W [n_cols, k_all]: the forward's, K and F exchanged
inline DensePlan DenseBwdRowsPlan(int64_t k_all, int64_t n_cols, bool f32) { return DenseMakePlan(k_all, 0, n_cols, f32); }

}  // namespace euler_gpu
