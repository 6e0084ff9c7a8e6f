// The fused backward of pool_aggregate (mp_pool.h) - the gradients of the meanpool / maxpool aggregators of
// the reference's SageEncoder (tf_euler/python/utils/aggregators.py:75-114) - on the matrix units of gfx950.
// This file states the contract and holds the workspace rule; the host entry, the kernels
// (pool_aggregate_backward_kernels.hip) and a host-only program can all include it.
//
// WHAT IS COMPUTED.  The forward's arguments keep their meaning.  grad [size, F] is fp32 or of the table's
// dtype.  Per position p of destination r, z[p] = table[g[p]] @ W + b and h[p] = act(z[p]) are recomputed
// by the forward's own fragment code (mp_pool_frag.h) under PoolMakePlan: the forward's K order and bias
// add, so the relu mask and the maximum are the forward's fp32 values bit for bit.
//     share[r][c] = grad[r][c]                                  add
//                   fl32(grad[r][c] * fl32(1 / len))            mean: the forward's one multiply
//                   fl32(grad[r][c] / ties)                     max: ties = the positions of the segment with
//                                                               h[p][c] == m[r][c], m the fold's fp32 maximum
//     dZ[p][c]    = share[r][c] where the position takes part (max: h[p][c] == m[r][c]) and z[p][c] > 0
//                   (act none: the second condition is dropped), else +0
// The max rule is the even split among maximal positions of TF's reduce_max and torch's amax.  dZ is narrowed
// ONCE to the table's dtype (exact when grad has it and op is add; fp32 stays) and is an MFMA operand from
// then on.  A position outside every segment has a dZ row of +0.
//     d_bias = sum_p dZ[p]      d_weight = sum_p X[p]^T dZ[p]      dX[p] = dZ[p] W^T
// X[p] = table[g[p]], a row of +0 for an index outside the table (RANGE RULE): such a position adds nothing
// to d_weight, its dZ still counts in d_bias, and its table gradient is dropped - d_table is the grouped
// in-place add of embed_store.h in its plain form (ids = g or p, values = dX, m = e) on a zeroed table:
// occurrences in increasing p in fp32, one rounding.
// ARITHMETIC.  Every product accumulates in fp32 on the matrix units in an order fixed by the shapes alone:
//   dX: over f in the K chunks of 32 in increasing f;
//   d_weight, d_bias: the POSITIONS are cut into slabs by DenseBwdSlabRows(e) (mp_dense_backward.h); a slab
//     is accumulated in steps of 32 positions in increasing p (d_bias as the products of a row of ones with
//     dZ, in the same steps) into an fp32 partial; the partials are added in increasing slab from +0, one
//     rounding per add, then one rounding to the parameter's dtype (d_bias: the bias's).
// No float atomics, no host wait (seg_ptr is read on the device only), the same bits on every run, on every
// stream and for count or the equivalent seg_ptr.
// NaN.  The fold takes NaN as greatest, as the forward does; `h == m` is false for a NaN, so a (segment,
// column) whose maximum is NaN has ties = 1 and a dZ of +0 at every position.  `z > 0` is false for a NaN: the
// relu mask is 0 there.  With act none and op add / mean no z is looked at and dZ is the share whatever the
// table holds.  A NaN in grad reaches the share and every gradient it is multiplied into.
// LIMITS.  Those of the forward, and 1 <= d <= kPoolBwdMaxK, 1 <= F <= kPoolBwdMaxF: every forward plan in
// that range has k_tiles == 1 (no lockstep K tiling), and kernels 3 and 4 stage as in mp_dense_backward.h.
// WORKSPACES, caller-allocated: dz_ws [e, F] of the table's dtype, 16-byte aligned (every row is written);
// for max, m_ws and share_ws, fp32 [size, F]; partial_ws, fp32, PoolBwdWorkspaceFloats(e, d, F) (with
// d_weight or d_bias); d_rows [e, d] fp32 is dX, asked for only when the table wants a gradient.
//
// THE KERNELS (all cap their grid and loop beyond the cap).
// 1. PoolBwdWalkKernel<.., false>, op max only: the forward's tiling and fold - a wave owns runs of 16
//    destinations, walks tiles of 16 gathered rows, W^T in LDS - with a tie counter next to the running
//    maximum; where the forward stores a destination it stores m and share = grad / ties in fp32.
// 2. PoolBwdWalkKernel<.., true>: the same recompute once more; the staging walk, lane l down column l in
//    increasing p, turns z into dZ - compare with m, mask, select the share (mean / add: the share comes
//    from grad and the boundary values) - and stores the row in the table's dtype, 64 columns of a row per
//    wave store.  That row layout is the A-operand layout of kernel 3 and the Y layout of kernel 4: the
//    accumulator-to-operand turn goes through memory.  With act none and op add / mean no z is needed: the
//    MFMA stage, the table reads and the staging of W are skipped.
//    PoolBwdEdgesKernel (seg_ptr only) writes +0 to the rows before the first and after the last boundary.
// 3. DenseBwdRowsKernel (mp_dense_backward_frag.h) over the e rows of dZ, every denominator 1.
// 4. DenseBwdWeightKernel<.., GATHER> over positions, its X rows gathered through g, then DenseBwdSumKernel.
#pragma once

#include <stdint.h>

#include "mp_dense_backward.h"
#include "mp_pool.h"

namespace euler_gpu {

constexpr int kPoolBwdMaxK = kDenseBwdMaxK;  // d
constexpr int kPoolBwdMaxF = kDenseBwdMaxF;  // F

// slabs of positions of the weight kernel: the dense rule applied to e (0 for e == 0)
inline int64_t PoolBwdSlabs(int64_t e) { return DenseBwdSlabs(e); }

// fp32 elements of partial_ws: the weight partials, the bias rows after them
inline int64_t PoolBwdWorkspaceFloats(int64_t e, int64_t d, int64_t f) { return PoolBwdSlabs(e) * (d * f + f); }

}  // namespace euler_gpu
