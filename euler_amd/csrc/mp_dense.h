// Fused mean-aggregator layer - reduce, THEN dense - the default aggregator family of the
// reference: MeanAggregator (tf_euler/python/utils/aggregators.py:38-72), GCNAggregator
// (aggregators.py:25-35), SAGEConv / GraphConv (convolution/sage_conv.py) and GINConv
// (convolution/gin_conv.py).  With A[r] the aggregate of destination r,
//
//     A[r]   = reduce_{p in segment(r)} table[g[p]]                          reduce = add | mean
//     out[r] = act(A[r] @ W + b)                                             root == none
//            = act(A[r] @ W + b) + act(root[r] @ Ws)                         combine add
//            = [ act(root[r] @ Ws) , act(A[r] @ W + b) ]                     combine concat
//            = act(A'[r] @ W + b),  A' = reduce over (s * root[r], rows...)  combine fold
//
// in one pass on the matrix units: the aggregate never leaves registers, and neither the [size, d]
// aggregate nor the [size, F] results of the two paths are written.  This file states the
// contract and holds the tile plan; the host entry, the kernel (aggregate_dense_kernels.hip) and a
// host-only program can all include it.
//
// ARGUMENTS.  table [rows, d] and weight [d, F] (a TF Dense kernel's layout), contiguous, one dtype
// of fp32 / bf16 / fp16.  bias [F], fp32 or the table's dtype, widened exactly; none = +0.  root
// [size, ds] and root_weight [ds, Fs] of the table's dtype; Fs == F for add; fold has no
// root_weight and ds == d.  op: mean or add.  act: relu or none.
// SEGMENTS AND INDICES are those of mp_pool.h: seg_ptr (int64 [size + 1]) or count with e == size
// * count, exactly one; g[p] an int32 index, a signed int64 id compared in 64 bits, or p itself.
// RANGE RULE: an index outside [0, rows) names no row, is never dereferenced and reads as a row
// of +0; it still counts in the segment's length.  Its table gradient is dropped.  A destination's
// boundaries are kept inside [0, e] and its end at or after its begin (TkSegment), so a malformed
// seg_ptr reads and writes nothing out of bounds; what is reduced then is unspecified.
// ARITHMETIC.  The fold starts at +0 and adds the widened rows in increasing p in fp32, one
// rounding per add (fold mode: the root term first - root[r] as it is, or one fp32 multiply by
// root_scale).  mean then divides by fl(len + 1e-7f), len + 1 in fold mode: the denominator and
// the correctly rounded division of gather_segment_reduce, NOT a multiply by a reciprocal, so that
// A has the bits that op stores today (x / 3 and x * fl(1 / 3) differ).  A is then rounded ONCE to
// the table's dtype (fp32: kept).  Products of the stored values are accumulated in fp32 by the
// matrix instructions in an order that depends only on d (and ds): the K chunks of 32 in
// increasing k, a zero-filled tail adding +0 - never on where the row sits in a tile, a wave, a
// workgroup or the grid.  Bias and activation (relu: x > 0 ? x : +0, NaN stays) are applied in
// fp32 per path, the paths are combined in fp32, and the result is rounded once to the output
// dtype (fp32 or the table's).  An empty segment has A = +0.
// DETERMINISM.  The same bits on every run, on every stream, and for count or the equivalent
// seg_ptr: a lane sees only its own destination's [begin, end).
// LIMITS.  e, size < 2^31; 1 <= d, ds <= 1024; 1 <= F, Fs <= 4096; rows >= 1.  size == 0 touches
// nothing.
//
// THE TILING (DensePlan below is its one statement).
// A workgroup is 4 waves; a wave owns RUNS of 16 consecutive destinations: the M of the matrix
// instruction is 16 DESTINATIONS.  Lane l owns destination l % 16 and, per K chunk of 32, the 8
// consecutive k from 8 * (l / 16): the A operand of v_mfma_f32_16x16x32_{bf16,f16} (fp32: the
// eight v_mfma_f32_16x16x4_f32 of mp_pool.h, the same fixed permutation of k in A and B).
// THE FOLD.  K is folded in tiles of 128 elements = 4 chunks = 32 fp32 registers.  The lane walks
// its own segment in increasing p; per position and chunk it loads 16 bytes of the gathered row
// (fp32: 2 x 16; element loads when the table or root is off a 16-byte boundary or d % 8 != 0,
// fp32 % 4; nothing is read past a row), the loads of 4 positions (fp32: 2) issued before the
// first add.  The trip count is the run's longest segment - the scalar `count` in the count form
// - predicated per lane.  For d > 128 the positions are walked once per fold tile; every byte of
// a row is still read once.  After the last position: the division, the narrowing, and the 32
// registers ARE the A fragments of 4 chunks.  No LDS, no cross-lane traffic.
// THE SELF PATH loads its A fragments straight from root rows in the same layout; fold mode
// seeds the fold with them.
// ACCUMULATORS.  N is 16 columns; a wave keeps NT fragments (1, 2, 4, 8) PER PATH: two
// accumulator sets, so that act() of the neighbour path and of the self path are both formed in
// the epilogue.  That costs 32 registers at NT = 8 and nothing in NT.  The accumulator of lane l
// holds rows 4 * (l / 16) + i of column l % 16; bias, activation, combine and store work from
// that layout: no LDS, no atomics.
// W IN LDS.  Both paths' W^T for the F tile are staged k-contiguous, Wt[c][k], in 16-byte units.
// Where a column's K extent is a multiple of 256 bytes the columns are packed (stride = extent)
// and unit u of column c sits at unit u ^ (c % 16): the 16 columns of a quarter wave then fall
// on distinct banks without padding - d = ds = F = 128 in 16 bits is exactly 64 KB and ONE pass.
// Otherwise the stride is the extent + 16 bytes, as in mp_pool.h.  Columns >= F and k >= d are +0.
// LDS BUDGET: 64 KB, all of it W.  gfx950 has 160 KB per CU: 2 workgroups (8 waves) per CU at
// the full budget.
// F TILING: NT is the largest of 8 / 4 / 2 / 1, not above max(F, Fs) rounded up to 16 columns,
// at which both paths' columns fit.  There are ceil(max(F, Fs) / (16 NT)) passes; a gathered
// row is read once per pass.  16-bit storage always fits at NT = 1 (16 x 2 x 2048 bytes).
// K TILING: fp32 with a self path may not fit even 16 columns (e.g. d = 544, ds = 512).  Then K
// is cut into W tiles of 512 (4 fold tiles), both paths' tile is re-staged per W tile and run
// group, and the 4 waves move in lockstep; otherwise W is staged once per pass and the waves run
// free.
// The grid is capped (kDenseMaxBlocks); a workgroup loops over groups of 4 runs beyond it.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "mp_pool.h"

namespace euler_gpu {

constexpr int kDenseNone = 0, kDenseAdd = 1, kDenseConcat = 2, kDenseFold = 3;   // combine
constexpr int kDenseMaxK = 1024;          // d, ds
constexpr int kDenseMaxF = 4096;          // F, Fs
constexpr int kDenseWaves = 4;            // per workgroup
constexpr int kDenseFoldTile = 128;       // k per fold tile: 4 chunks of kPoolChunk
constexpr int kDenseLdsBytes = 65536;
constexpr int kDenseLockTile = 512;       // k per W tile when the waves move in lockstep
constexpr int kDenseMaxBlocks = 512;         // 2 resident workgroups x 256 CUs: W is staged once per slot

struct DensePlan {
  int32_t nt;         // accumulator fragments per path: F_tile = 16 * nt
  int32_t f_passes;   // F-tile passes over the gathered rows
  int32_t w_tile;     // k per staged W tile, a multiple of 128
  int32_t w_tiles;    // 1: both W^T of an F tile are staged once per pass
  int32_t stride_n;   // bytes between the columns of the neighbour path's Wt
  int32_t stride_s;   // ... of the self path's (0: no root_weight)
  int32_t lds_bytes;  // dynamic LDS of a workgroup
};

// bytes between the columns of a Wt whose K extent is k32 elements
inline int32_t DenseColumnBytes(int32_t k32, int32_t esz) {
  const int32_t b = k32 * esz;
  return b % 256 == 0 ? b : b + 16;
}

// ds_w: the rows of root_weight, 0 without one; f_max: max(F, Fs)
inline DensePlan DenseMakePlan(int64_t d, int64_t ds_w, int64_t f_max, bool f32) {
  const int32_t esz = f32 ? 4 : 2;
  const int32_t d32 = (int32_t)((d + kPoolChunk - 1) / kPoolChunk) * kPoolChunk;
  const int32_t s32 = (int32_t)((ds_w + kPoolChunk - 1) / kPoolChunk) * kPoolChunk;
  const int32_t f16 = (int32_t)((f_max + 15) / 16);
  DensePlan p{};
  p.stride_n = DenseColumnBytes(d32, esz);
  p.stride_s = s32 ? DenseColumnBytes(s32, esz) : 0;
  p.nt = 8;
  while (p.nt > 1 && (p.nt / 2 >= f16 || (int64_t)16 * p.nt * (p.stride_n + p.stride_s) > kDenseLdsBytes)) p.nt /= 2;
  const int32_t k_max = d32 > s32 ? d32 : s32;
  p.w_tile = (k_max + kDenseFoldTile - 1) / kDenseFoldTile * kDenseFoldTile;
  if ((int64_t)16 * p.nt * (p.stride_n + p.stride_s) > kDenseLdsBytes) {
    p.w_tile = kDenseLockTile;
    p.stride_n = DenseColumnBytes(d32 < kDenseLockTile ? d32 : kDenseLockTile, esz);
    p.stride_s = s32 ? DenseColumnBytes(s32 < kDenseLockTile ? s32 : kDenseLockTile, esz) : 0;
  }
  p.w_tiles = (k_max + p.w_tile - 1) / p.w_tile;
  p.f_passes = (int32_t)((f_max + 16 * p.nt - 1) / (16 * p.nt));
  p.lds_bytes = 16 * p.nt * (p.stride_n + p.stride_s);
  return p;
}

// byte offset of byte kb (of the staged K extent) of column c
EG_MPW_HD uint32_t DenseWtByte(int32_t c, int32_t kb, int32_t stride) {
  const int32_t unit = kb >> 4;
  return (uint32_t)(c * stride + (((stride & 255) == 0 ? unit ^ (c & 15) : unit) << 4) + (kb & 15));
}

// The denominator of a mean over n terms: that of gather_segment_reduce
EG_MPW_HD float DenseDenominator(int64_t n) { return MpwAdd((float)n, 1e-7f); }

}  // namespace euler_gpu
