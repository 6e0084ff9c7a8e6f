// Layerwise-adjacency aggregation straight from the bit mask - the aggregators the reference runs
// over the SparseTensor of a layerwise sample (tf_euler/python/utils/sparse_aggregators.py:37-84:
// GCNAggregator with and without renorm, MeanAggregator; tf.sparse_tensor_dense_matmul(adj, x)
// divided by the degree) - on the matrix units, read from the [batch, n, m] adjacency as
// euler_gpu_sparse_adj_mask writes it: uint64 [batch * n][(m + 63) / 64], bit c % 64 of word c / 64
// of source i = "candidate c of this batch row is a neighbour".  No COO triple, no nnz, no host
// wait, no index array, no atomics.  This file states the contract and holds the tile plan; the
// host entry, the kernels (mask_aggregate_kernels.hip) and a host-only program can all include it.
//
// For batch row b, source i and feature column f:
//
//     N(b,i)   = { c < m : bit c of mask[b*n + i] }          deg = |N(b,i)|
//     S[b,i,f] = sum_{c in N(b,i)} x[b*m + c, f]
//
//     add          out[b*n + i] = S                                 sparse_tensor_dense_matmul
//     mean                      = S / max(deg, 1e-7)                MeanAggregator
//     gcn                       = root + S / max(deg, 1e-7)         GCNAggregator, renorm=False
//     gcn_renorm                = (root + S) / (1 + deg)            GCNAggregator, renorm=True
//
// ARGUMENTS.  mask uint64 [batch * n, words], words = (m + 63) / 64, contiguous.  x [>= batch * m,
// d] fp32 / bf16 / fp16, contiguous rows; a view off a 16-byte boundary (or d % 8 != 0, fp32 % 4)
// is read by element loads.  root [batch * n, d] of x's dtype, required by the two gcn ops and
// ignored by the others.  out fp32 or x's dtype.  degree_out: optional fp32 [batch * n], written
// from the popcounts in the same launch.
// STRAY BITS at positions >= m of the last word are ignored: they neither count towards the degree
// nor contribute to the sum, and row b*m + c of x for c >= m is never read.
// ARITHMETIC.  The bits expand to operands that are exactly 0 or 1, so every product is exact; S is
// accumulated in fp32 by the matrix instructions in a fixed order of c that depends only on m and
// the plan (the chunks of 32 candidates in increasing c) - never on where the source sits in a
// wave, a workgroup or the grid.  The root term is added in fp32; the division is ONE correctly
// rounded fp32 division by fl(max(deg, 1e-7f)) resp. fl(1 + deg); one rounding to the output
// dtype.  A source with no bit set has S = +0.
// NON-FINITE VALUES.  0 * inf and 0 * NaN are NaN: a non-finite x[b*m + c, f] makes column f NaN
// for the sources of batch row b whether c is their neighbour or not - the reference's sparse
// product does not do this.  It is not hidden behind a branch per element.  (The one exception is
// the zero-word skip below: a run of 16 sources none of which has a bit in c's word of 64 never
// multiplies by that word, and keeps its finite sums.)
// DETERMINISM.  The same bits on every run and on every stream.
// LIMITS.  batch * n < 2^31, batch * m < 2^31, 1 <= d <= 1024.  batch * n == 0 touches nothing; m
// == 0 reads no x and writes the zero-fill (gcn, gcn_renorm: the copy of root) and a degree of 0.
//
// THE TILING (MaskPlan below is its one statement).
// ROLES: M = 16 sources, K = candidates, N = 16 feature columns.  A wave owns 2 RUNS of 16 sources;
// a workgroup of 4 waves (2 where that fills more of the device) owns one batch row's tile of 128
// (64) sources and one column tile of 16 NT <= 128 columns, and loops over candidate blocks of KB.
// Work items (batch row, source tile, column tile) are laid on a capped grid, the column tile
// fastest, with a loop beyond the cap.
// MASK OPERAND, 16 bits.  Lane l holds source l % 16 and, per chunk of 32 candidates, the 8
// consecutive candidates from 8 * (l / 16): its A fragment of v_mfma_f32_16x16x32_{bf16,f16} is ONE
// BYTE of its source's mask row - bytes l / 16 and 4 + l / 16 of a word it reads once - expanded to
// eight 16-bit values 0x3F80 / 0x3C00 or 0 with bit tests and selects, in registers (no table in
// LDS: the LDS pipe is what the B reads need).  fp32: instruction j of the eight
// v_mfma_f32_16x16x4_f32 of a chunk takes candidate 4 j + l / 16, i.e. bit 4 j + l / 16 of the
// chunk's 32, as 1.0f or 0.  Every lane of a source reads the whole word, so its popcount IS the
// degree; the epilogue fetches the degrees of its rows by lane index.
// FEATURE OPERAND, 16 bits.  x[b*m + c0 .. c0 + KB, f0 .. f0 + 16 NT] is staged once per workgroup
// and candidate block and shared by all its runs.  B wants 8 consecutive candidates of one column
// per lane, so the tile is staged TRANSPOSED, Xt[f][c], in 16-byte units: a thread loads an 8 x 8
// block (eight 16-byte global loads of row-major rows), transposes it in registers and stores
// eight 16-byte units.  No 2-byte LDS store.  Where a column's extent KB * 2 is a multiple of 256
// bytes the columns are packed and unit u of column f sits at u ^ ((f + f / 16) % 16): the 16
// columns of a B read fall on distinct banks, and so do the 16 column blocks of a staging store.
// Otherwise the stride is the extent + 16 bytes.  Candidates >= m and columns >= d are +0.
// FEATURE OPERAND, fp32: row-major X[c][f], row stride 16 NT + 16 floats, so that the four rows 4 j
// .. 4 j + 3 one instruction reads fall on distinct banks.  No transpose.
// A B fragment is read from LDS once and multiplied into both runs of the wave.
// ZERO-WORD SKIP.  A run whose 16 sources all have a zero word skips the MFMAs of that word: one
// ballot, a wave-uniform branch.
// EPILOGUE in the accumulator layout (lane l: rows 4 (l / 16) + i of column l % 16): root add,
// division, narrowing, store.  No LDS round trip, no atomics.
// LDS BUDGET: 64 KB (16 bits, KB = 256, 128 columns); fp32 36 KB (KB = 64).
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "mp_dense.h"

namespace euler_gpu {

constexpr int kMaskAdd = 0, kMaskMean = 1, kMaskGcn = 2, kMaskGcnRenorm = 3;
constexpr int kMaskMaxD = 1024;
constexpr int kMaskWaves = 4;             // per workgroup, at most
constexpr int kMaskRuns = 2;              // runs of 16 sources per wave
constexpr int kMaskBlock16 = 256;         // candidates per block, 16-bit x
constexpr int kMaskBlock32 = 64;          // ... fp32 x
constexpr int kMaskMaxNt = 8;             // 128 columns per column tile
constexpr int kMaskLdsBytes = 65536;
constexpr int kMaskMaxBlocks = 1024;      // 2 resident workgroups x 256 CUs x 2
constexpr int kMaskFewItems = 256;        // below this many work items a workgroup is 2 waves

struct MaskPlan {
  int32_t nt;         // accumulator fragments per run: the column tile is 16 * nt
  int32_t col_tiles;  // column tiles of d
  int32_t kb;         // candidates per block, a multiple of 64
  int32_t stride;     // bytes between the columns of Xt (16 bits) / the rows of X (fp32)
  int32_t lds_bytes;  // dynamic LDS of a workgroup
};

inline MaskPlan MaskMakePlan(int64_t m, int64_t d, bool f32) {
  MaskPlan p{};
  p.nt = 1;
  while (p.nt < kMaskMaxNt && 16 * p.nt < d) p.nt *= 2;
  p.col_tiles = (int32_t)((d + 16 * p.nt - 1) / (16 * p.nt));
  const int64_t m64 = (m < 1 ? 1 : m) + 63 - ((m < 1 ? 1 : m) + 63) % 64;
  const int32_t cap = f32 ? kMaskBlock32 : kMaskBlock16;
  p.kb = m64 < cap ? (int32_t)m64 : cap;
  if (f32) {
    p.stride = (16 * p.nt + 16) * 4;
    p.lds_bytes = p.kb * p.stride;
  } else {
    p.stride = DenseColumnBytes(p.kb, 2);
    p.lds_bytes = 16 * p.nt * p.stride;
  }
  return p;
}

// sources of a workgroup's tile
inline int32_t MaskTile(int32_t waves) { return waves * kMaskRuns * kPoolTile; }

// waves of a workgroup: 4, or 2 where 4 would leave fewer work items than the device has slots for
inline int32_t MaskWaves(int64_t batch, int64_t n, int32_t col_tiles) {
  const int64_t tiles = (n + MaskTile(kMaskWaves) - 1) / MaskTile(kMaskWaves);
  return batch * tiles * col_tiles < kMaskFewItems && n > MaskTile(2) ? 2 : kMaskWaves;
}

// byte offset in Xt of byte kbyte (of the block's candidates, 2 bytes each) of column f
EG_MPW_HD uint32_t MaskXtByte(int32_t f, int32_t kbyte, int32_t stride) {
  const int32_t unit = kbyte >> 4;
  return (uint32_t)(f * stride + (((stride & 255) == 0 ? unit ^ ((f + (f >> 4)) & 15) : unit) << 4) + (kbyte & 15));
}

// the denominators of the dividing ops
EG_MPW_HD float MaskMeanDenominator(float deg) { return deg > 1e-7f ? deg : 1e-7f; }
EG_MPW_HD float MaskRenormDenominator(float deg) { return MpwAdd(1.0f, deg); }

}  // namespace euler_gpu
