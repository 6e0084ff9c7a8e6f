// Fused mean-aggregator layer (mp_dense.h) over a quantised row table (Fp8Rows: mp_fp8.h): layer 0
// of a GraphSAGE forward over the outermost hop, where the gathered rows are the model's constant
// input features and their bytes are what the kernel waits for.  The four formulas - root none /
// add / concat / fold -, the segment forms, the range rule, the limits and the determinism are
// those of mp_dense.h; this file states what differs and holds the one map the layout needs.  The
// host entry, the kernel (fp8_dense_kernels.hip) and a host-only program can all include it.
//
// TABLE.  q [rows, d] of e4m3fn codes and scale [d] fp32, finite and positive.  An element's value
// is that of mp_fp8.h: x^ = fl(Dec(code) * scale[c]), one correctly rounded fp32 multiply per
// element, never contracted into the add.  The codes are NOT summed and scaled afterwards: that is
// cheaper, and it breaks the family's one rule - an op on the table is the fp32 op on dequantize().
// COMPUTE DTYPE: the weight's, fp32 / bf16 / fp16.  A dense root, root_weight and bias follow it as
// they follow the table's dtype in mp_dense.h (bias may also be fp32); out is fp32 or of it.
// THE FOLD is mp_dense.h's: from +0, in increasing p, fp32, one rounding per add; mean divides by
// fl(len + 1e-7f) with a rounded division; A is rounded once to the weight's dtype (fp32: kept).
// With an identity weight, no bias, no activation and no root the output has the bits of
// gather_segment_reduce over the same table with out_dtype = the weight's dtype.  An index outside
// [0, rows) is a row of zero codes - +0 under every scale - that still counts.
// ROOT.  Either dense, [size, ds] of the weight's dtype, as in mp_dense.h; or INDEXED: root_index
// [size], int32 indices or int64 ids, rows of the same table, which is how layer 0 gets them.  Then
// ds == d; the root row is x^, rounded once to the weight's dtype as the self path's A operand
// (add, concat), or the fold's first term in fp32, times root_scale when given (fold).  An index
// outside the table is a row of +0.
// PRODUCTS.  Accumulated in fp32 by the matrix instructions in an order that depends only on d and
// ds: the K chunks of 32 in increasing SLOT order, where slot k' of the neighbour path (and of an
// indexed root's self path) holds element Fp8DenseRow(k') - below; a dense root's self path keeps
// the plain order.  So the bits are not those of aggregate_dense on the dequantised table; the
// error bound is.
//
// THE LAYOUT.  mp_dense.h gives lane l destination l % 16 and, per chunk of 32, 8 consecutive k:
// 8 bytes of an fp8 row, too little for a 16-byte load.  Here K is walked in BLOCKS of 64 codes: in
// block b lane l (g = l / 16) loads the 16 bytes at k = 64 b + 16 g of its gathered row, so the
// four lane groups of a wave cover 64 contiguous bytes of a row per block, a 128-d row is read as
// exactly its one 128-byte line, and every byte is read once per F pass.  A fold tile stays 128 k =
// 2 blocks = 32 fp32 registers, with 2 loads per position instead of 4.  The sixteen codes are
// decoded (v_cvt_pk_f32_fp8) and multiplied by the lane's sixteen column scales: d / 4 scale
// registers per fold tile, loaded once per pass when d <= 128 and per fold tile beyond (they are
// hot).  The lane's sixteen values are two MFMA chunks: values 0..7 are chunk 2 b, values 8..15
// chunk 2 b + 1.  W^T therefore sits in LDS under the fixed permutation Fp8DenseRow, rows from d on
// +0 up to the next multiple of 64; everything downstream - DenseChunkMma, the XOR-swizzled packed
// columns, the accumulator layout, the epilogue, the fp32 16x16x4 path - is mp_dense.h's, because
// only the row that sits at a slot changes.
// PLAN: DenseMakePlan with d (and the ds of an indexed root) rounded up to 64.  d = ds = F = 128 in
// 16 bits stays one pass of 64 KB; the lockstep K tile of 512 is a multiple of 64.
// LOAD RULES.  16-byte loads when d % 16 == 0 and q is 16-byte aligned (and a dense root obeys
// PoolVectorLoads); otherwise byte loads, correct and slower.  Nothing is read past a row.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "mp_dense.h"

namespace euler_gpu {

constexpr int kFp8DenseBlock = 64;        // codes per K block: 4 lane groups x one 16-byte load

// The element (row of W, column of the table) that sits at slot kp of the staged K extent: with
// kp = 32 (2 b + j) + 8 g + i - chunk 2 b + j, lane group g, element i of the chunk's A fragment -
// it is 64 b + 16 g + 8 j + i, value 8 j + i of the 16-byte load of group g in block b.
EG_MPW_HD int32_t Fp8DenseRow(int32_t kp) {
  return (kp & ~63) | ((kp & 24) << 1) | ((kp & 32) >> 2) | (kp & 7);
}

inline int32_t Fp8DenseRound(int64_t d) { return (int32_t)((d + kFp8DenseBlock - 1) / kFp8DenseBlock) * kFp8DenseBlock; }

// root_rows: the rows of root_weight, 0 without one; indexed: they are read from the table
inline DensePlan Fp8DenseMakePlan(int64_t d, int64_t root_rows, bool indexed, int64_t f_max, bool f32) {
  return DenseMakePlan(Fp8DenseRound(d), indexed && root_rows ? Fp8DenseRound(root_rows) : root_rows, f_max, f32);
}

inline bool Fp8DenseVectorLoads(int64_t d, uintptr_t q) { return q % 16 == 0 && d % 16 == 0; }

}  // namespace euler_gpu
