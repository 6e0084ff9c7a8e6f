// Fused gated-graph step - the neighbour sum of the reference's GatedConv
// (tf_euler/python/convolution/gated_graph_conv.py:26-57) and ONE tf.nn.rnn_cell.GRUCell of its
// stack, seeded with the destination's own row.  With m[r] the aggregate of destination r,
// h = state[r] and K = d + U:
//
//     m[r]    = reduce_{p in segment(r)} table[g[p]]                  reduce = add | mean
//     [r | u] = sigmoid([m, h] @ gate_weight + gate_bias)             gate_weight [K, 2U]
//     c       = tanh([m, r * h] @ cand_weight + cand_bias)            cand_weight [K, U]
//     out[r]  = u * h + (1 - u) * c                                   [size, U]
//
// in one pass on the matrix units.  This is GRUCell.call of TF 1.x: r * h is formed BEFORE the
// candidate product (torch.nn.GRUCell multiplies after it), the weights are the cell's own
// gates/kernel and candidate/kernel - rows 0 .. d - 1 multiply the input, rows d .. d + U - 1 the
// state; r is the first U gate columns, u the last U.  Neither the [size, d] sum nor the [size, 2U]
// and [size, U] pre-activation blocks are written.  One call is one cell; the second cell of a stack
// is a call with no gather array and count 1 over the first cell's output, with the same state.
// This file states the contract and holds the plan; the kernel (aggregate_gru_kernels.hip) and a
// host-only program can both include it.
//
// ARGUMENTS.  table [rows, d], state [size, U], gate_weight [d + U, 2U] and cand_weight [d + U, U],
// contiguous, one dtype of fp32 / bf16 / fp16.  gate_bias [2U] and cand_bias [U], each fp32 or that
// dtype, widened exactly; none = +0 (the TF cell's gate bias of 1.0 is the caller's to pass).
// SEGMENTS, INDICES, THE RANGE RULE, DETERMINISM: those of mp_dense.h, word for word - seg_ptr or
// count, exactly one; int32 indices, int64 ids or the position itself; an index outside [0, rows)
// is never dereferenced, reads as a row of +0 and still counts in a mean's length; the same bits on
// every run, on every stream and for count or the equivalent seg_ptr.
// ARITHMETIC.  The fold is that of mp_dense.h: from +0, the widened rows in increasing p in fp32,
// one rounding per add; mean divides by fl(len + 1e-7f); m is rounded ONCE to the table's dtype
// (fp32: kept).  The products of both GEMMs are accumulated in fp32 by the matrix instructions in an
// order that depends only on d and U: the chunks of 32 k of the input rows in increasing k, then
// those of the state rows; a zero-filled tail adds +0.  The bias is added in fp32 (one add), then
//     sigmoid(x) = 1 / (1 + expf(-x))      expf: the device library's (1 ulp); the add and the
//                                          division are single correctly rounded fp32 operations
//     tanh(x)    = tanhf(x)                the device library's (2 ulp)
// - no fast-math substitution (no __expf, no reciprocal for the division, no exp-based tanh): this
// translation unit is built without -ffast-math and with contraction off.  Both results lie in
// [-1, 1], so kGruActUlps * 2^-24 bounds the absolute error of either (sigmoid: the relative error
// 2^-23 of expf reaches the result with a factor s (1 - s) <= 1/4, plus two roundings of values
// <= 2; tanh: 2 ulp of a value <= 1).  r * h is ONE fp32 multiply, rounded once to the table's
// dtype before it is a matrix operand (fp32: kept).  The blend is fl(fl(u * h) + fl(fl(1 - u) * c))
// in fp32, rounded once to the output dtype (fp32 or the table's).
// LIMITS.  e, size < 2^31; 1 <= d <= 256; 1 <= U <= 256; rows >= 1.  Anything wider is refused,
// never served by another route.  size == 0 touches nothing.
//
// THE DESIGN (GruPlan below is its one statement).
// A workgroup is 8 waves; a wave owns RUNS of 16 consecutive destinations, one run per staging of
// the weights: 128 destinations share every byte of W that is staged.  Lane l owns destination
// c = l % 16 and, per chunk of 32 k, the slots 8 g .. 8 g + 7, g = l / 16.
// TRANSPOSED PRODUCTS.  Z^T = W^T @ [m, h]^T: the staged W^T is the A operand of
// v_mfma_f32_16x16x32_{bf16,f16} (row = gate column), the lane's own registers are the B operand
// (column = destination c, the 8 k of group g) - exactly what the fold of mp_dense.h leaves in a
// lane.  The accumulator of tile t then gives lane l the gate columns 16 t + 4 g + i, i < 4, of ITS
// OWN destination: the lane that owns m and h of a destination owns its r, u and c.
// r * h STAYS IN REGISTERS.  Two adjacent tiles 2 x, 2 x + 1 give the lane 8 values of r * h:
// state columns 32 x + 16 (j / 4) + 4 g + j % 4, j < 8.  They are slot 8 g + j of chunk x of the
// candidate product's B operand, PROVIDED cand_weight's state rows sit in LDS under the same
// permutation: slot 8 g + j of chunk x holds row d + 32 x + 16 (j / 4) + 4 g + j % 4
// (GruStateRow).  A sum over k does not care in which slot a k sits as long as A and B agree, so
// r * h goes from accumulator to operand with one multiply and one narrowing: no LDS round trip, no
// cross-lane traffic.  fp32 uses the eight v_mfma_f32_16x16x4_f32 of mp_pool.h per chunk,
// instruction j taking slot j of every lane: the same permutation holds.  The input rows of both
// weights and the state rows of gate_weight are staged in plain order.
// WHAT IS KEPT.  Per run a lane keeps the m fragments (d32 / 32 chunks) and the r * h fragments
// (U32 / 32 chunks): 4 registers a chunk in 16 bits, 8 in fp32 - 32 registers at d = U = 128 in 16
// bits, 128 at d = U = 256 in fp32.  Every byte of a gathered row is read ONCE; with CH = 8 and d > 128
// the fold walks the segment once per fold tile of 128 k, so the gather indices are read twice.  The
// h fragments of the gate
// products are re-read from the destination's state row per pass, and the 4 h values a lane needs
// per tile for r * h and the blend are 4 consecutive elements of that row: the row is hot.  u and c
// of a column tile are formed in the same pass and never kept.
// PHASES.  The weights do not fit LDS (3 U (d + U) elements: 192 KB at d = U = 128 in 16 bits), so
// the gate and candidate columns are phased over a 64 KB window.  ONE workgroup is resident per CU:
// every instantiation needs more than 128 registers, so a SIMD holds 2 or 3 waves and a CU one
// workgroup of 8, and the second 64 KB of a 128 KB allocation would be free.  What a 128 KB window
// (NT doubled, 8 NT more accumulator registers) would and would not change: every column of W is
// staged once per group whatever the window, so the staged bytes per destination stay; the passes,
// their barriers and the re-reads of the h fragments halve (d = U = 128 in 16 bits: 1 r + 2 c
// passes become 1 + 1).  It is not taken here - DESIGN 4.31 says what the measured time leaves to
// gain from it.  Per group of 8 runs the waves move in LOCKSTEP:
//   fold      every wave folds its run (no LDS);
//   r passes  32 NT gate columns of r over the whole K are staged; 2 NT accumulator tiles; sigmoid,
//             times h, narrowed into the r * h fragments;
//   c passes  16 NT columns of u (gate_weight) and the same 16 NT columns of c (cand_weight, state
//             rows permuted) are staged side by side; NT + NT accumulator tiles; the blend; the store.
// Two barriers per pass.  Columns past U are staged as +0 and multiplied like any other: a pass has
// no branch per tile, which is what keeps the unrolled chunk steps out of scratch.
// NT and the register arrays' extent CH are fixed per instantiation by max(d, U) and the dtype:
//   CH = 4 (d, U <= 128):  NT = 4 in 16 bits (d = U = 128: 1 r pass + 2 c passes), 2 in fp32
//   CH = 8 (<= 256):       NT = 2 in 16 bits, 1 in fp32
// so that 32 NT columns of the widest K of the instantiation are 64 KB at most.
// W IN LDS is Wt[column][k] as in mp_dense.h (DenseWtByte: packed and XOR-swizzled where the K
// extent is a multiple of 256 bytes, else + 16 bytes a column).
// The grid is capped (kGruMaxBlocks); a workgroup loops over groups of 8 runs beyond it.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <math.h>
#include <stdint.h>

#include "mp_dense.h"

namespace euler_gpu {

constexpr int kGruMaxD = 256;             // d
constexpr int kGruMaxU = 256;             // U
constexpr int kGruWaves = 8;              // per workgroup
constexpr int kGruLdsBytes = 65536;
constexpr int kGruMaxBlocks = 512;        // 2 rounds of 1 resident workgroup x 256 CUs
constexpr int kGruActUlps = 4;            // |error| of sigmoid and of tanh <= kGruActUlps * 2^-24

struct GruPlan {
  int32_t ch;         // extent of the fragment arrays in chunks of 32: 4 (d, U <= 128) or 8
  int32_t nt;         // accumulator tiles per gate in a c pass; an r pass has 2 nt
  int32_t kd;         // chunks of the input rows: d32 / 32
  int32_t ku;         // chunks of the state rows: U32 / 32
  int32_t r_passes;   // ceil(ku / nt)
  int32_t c_passes;   // ceil(U / (16 nt))
  int32_t stride;     // bytes between the columns of Wt: the staged K extent is 32 (kd + ku)
  int32_t lds_bytes;  // dynamic LDS of a workgroup
};

inline GruPlan GruMakePlan(int64_t d, int64_t u, bool f32) {
  GruPlan p{};
  p.ch = d > 128 || u > 128 ? 8 : 4;
  p.nt = (f32 ? 8 : 16) / p.ch;
  p.kd = (int32_t)((d + kPoolChunk - 1) / kPoolChunk);
  p.ku = (int32_t)((u + kPoolChunk - 1) / kPoolChunk);
  p.r_passes = (p.ku + p.nt - 1) / p.nt;
  p.c_passes = (int32_t)((u + 16 * p.nt - 1) / (16 * p.nt));
  p.stride = DenseColumnBytes(kPoolChunk * (p.kd + p.ku), f32 ? 4 : 2);
  p.lds_bytes = 32 * p.nt * p.stride;
  return p;
}

// The state row (0 .. 32 ku) that slot s of the PERMUTED state rows of cand_weight holds: the lane
// of group g = (s % 32) / 8 finds in its slots j = s % 8 the columns its two accumulator tiles gave it
EG_MPW_HD int32_t GruStateRow(int32_t s) {
  const int32_t x = s >> 5, g = (s >> 3) & 3, j = s & 7;
  return 32 * x + 16 * (j >> 2) + 4 * g + (j & 3);
}

EG_MPW_HD float GruSigmoid(float x) { return MpwDiv(1.f, MpwAdd(1.f, expf(-x))); }
EG_MPW_HD float GruTanh(float x) { return tanhf(x); }

// out = u * h + (1 - u) * c, every operation rounded on its own
EG_MPW_HD float GruBlend(float u, float h, float c) { return MpwAdd(MpwMul(u, h), MpwMul(MpwAdd(1.f, -u), c)); }

}  // namespace euler_gpu
