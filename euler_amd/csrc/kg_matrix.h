// TransR's per-relation matrix projection fused into triple scoring (generate_embedding of
// examples/TransX/transR.py:41-68, calculate_energy of transX.py:72-79,105-133): the arithmetic
// contract, built on kg_score.h, shared by the kernels of kg_matrix_kernels.hip and by
// tests/csrc/kg_matrix_check.cc, which compiles this file with the host compiler.  As in
// kg_score.h every operation is one correctly rounded fp32 operation without contraction, and the
// RANGE RULE holds for all three tables: an id outside [0, rows) names no row, is never
// dereferenced, reads as +0 and gets +0 gradient rows; a rel_id that names no relation removes
// both rel[rho] and M_rho (every element reads as +0).
//
// Tables ent [N, de], rel [R, dr], matrix [R, de * dr] read row-major as M_rho [de, dr], each
// widened exactly to fp32.  Per triple (src, rho, dst) with negatives neg [K]:
//   an entity row x = ent[i] is NOT normalised;  z_j = sum_c x_c * M_rho[c, j], j < dr;
//   ss = sum z_j * z_j, inv = KgInv(ss, true), y_j = z_j * inv;  r = N(rel[rho]) as in kg_score.h;
//   scores: kind trans_l1 or trans_l2 of kg_score.h over the dr columns, e_j = (a_j + r_j) - c_j,
//   KgFinish; corrupt and the layout of the outputs as there.  The projection of n_k is computed
//   once per k and serves the front and the tail score.
//
// SUMMATION ORDERS.  Each depends on de, dr, the dtypes and the alignment of `rel` only - never on
// B, K, R, the grid, the grouping of the triples or on which other triples are in the batch.
//   z_j     for each column j on its own: the terms fl(x_c * M[c, j]) are added one by one in
//           increasing c, starting FROM the first term (KgmStep).  No tiling of M over c shows.
//   ss, the dot of the normalisation's gradient, the scores over dr: kg_score.h's order with
//           d = dr and V = KgMatrixChunkWidth: KgChunkWidth applied to `rel` alone (no other
//           table's rows meet these sums); L = min(64, the power of two >= dr / V) lanes, lane l
//           takes the chunks l, l + L, ..., then the xor butterfly.
// GRADIENT.  The score-level gy are KgLaneScoreGrad's: sign(0) = 0, gq = 0 where q == 0, every gy
//   from +0, the true triple, then k = 0 .. K - 1, front before tail.  A projected row whose gy is
//   complete goes through its normalisation (whether or not its entity id names a row):
//     dot = sum y_j * gy_j,  gz_j = inv * (gy_j - y_j * dot) where ss > 1e-12f, else inv * gy_j.
//   gx_c = sum_j gz_j * M[c, j]: for each c on its own the terms fl(gz_j * M[c, j]) are added in
//     increasing j, starting from the first term (KgmRowDot); +0 for an entity id without a row.
//   G_M[rho][c, j] = sum fl(x_c * gz_j) over the occurrences of relation rho, one by one from the
//     first term: by increasing triple index b, within a triple n_0 .. n_{K-1}, h, t (kg_proj.h's
//     row order).  An occurrence whose entity id names no row contributes no term; a relation
//     with no term gets +0.  The sum is rounded once to the matrix's dtype.
//   g_rel goes through rel's normalisation as in kg_score.h (KgLaneRowGrad).
// CAP: 1 <= de, dr <= kKgMatrixMaxDim.  With dr <= 512 a lane owns at most 8 columns at every V
// (V = 8: one chunk, V = 4: two, V = 1: eight), which is what KgmRegs holds.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "kg_score.h"

namespace euler_gpu {

constexpr int64_t kKgMatrixMaxDim = 512;
constexpr int kKgmCols = 8;                       // the columns a lane owns at most

// V of the dr-sums: kg_score.h's rule over `rel` alone
inline int32_t KgMatrixChunkWidth(int64_t dr, uintptr_t rel, bool rel_f32) {
  return KgChunkWidth(dr, rel, rel_f32, rel, rel_f32);
}

// A lane's columns of one projected row (or of its gy) in registers: the chunks l, l + L, ...
// l + (NC - 1) L of V columns each, NC * V == kKgmCols.  It is a Row and an Acc of kg_score.h;
// chunk j of lane l is slot j >> log_l (l < L).  The slot is picked by bit masks, never by a
// run-time index or a select between loads, so the values stay in registers; the bits of a value
// pass unchanged.
EG_MPW_HD uint32_t KgmBits(float x) { return __builtin_bit_cast(uint32_t, x); }
EG_MPW_HD float KgmFloat(uint32_t w) { return __builtin_bit_cast(float, w); }
EG_MPW_HD uint32_t KgmMask(bool on) { return on ? 0xffffffffu : 0u; }

template <int V>
struct KgmRegs {
  static constexpr int NC = kKgmCols / V;
  float v[kKgmCols];
  int32_t log_l;
  EG_MPW_HD void Clear(int32_t log_lanes) {
    log_l = log_lanes;
EG_MPW_UNROLL
    for (int i = 0; i < kKgmCols; ++i) v[i] = 0.f;
  }
  EG_MPW_HD void Chunk(int32_t j, float f[V]) const {
    const int32_t m = j >> log_l;
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) {
      uint32_t r = 0;
EG_MPW_UNROLL
      for (int q = 0; q < NC; ++q) r |= KgmBits(v[q * V + k]) & KgmMask(m == q);
      f[k] = KgmFloat(r);
    }
  }
  EG_MPW_HD void Get(int32_t j, float f[V]) const { Chunk(j, f); }
  EG_MPW_HD void Put(int32_t j, const float f[V]) {
    const int32_t m = j >> log_l;
EG_MPW_UNROLL
    for (int q = 0; q < NC; ++q) {
      const uint32_t on = KgmMask(m == q);
EG_MPW_UNROLL
      for (int k = 0; k < V; ++k) v[q * V + k] = KgmFloat((KgmBits(f[k]) & on) | (KgmBits(v[q * V + k]) & ~on));
    }
  }
};

// The first column of each slot of lane l, or -1 for a slot past the row's chunks.
template <int V>
EG_MPW_HD void KgmSlots(int32_t l, int32_t lanes, int32_t chunks, int32_t col[kKgmCols / V]) {
EG_MPW_UNROLL
  for (int q = 0; q < kKgmCols / V; ++q) {
    const int32_t j = l + q * lanes;
    col[q] = j < chunks ? j * V : -1;
  }
}

// One c-step of a lane's z: z_j = z_j + x * m[j] for its columns (first: z_j = x * m[j]).
// m: the fp32 row M[c, 0 .. dr).  A slot without columns reads m[0 .. V) and is never used.
template <int V>
EG_MPW_HD void KgmStep(KgmRegs<V>& z, float x, const float* m, const int32_t col[kKgmCols / V], bool first) {
EG_MPW_UNROLL
  for (int q = 0; q < kKgmCols / V; ++q) {
    const float* p = m + (col[q] < 0 ? 0 : col[q]);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) {
      const float t = MpwMul(x, p[k]);
      z.v[q * V + k] = first ? t : MpwAdd(z.v[q * V + k], t);
    }
  }
}

// gx_c from the row gz [n] and the fp32 row M[c, 0 .. n): increasing j from the first term
EG_MPW_HD float KgmRowDot(const float* gz, const float* m, int32_t n) {
  float s = MpwMul(gz[0], m[0]);
  for (int32_t j = 1; j < n; ++j) s = MpwAdd(s, MpwMul(gz[j], m[j]));
  return s;
}

}  // namespace euler_gpu
