// The gradient of mask_attention (mp_mask_attention.h) in two launches on the matrix units: a
// SOURCE-MAJOR kernel over the mask and a CANDIDATE-MAJOR kernel over its transpose (mask_transpose).
// No COO triple, no [n, m] block in memory, no atomics, no host wait.  This file states the contract
// and holds the tile plan; the host entry and the kernels (mask_attention_backward_kernels.hip) and a
// host-only program can all include it.
//
// Notation of mp_mask_attention.h; per batch row b, source i, head h, with g the incoming gradient row
// of the head (with relu: zeroed where the SAVED forward output is <= 0 - the forward's own select):
//
//     a_c = fl(s_src + s_nb[c])      lambda_c = a_c < 0 ? slope : 1     (a_0, lambda_0: the self term)
//     p_c, M, l as in the forward    alpha_c = p_c / l
//     D          = sum_c alpha_c (g . z_c) + alpha_0 (g . root_h)
//     d z[c]    += alpha_ic g_i                              over the sources i of the batch row
//     d s_nb[c] += alpha_ic lambda_ic (g_i . z_c - D_i)      over the sources i
//     d s_root   = alpha_0 lambda_0 (g . root_h - D)         renorm form only
//     d s_src    = sum_c alpha_c lambda_c (g . z_c - D) + d s_root
//     d root     = g (root-only form) | alpha_0 g (renorm form)
//
// The product g . z_c is never formed per (source, candidate).  Both sums are linear in g, and lambda
// takes two values: every numerator is SPLIT by the sign of its pre-activation, p+ = (a >= 0) ? p : 0
// and p- = p - p+ (a select of the forward's own rounded p, never a product), into two A fragments and
// two accumulator sets.
//
// KERNEL 1, SOURCE-MAJOR.  Work item = (batch row, source tile, head) on a capped grid with a loop
// beyond the cap; the item loops over the head's column tiles itself, because the dot products with g
// need every column of the head.  Pass 1 is the forward's: the shift M over the source's OWN
// neighbours.  Pass 2 is the forward's with the split: A+ = sum p+ z, A- = sum p- z on the matrix units
// (fp32: eight 16x16x4_f32 steps per chunk; 16 bits: v_mfma_f32_16x16x32_{bf16,f16}), ONE B read shared
// by the wave's two runs and by both fragments, the zero-word skip kept; l+ = sum p+, l- = sum p- of the
// same rounded values, per lane in increasing c on the FIRST column tile only, then the four lane
// groups in order; l = fl(fl(l+ + l-) + p_0), den = MaskAttDenominator(l).
// EPILOGUE in the accumulator layout.  g, root and the saved out are read from global memory.  Per row
// the lane adds, over its fragments and column tiles in increasing column, each step one fp32 rounding:
//     dA += g * fl(fl(A+ + A-) + fl(p_0 root))     dS += g * fl(A+ + fl(slope A-))     dR += g * root
// then the 16 column lanes are summed by exchanges at lane distance 1, 2, 4, 8 in that order, and
//     D       = dA / den
//     d s_root = fl(fl(p_0 lambda_0) fl(dR - D)) / den
//     d s_src  = fl(dS - fl(D fl(l+ + fl(slope l-)))) / den + d s_root
//     d root   = g | fl(fl(p_0 / den) g), one rounding to root's dtype
// STATISTICS.  The kernel writes fp32 [batch * n, H, 4] for kernel 2: s_src, M, den, D / den.
//
// KERNEL 2, CANDIDATE-MAJOR, over mask_t = mask_transpose(mask): a lane's row is a candidate and
// carries its s_nb[c, h]; the contraction runs over the batch row's sources in blocks.  Per source
// block the workgroup stages s_src_i, M_i and D_i / den_i from the statistics (3 floats per source
// beside the tile) and, as the B operand, the gated gradient of the head's columns divided by its
// source's den: ONE correctly rounded division, ONE rounding to the operand type (z's dtype; fp32
// kept), transposed in registers exactly like z in the forward.  p_ic = bit ? exp2(fl(fl(e_ic - M_i)
// log2e)) : +0 with the forward's arithmetic and rounding, split by the sign of a_ic:
//     P+- = sum_i p+-_ic G~_i  (matrix units)      W+- = sum_i p+-_ic (D_i / den_i)
// W per lane in increasing i on the first column tile only, then the four lane groups in order.
// EPILOGUE:  d z[c] = fl(P+ + P-), one rounding to z's dtype;  d s_nb[c] = dot - fl(W+ + fl(slope W-)),
// where dot adds z_c[col] * fl(P+ + fl(slope P-)) over the lane's fragments and tiles in increasing
// column (z re-read from global memory) and then over the 16 column lanes at distance 1, 2, 4, 8.
//
// EDGES.  A source without neighbours and without s_root has M = -inf, every p selected to +0, l = 0,
// den = 1: it contributes exactly +0 to every gradient; leaky and exp2 of its shift are never used
// unselected.  A non-neighbour's p is removed by a select, in both kernels.  m == 0: no mask is read,
// kernel 2 is not launched, d root is the gated grad in both root forms and the score gradients are +0.
// batch * n == 0 touches nothing.  At a pre-activation of exactly 0 lambda is 1, AttAdditiveGrad's
// choice (mp_attention.h); torch's leaky_relu takes the slope there.
// DETERMINISM.  Every sum has the one order stated above; a source sees only its own mask row and its
// batch row's candidates and vice versa: the same bits on every run, on every stream and under any
// split of the batch.
// COLUMN TILE: NT <= 2 (32 columns), where the forward has 4: two accumulator sets per run double
// the accumulator registers, and the carried dot products need registers beside them.
// LDS: the forward's tile and scores at NT <= 2; kernel 2 holds three score arrays (3 KB at KB = 256).
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "mp_mask_attention.h"

namespace euler_gpu {

constexpr int kMaskAttBwdMaxNt = 2;       // 32 columns per column tile
constexpr int kMaskAttStats = 4;          // floats per (source, head): s_src, M, den, D / den

// k: the extent of the contraction (m for kernel 1, n for kernel 2); scores: staged arrays of kb floats
inline MaskAttPlan MaskAttBwdMakePlan(int64_t k, int64_t dh, bool f32, int32_t scores) {
  const int64_t tile = 16 * kMaskAttBwdMaxNt;
  const MaskPlan x = MaskMakePlan(k, dh < tile ? dh : tile, f32);      // nt <= kMaskAttBwdMaxNt
  MaskAttPlan p{};
  p.nt = x.nt;
  p.col_tiles = (int32_t)((dh + 16 * p.nt - 1) / (16 * p.nt));
  p.kb = x.kb;
  p.stride = x.stride;
  p.score_off = x.lds_bytes;
  p.lds_bytes = p.score_off + scores * p.kb * 4;
  return p;
}

}  // namespace euler_gpu
