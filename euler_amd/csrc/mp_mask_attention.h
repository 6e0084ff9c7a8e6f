// Layerwise attention aggregation straight from the bit mask - the reference's AttentionAggregator
// (tf_euler/python/utils/sparse_aggregators.py:87-139: SingleAttentionAggregator per head, concatenated;
// the default aggregator of GenieEncoder) over the [batch, n, m] adjacency of a layerwise sample, read as
// the uint64 hit mask of mp_mask.h, in ONE launch on the matrix units.  No COO triple, no nnz, no host
// wait, no atomics, and no [n, m] block of logits in memory.  This file states the contract and holds
// the tile plan; the host entry, the kernel (mask_attention_kernels.hip) and a host-only program can
// all include it.
//
// With H heads, d = H * dh, batch row b, source i, head h and N(b,i) the set bits c < m of mask[b*n + i]:
//
//     e_c   = leaky(s_src[b*n+i, h] + s_nb[b*m+c, h])             c in N(b,i)
//     e_0   = leaky(s_src[b*n+i, h] + s_root[b*n+i, h])           only with s_root (renorm=True: the eye column)
//     alpha = softmax over {e_c} (and e_0)
//     A     = sum_c alpha_c * z[b*m+c, h*dh : (h+1)*dh]  (+ alpha_0 * root[b*n+i, the same columns])
//     out   = A              with s_root                          (renorm=True)
//           = root + A       with root and no s_root              (renorm=False: from_self + output)
//           = A              with neither
//     then relu if asked, ONE rounding to the output dtype.
//
// ARGUMENTS.  mask as in mp_mask.h; stray bits at positions >= m are ignored.  z [>= batch*m, d] fp32 /
// bf16 / fp16, contiguous: the projected candidate rows (the dense layer stays a GEMM outside).  s_src
// [batch*n, H] and s_nb [>= batch*m, H] fp32: the two halves of the additive logit.  root [batch*n, d]
// of z's dtype, optional; s_root [batch*n, H] fp32, optional and only with root.  negative_slope >= 0
// (leaky must be monotone for the shift below; 1.0 is the identity).  out fp32 or z's dtype.
// ARITHMETIC.  leaky(a) = a < 0 ? fl(a * slope) : a on a = fl(s_src + s), AttAdditiveLogit of
// mp_attention.h.
// SHIFT.  leaky and the rounded add are monotone in s, so M = leaky(s_src + max_{c in N} s_nb[c]) IS the
// largest e_c; with s_root, M = max(M, e_0).  A source with no neighbour has M = e_0, or -inf without
// s_root: leaky is never applied to -inf (slope 0 would make it NaN).  The max runs over the source's
// OWN neighbours, never over all candidates of the batch row: a large score on a non-neighbour does
// not underflow the real terms.
// OPERAND.  p_c = bit ? exp2(fl(fl(e_c - M) * log2e)) : +0 - a SELECT, not a product with the bit: a
// non-neighbour's exp may be inf.  exp2 is the hardware instruction (v_exp_f32; results below 2^-126 are
// +0).  Each p_c is rounded ONCE to the operand type of the matrix instruction, z's dtype (fp32: kept).
// DENOMINATOR.  l sums the SAME rounded p_c in fp32 in a fixed order: per lane in increasing c, then the
// four lane groups in order.  The weights therefore sum to one over what was actually multiplied.  The
// products accumulate in fp32 in the order of mp_mask.h (the chunks of 32 candidates in increasing c).
// SELF TERM.  p_0 = exp2(fl(fl(e_0 - M) * log2e)) enters in the epilogue in fp32, unrounded:
// acc = fl(acc + fl(p_0 * root)), l = fl(l + p_0).
// DIVISION.  ONE correctly rounded division acc / l (l == 0: by 1, so a source with no neighbour and no
// s_root has A = +0, what tf.sparse_softmax gives for an empty row); then the root add of the root-only
// form, then relu (x <= 0 ? +0 : x, NaN stays), then the narrowing.
// With all scores 0 every p is exactly 1 and l is the degree: the result then has the BITS of
// mask_aggregate's mean (neither root nor s_root), gcn (root) and gcn_renorm (root and s_root).
// NON-FINITE z: 0 * inf and 0 * NaN are NaN, so a non-finite z[b*m + c, f] makes column f NaN for the
// sources of batch row b whether c is their neighbour or not, as in mp_mask.h (a run of 16 sources
// with no bit in c's word of 64 is spared by the zero-word skip).
// DETERMINISM.  The same bits on every run, on every stream and under any split of the batch: a source
// sees only its own mask row, its own scores and its batch row's candidates.
// LIMITS.  batch*n < 2^31, batch*m < 2^31, 1 <= d <= 1024, H >= 1 divides d.  batch*n == 0 touches
// nothing; m == 0 reads neither mask, z nor s_nb and writes root (either root form) or zeros.
//
// THE TILING (MaskAttPlan below is its one statement; roles, fragments, staging and the Xt swizzle are
// those of mp_mask.h).
// WORK ITEM = (batch row, source tile, head, column tile of that head), head and column tile fastest,
// on a capped grid with a loop beyond the cap.  A 16-column fragment never straddles two heads: a
// head's dh columns are padded to 16 NT per column tile; staged columns >= dh of the head are +0 and
// are not stored.  16-byte loads where z starts on a 16-byte boundary and dh % 8 == 0 (fp32: % 4) -
// the rule of mp_mask.h with dh for d; element loads otherwise.
// COLUMN TILE: NT <= 4 (64 columns), not mask_aggregate's 8.  The head's score block needs LDS beside
// the 64 KB an NT = 8 tile of 256 candidates takes, and the p pipeline (8 scores, 8 p and a partial l
// per run) needs registers beside the accumulators; heads wider than 64 columns take further tiles
// and evaluate p once per tile.
// PASS 1 (SHIFT).  Per candidate block the workgroup stages the head's s_nb slice (4 bytes per
// candidate, blocked like the candidates) and every wave walks its sources' mask words: lane (source
// l % 16, group l / 16) takes the same 8 candidates per chunk of 32 as in pass 2 and keeps a running
// max by select; the four groups are combined by lane exchange.  Nothing is multiplied.
// PASS 2.  Per candidate block: the z tile staged transposed in 16-byte units (fp32: row-major) and the
// block's s_nb; per chunk each lane turns its mask byte and eight scores into an A fragment of eight p
// (add, leaky, subtract, scale, exp2, select, pack to 16 bits), adds the eight rounded p to its partial
// l, and the chunk issues v_mfma_f32_16x16x32_{bf16,f16} (fp32: eight 16x16x4_f32, instruction j on
// candidate 4 j + l / 16) with ONE B read shared by the wave's two runs.  The zero-word skip is kept.
// EPILOGUE in the accumulator layout: l, M and p_0 of a lane's four rows fetched by lane index; self
// term, division, root add, relu, narrowing, store.  No LDS round trip.
// LDS BUDGET: 33 KB (16 bits: 64 columns x 256 candidates + 1 KB of scores); fp32 20.25 KB.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "mp_attention.h"
#include "mp_mask.h"

namespace euler_gpu {

constexpr int kMaskAttMaxNt = 4;          // 64 columns per column tile
constexpr int kMaskAttNone = 0, kMaskAttRelu = 1;
constexpr float kMaskAttLog2e = 1.44269504088896340736f;

struct MaskAttPlan {
  int32_t nt;         // accumulator fragments per run: the column tile is 16 * nt
  int32_t col_tiles;  // column tiles of ONE head
  int32_t kb;         // candidates per block, a multiple of 64
  int32_t stride;     // bytes between the columns of Xt (16 bits) / the rows of X (fp32)
  int32_t score_off;  // byte offset of the block's scores: float [kb]
  int32_t lds_bytes;  // dynamic LDS of a workgroup
};

inline MaskAttPlan MaskAttMakePlan(int64_t m, int64_t dh, bool f32) {
  const int64_t tile = 16 * kMaskAttMaxNt;
  const MaskPlan x = MaskMakePlan(m, dh < tile ? dh : tile, f32);      // nt <= kMaskAttMaxNt
  MaskAttPlan p{};
  p.nt = x.nt;
  p.col_tiles = (int32_t)((dh + 16 * p.nt - 1) / (16 * p.nt));
  p.kb = x.kb;
  p.stride = x.stride;
  p.score_off = x.lds_bytes;
  p.lds_bytes = p.score_off + p.kb * 4;
  return p;
}

// the divisor of the one division: l, or 1 where nothing was summed (a NaN stays a NaN)
EG_MPW_HD float MaskAttDenominator(float l) { return l == 0.f ? 1.f : l; }

}  // namespace euler_gpu
