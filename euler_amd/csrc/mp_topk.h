// Per-column top-k over the gathered rows of a segment - the step of the reference's LGCEncoder
// (tf_euler/python/utils/encoders.py:872-922; lines 911-914: get_dense_feature, reshape
// [B, nb, d], transpose, tf.nn.top_k, transpose): the arithmetic of ONE LANE, shared by the
// kernels of segment_topk_kernels.hip and by tests/csrc/segment_topk_check.cc, which compiles this
// file with the host compiler.  A top-k is a pure selection: nothing here rounds, so host and
// device return the same bits by construction.
//
// For destination r, the candidate positions p of its segment in segment order, and column c:
// SEGMENT FORMS: p runs over seg_ptr[r] .. seg_ptr[r + 1], or over r * count .. (r + 1) * count.
// CANDIDATE VALUE: params[g[p]][c], widened exactly to fp32; g[p] is an int32 index, the full
// signed int64 id a sampler returned (compared in 64 bits, not its low word), or p itself when
// no gather array is given.
// RANGE RULE (that of kg_score.h): an index outside [0, params_rows) names no row and is never
// dereferenced.  It reads as a row of +0 and DOES take part as a candidate - a default_node
// fill's feature row is zeros in the reference, and those zeros enter top_k.  The gradient to
// such a candidate is dropped.
// ORDER: a precedes b iff a > b, or a is NaN and b is not (NaN greatest, as torch.topk);
// otherwise the earlier position precedes - a stable sort.  +0 and -0 compare equal, any two
// NaNs compare equal.
// OUTPUT: out[r][j][c] = the j-th candidate in that order for j < min(k, len), layout
// [size, k, d] (what the reference has after its second transpose); sel[r][j][c] = that
// candidate's global position p (int32).  For j >= len: out = fill (an fp32 argument, rounded
// once to the output dtype) and sel = -1.
// STORAGE: params fp32 / bf16 / fp16; out fp32 or the input dtype.  The stored value is the
// project's narrowing (half_cvt.h) of the exactly widened candidate: the original bits for every
// non-NaN, a NaN for a NaN.
// LIMITS: 1 <= k <= 16, e < 2^31, exactly one of seg_ptr / count.  size == 0 or d == 0 touches
// nothing.
//
// THE INSERTION of one candidate into a lane's list of K slots is a STICKY SHIFT: walking
// j = 0 .. K - 1, shift |= (j >= seen) | precedes(candidate, slot[j]); from the first slot where
// shift is set on, the carried value and the slot swap at EVERY slot.  (A chain of independent
// compare-swaps that re-tests every slot is wrong: for [2.5, 2.5, +inf], k = 2 the displaced
// 2.5@0 fails `>` against 2.5@1 and falls off; the answer is positions (2, 0).)  `seen` is the
// number of candidates inserted before: slots j >= seen are empty.
//
// GRADIENT: per_edge [e, d] fp32 is +0 everywhere except per_edge[sel[r][j][c]][c] =
// grad[r][j][c] for sel >= 0; a candidate is selected at most once per column, so every element
// has at most one writer.  The table gradient is the scatter-add of per_edge by the gather keys,
// keys outside [0, params_rows) left out.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "half_cvt.h"
#include "kg_score.h"
#include "mp_weighted.h"

namespace euler_gpu {

constexpr int kTkMaxK = 16;

// a precedes b by value alone (ties are broken by position: the insertion keeps the earlier first)
EG_MPW_HD bool TkPrecedes(float a, float b) { return !(a <= b) & (b == b); }

// The template capacity that serves k: 1, 2, 4, 8 or 16
inline int32_t TkCapacity(int32_t k) {
  int32_t cap = 1;
  while (cap < k) cap *= 2;
  return cap;
}

// Do the value (and, with positions, the position) slots of a lane of width v fit 64 registers?
// The one statement of the cap: TkChunkWidth lowers V by it and the dispatch instantiates only
// the kernels that pass it (V = 1 always does).
constexpr bool TkFits(int32_t v, int32_t cap, bool positions) { return v == 1 || v * cap * (positions ? 2 : 1) <= 64; }

// V, the adjacent columns of a lane: the alignment and divisibility rule of KgChunkWidth over
// params and out (sel, int32, must start on a 16-byte boundary for V > 1), then lowered until
// TkFits holds.
inline int32_t TkChunkWidth(int64_t d, uintptr_t params, bool params_f32, uintptr_t out, bool out_f32,
                            uintptr_t sel, int32_t cap) {
  int32_t v = KgChunkWidth(d, params, params_f32, out, out_f32);
  if (sel % 16 != 0) v = 1;
  while (!TkFits(v, cap, sel != 0)) v = v == 8 ? 4 : 1;
  return v;
}

// The table row of position p (gather: nullptr, int32 [e] or int64 [e] by is_ids); -1 when the
// range rule removes it.
EG_MPW_HD int64_t TkRow(const void* gather, int32_t is_ids, int64_t p, int64_t rows) {
  int64_t g = p;
  if (gather) g = is_ids ? static_cast<const int64_t*>(gather)[p] : (int64_t)static_cast<const int32_t*>(gather)[p];
  return KgInRange(g, rows) ? g : -1;
}

// [begin, end) of destination r, kept inside [0, e]
EG_MPW_HD void TkSegment(const int64_t* seg_ptr, int64_t count, int64_t e, int64_t r, int64_t* begin, int64_t* end) {
  int64_t b = seg_ptr ? seg_ptr[r] : r * count, en = seg_ptr ? seg_ptr[r + 1] : (r + 1) * count;
  b = b < 0 ? 0 : (b > e ? e : b);
  en = en < b ? b : (en > e ? e : en);
  *begin = b;
  *end = en;
}

// One candidate (value v at position p; live = false: not a candidate, nothing changes) into the
// list slot[0 .. K) / pos[0 .. K) that holds `seen` candidates.  SEL = false: positions are not
// tracked (pos may be nullptr).  Fully unrolled: no array is indexed at run time.
template <int K, bool SEL>
EG_MPW_HD void TkInsert(bool live, float v, int32_t p, int32_t seen, float* slot, int32_t* pos) {
  bool shift = false;
EG_MPW_UNROLL
  for (int j = 0; j < K; ++j) {
    shift |= live & ((j >= seen) | TkPrecedes(v, slot[j]));
    const float t = slot[j];
    slot[j] = shift ? v : t;
    v = shift ? t : v;
    if constexpr (SEL) {
      const int32_t q = pos[j];
      pos[j] = shift ? p : q;
      p = shift ? q : p;
    }
  }
}

// An element as its bits in a uint32 (fp32: all 32, 16-bit types: the low 16), widened exactly
template <int DT>
EG_MPW_HD float TkWiden(uint32_t raw) {
  if constexpr (DT == kF32) return BitsF32(raw);
  else return HalfCvt<DT>::Widen((uint16_t)raw);
}

// The stored form of a list entry: fp32 as it is, else the project's narrowing
template <int DT>
EG_MPW_HD uint32_t TkStored(float f, bool out_f32) {
  if constexpr (DT == kF32) return F32Bits(f);
  else return out_f32 ? F32Bits(f) : (uint32_t)HalfCvt<DT>::Narrow(f);
}

}  // namespace euler_gpu
