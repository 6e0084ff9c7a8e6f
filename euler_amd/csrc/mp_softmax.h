// The softmax over the updates of one destination (edge_softmax): the arithmetic of ONE
// (segment, head), shared by the kernels of edge_softmax_kernels.hip and by
// tests/csrc/edge_softmax_check.cc, which compiles this file with the host compiler.  Every
// operation is a correctly rounded fp32 add, multiply or divide (the __f*_rn intrinsics on the
// device, plain operators in a translation unit built with -ffp-contract=off on the host), an
// integer operation or a comparison: host and device return the same bits by construction.
//
// FORWARD of the n logits x_0 .. x_{n-1} of a (segment, head), widened to fp32:
//   m = max_p x_p,  d_p = fl(x_p - m),  e_p = ExpNonPositive(d_p),  s = SUM e_p,  y_p = fl(e_p / s)
// BACKWARD, given the forward's y and the incoming g:
//   t = SUM fl(y_q * g_q),  gx_p = fl(y_p * fl(g_p - t))
// No "online" rescaling: the maximum is known before the first exponential is taken.
//
// SUMMATION ORDER of SUM (a function of n and of heads alone - never of e, size, the grid, the
// storage type or the segment form).  Every sum starts from +0 and adds its terms one by one.
//   n <= kSmxShort (32):  the terms in increasing p.
//   n >  kSmxShort:       W = 256 / hc partial sums, hc = SmxHeadsPerWave(heads) (heads when heads
//                         divides 64, else 1).  Partial l adds the terms p = l, l + W, l + 2 W, ...
//                         in increasing p (SmxLaneExpSum / SmxLaneDotSum).  Combine tree: the W
//                         partials are cut into 4 runs of W / 4 adjacent ones; inside a run a
//                         butterfly, for off = W / 8, W / 16, ..., 1:  s_l = s_l + s_(l ^ off);
//                         then the four run sums as (S0 + S1) + (S2 + S3) (SmxCombine4).
// (The kernels give a run to each wave of a 256-thread block.)  The maximum is exact whatever its
// order is.
//
// Outside the contract: a segment whose maximum is not finite.  All -inf, or a +inf: every d_p
// is -inf or NaN, every e_p is 0, s is 0 and every y_p is NaN (0 / 0).  A NaN logit never wins a
// comparison and every fold of the maximum starts from -inf (short and long alike), so it is left
// out of the maximum, and its own e_p and y_p are 0.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "half_cvt.h"
#include "mp_weighted.h"

namespace euler_gpu {

constexpr int kSmxShort = 32;          // the longest segment one lane keeps in registers
constexpr int kSmxBlock = 256;         // lanes that share a longer segment: 4 runs of 64
// T: below it ExpNonPositive returns +0.  exp(-86) = 2^-124.07: every result, and every
// intermediate, is a NORMAL fp32 number - nothing depends on how denormals are handled.
constexpr float kSmxExpFloor = -86.0f;

EG_MPW_HD int32_t SmxHeadsPerWave(int32_t heads) { return (heads <= 64 && 64 % heads == 0) ? heads : 1; }

// The grid of a kernel over the segments longer than kSmxShort (host; size > 0): x = chunks of kSmxBlock
// destinations, at most 256 * 32 (the chunks are strided); y = blocks that share the long
// destinations of a chunk - few destinations: more blocks a chunk.  edge_softmax and
// segment_attention both launch by it: the two walk the long segments with the same lanes, and the
// summation order above must stay a function of n and heads alone in both.
struct SmxLongGrid { unsigned chunks, share; };
inline SmxLongGrid SmxLongGridFor(int32_t size) {
  int64_t chunks = ((int64_t)size + kSmxBlock - 1) / kSmxBlock;
  if (chunks > 256 * 32) chunks = 256 * 32;
  int64_t share = 2048 / chunks;
  share = share < 1 ? 1 : (share > 16 ? 16 : share);
  return SmxLongGrid{(unsigned)chunks, (unsigned)share};
}

EG_MPW_HD float SmxSub(float a, float b) { return MpwAdd(a, -b); }       // fl(a - b)
EG_MPW_HD float SmxMax(float m, float x) { return x > m ? x : m; }
EG_MPW_HD float SmxNegInf() { return BitsF32(0xff800000u); }

// exp(d) for d <= 0: +0 below kSmxExpFloor (and for -inf and NaN), exactly 1 at 0.
//   k = round(d * log2(e)), by adding and subtracting 1.5 * 2^23 (k in [-124, 0]);
//   r = d - k * ln2, ln2 = C1 + C2 with a 9-bit C1, so that k * C1 and d - k * C1 are exact;
//   exp(r) = 1 + (r + r^2 * q(r)), q of degree 5 (fitted on |r| <= 0.3467 to 0.013 ulp of exp);
//   the result is that value with k added to its exponent field.
// Largest error against the real exp over every fp32 d in [kSmxExpFloor, 0]: DESIGN 4.11.
EG_MPW_HD float ExpNonPositive(float d) {
  if (!(d >= kSmxExpFloor)) return 0.f;
  const float magic = 12582912.f;
  const float t = MpwAdd(MpwMul(d, 0x1.715476p+0f), magic);
  const int32_t k = (int32_t)F32Bits(t) - (int32_t)F32Bits(magic);
  const float kf = MpwAdd(t, -magic);
  float r = MpwAdd(d, -MpwMul(kf, 0.693359375f));
  r = MpwAdd(r, -MpwMul(kf, -2.12194440e-4f));
  float q = 0x1.a151a8p-13f;
  q = MpwAdd(MpwMul(q, r), 0x1.6d4352p-10f);
  q = MpwAdd(MpwMul(q, r), 0x1.1110c6p-7f);
  q = MpwAdd(MpwMul(q, r), 0x1.5554e8p-5f);
  q = MpwAdd(MpwMul(q, r), 0x1.555556p-3f);
  q = MpwAdd(MpwMul(q, r), 0.5f);
  const float p = MpwAdd(1.0f, MpwAdd(r, MpwMul(MpwMul(r, r), q)));
  return BitsF32((uint32_t)((int32_t)F32Bits(p) + k * (1 << 23)));
}

EG_MPW_HD float SmxForwardValue(float x, float m, float s) { return MpwDiv(ExpNonPositive(SmxSub(x, m)), s); }
EG_MPW_HD float SmxBackwardValue(float y, float g, float t) { return MpwMul(y, SmxSub(g, t)); }
EG_MPW_HD float SmxCombine4(float a, float b, float c, float d) { return MpwAdd(MpwAdd(a, b), MpwAdd(c, d)); }

// ---- n <= kSmxShort: the whole (segment, head) in the registers of one lane -----------------
// x[0 .. n) in, y[0 .. n) out; 1 <= n <= K.  (Fully unrolled: no register array is indexed by a
// variable.)
template <int K>
EG_MPW_HD void SmxShortForward(const float x[K], int32_t n, float y[K]) {
  float m = SmxNegInf();
EG_MPW_UNROLL
  for (int k = 0; k < K; ++k) if (k < n) m = SmxMax(m, x[k]);
  float s = 0.f;
EG_MPW_UNROLL
  for (int k = 0; k < K; ++k) if (k < n) { y[k] = ExpNonPositive(SmxSub(x[k], m)); s = MpwAdd(s, y[k]); }
EG_MPW_UNROLL
  for (int k = 0; k < K; ++k) if (k < n) y[k] = MpwDiv(y[k], s);
}

template <int K>
EG_MPW_HD void SmxShortBackward(const float y[K], const float g[K], int32_t n, float gx[K]) {
  float t = 0.f;
EG_MPW_UNROLL
  for (int k = 0; k < K; ++k) if (k < n) t = MpwAdd(t, MpwMul(y[k], g[k]));
EG_MPW_UNROLL
  for (int k = 0; k < K; ++k) if (k < n) gx[k] = SmxBackwardValue(y[k], g[k], t);
}

// ---- n > kSmxShort: the fold of partial l of w; ld(p) is term p's logit (y, g), widened ------
// Four loads are issued before their terms are folded in, in increasing p.
template <typename Ld>
EG_MPW_HD float SmxLaneMax(const Ld& ld, int64_t l, int64_t w, int64_t n) {
  float m = SmxNegInf();
  int64_t p = l;
  for (; p + 3 * w < n; p += 4 * w) {
    const float a = ld(p), b = ld(p + w), c = ld(p + 2 * w), d = ld(p + 3 * w);
    m = SmxMax(SmxMax(SmxMax(SmxMax(m, a), b), c), d);
  }
  for (; p < n; p += w) m = SmxMax(m, ld(p));
  return m;
}

template <typename Ld>
EG_MPW_HD float SmxLaneExpSum(const Ld& ld, float m, int64_t l, int64_t w, int64_t n) {
  float s = 0.f;
  int64_t p = l;
  for (; p + 3 * w < n; p += 4 * w) {
    const float a = ld(p), b = ld(p + w), c = ld(p + 2 * w), d = ld(p + 3 * w);
    s = MpwAdd(s, ExpNonPositive(SmxSub(a, m)));
    s = MpwAdd(s, ExpNonPositive(SmxSub(b, m)));
    s = MpwAdd(s, ExpNonPositive(SmxSub(c, m)));
    s = MpwAdd(s, ExpNonPositive(SmxSub(d, m)));
  }
  for (; p < n; p += w) s = MpwAdd(s, ExpNonPositive(SmxSub(ld(p), m)));
  return s;
}

template <typename LdY, typename LdG>
EG_MPW_HD float SmxLaneDotSum(const LdY& ly, const LdG& lg, int64_t l, int64_t w, int64_t n) {
  float t = 0.f;
  int64_t p = l;
  for (; p + 3 * w < n; p += 4 * w) {
    const float y0 = ly(p), y1 = ly(p + w), y2 = ly(p + 2 * w), y3 = ly(p + 3 * w);
    const float g0 = lg(p), g1 = lg(p + w), g2 = lg(p + 2 * w), g3 = lg(p + 3 * w);
    t = MpwAdd(t, MpwMul(y0, g0));
    t = MpwAdd(t, MpwMul(y1, g1));
    t = MpwAdd(t, MpwMul(y2, g2));
    t = MpwAdd(t, MpwMul(y3, g3));
  }
  for (; p < n; p += w) t = MpwAdd(t, MpwMul(ly(p), lg(p)));
  return t;
}

}  // namespace euler_gpu
