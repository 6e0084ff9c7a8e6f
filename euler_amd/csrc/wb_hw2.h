// "Header + window" lines with 12-bit offsets ("HW2"): a second encoding of the side lines of
// wb_hw.h, read by hop 2 of the plain-graph fanout step with TWO requests per draw.
//
// wb_hw.h quantises the sums of a line's first eight entries into 8 bits over the line's own
// range, so a draw shares a quantum with a boundary - and guesses one entry too high - about
// once in a hundred; a wave carries 128 draws, so nine waves in ten have such a lane, and the 12
// bytes before the window are fetched for EVERY draw.  Here the offsets take 12 bits and run
// over the BUCKET's span instead of the line's: a draw that maps to bucket j has
// x = f * scale in [j, j + 1) (WbBucketOf), and x - j - exact, no load, no division beyond the
// scale's - is its position inside the bucket.  Same 128-byte line, same buckets
// (WbBuckets, WbScale, WbBucketOf, WbBlockStart) and the same wb_lo as wb_hw.h; only the words
// 0 .. 2 differ:
//
//   words 0..2     c[8]   u12   c[k] = Hw2Code(sum[k] * scale - j) of entries 0 .. 7 (96 bits,
//                               little-endian: code k at bit 12 k); 4095 past the row's end
//   word  3        the exact running sum before entry 0 (0 at the row's start)
//   words 4+3i ..  entry i = {id (2 words), sum (f32)}, i = 0 .. 8, as in wb_hw.h
//   word  31       the flat index of entry 0 (not read by the draw)
//
//   Hw2Code(v):    0 for v < 0 (sums below the bucket's span) and for NaN, floor(v * 4094)
//                  clamped to 4093 for v < 1, 4094 for v >= 1 (sums at or above the span's end)
//
//   draw:  header (words 0..3)  ->  t = Hw2Code(f * scale - j)
//          guess i = #{k < 8 : c[k] <= t}                                 (0 .. 8)
//          window i             ->  accept iff !(before > f) && sum > f   (HwCheck)
//          Builder and draw run the SAME operations on sum[k] and on f, each of them monotone,
//          so sum[k] <= f implies c[k] <= t: a guess is never too low.  It is one too high when
//          f shares a quantum with the next boundary - 1/4094 of the bucket per boundary, about
//          four boundaries per bucket: ~5e-4 of the draws on i.i.d. weights.  Such a draw (window
//          i says "before", i > 0) loads window i - 1 in a second dependent trip; with one wave
//          in ten asking, that is ~0.1 trip per wave-step where wb_hw.h pays a third request per
//          draw.  Anything else is COLD: the caller replays RandomSelect.
//
// The keys decide, never the layout (wb_hw.h): an accepted entry is the first edge of the row
// whose running sum exceeds f, whatever the header guessed.
//
// Everything here is __host__ __device__ per item: tests/csrc/hw2_check.hip runs the same
// source on the CPU against the oracle (`pytest -m "not gpu"`).
#ifndef EULER_AMD_CSRC_WB_HW2_H_
#define EULER_AMD_CSRC_WB_HW2_H_

#include "wb_hw.h"

namespace euler_gpu {

constexpr uint32_t kHw2In = 4093;        // largest code of a sum inside the bucket's span
constexpr uint32_t kHw2Max = 4094;       // sums at or above the span's end
constexpr uint32_t kHw2Pad = 4095;       // past the row's end

// the 12-bit code of the position v = x * scale - j (in buckets) of a running sum or a draw
EG_HD uint32_t Hw2Code(float v) {
  const float m = EG_FMUL(v, (float)kHw2Max);
  const uint32_t q = !(m >= 0.f) ? 0u : (m < (float)kHw2Max ? (uint32_t)m : kHw2In);
  return v >= 1.f ? kHw2Max : q;
}

// position of the (rounded-down) draw or running sum x inside bucket j
EG_HD float Hw2Pos(float x, float scale, uint32_t j) { return EG_FSUB(EG_FMUL(x, scale), (float)j); }

// Line of bucket j of a row, as HwBuildLine.  Returns true when the bucket OVERFLOWS its line.
EG_HD bool Hw2BuildLine(const float* prefix_w, const uint64_t* nbr, uint32_t lo, uint32_t deg,
                        float total, uint32_t j, HwLine* out) {
  const uint32_t nbk = WbBuckets(deg);
  const ArraySum nw{prefix_w + lo};
  const float scale = WbScale(nbk, total);
  const uint32_t s = WbBlockStart(nw, deg, nbk, scale, j);
  bool overflow = false;
  if (s + kHwEntries < deg) {
    if (j + 1u >= nbk) {
      overflow = true;                       // the row goes on past the line
    } else {
      const double U = ((double)(j + 1u) / (double)scale) * (1.0 + 1.0 / 1048576.0);
      overflow = !((double)nw(s + kHwEntries - 1u) > U);
    }
  }
  uint64_t c01 = 0ull;                       // codes 0 .. 4 (60 bits) and the low 4 bits of code 5
  uint32_t c2 = 0u;                          // the rest
  for (uint32_t k = 0; k < 8u; ++k) {
    const uint32_t v = s + k < deg ? Hw2Code(Hw2Pos(prefix_w[lo + s + k], scale, j)) : kHw2Pad;
    const uint32_t at = 12u * k;
    if (at < 64u) c01 |= (uint64_t)v << at;
    if (at + 12u > 64u) c2 |= at >= 64u ? v << (at - 64u) : v >> (64u - at);
  }
  out->w[0] = (uint32_t)c01; out->w[1] = (uint32_t)(c01 >> 32); out->w[2] = c2;
  out->w[3] = HwAsBits(s == 0u ? 0.f : prefix_w[lo + s - 1u]);
  for (uint32_t k = 0; k < kHwEntries; ++k) {
    const uint32_t m = s + k;
    const bool in = m < deg;
    const uint64_t id = in ? nbr[lo + m] : 0ull;
    out->w[4u + 3u * k] = (uint32_t)id;
    out->w[5u + 3u * k] = (uint32_t)(id >> 32);
    out->w[6u + 3u * k] = HwAsBits(in ? prefix_w[lo + m] : __builtin_huge_valf());
  }
  out->w[31] = lo + s;
  return overflow;
}

struct alignas(16) Hw2Head { uint32_t c0, c1, c2, base; };

EG_HD Hw2Head Hw2LoadHead(const HwLine* ln) { return *reinterpret_cast<const Hw2Head*>(ln->w); }

// the ONE candidate entry a header names for a draw of code t
EG_HD uint32_t Hw2Guess(const Hw2Head& h, uint32_t t) {
  uint32_t i = 0;
  i += (h.c0 & 4095u) <= t ? 1u : 0u;
  i += ((h.c0 >> 12) & 4095u) <= t ? 1u : 0u;
  i += ((h.c0 >> 24) | ((h.c1 & 15u) << 8)) <= t ? 1u : 0u;
  i += ((h.c1 >> 4) & 4095u) <= t ? 1u : 0u;
  i += ((h.c1 >> 16) & 4095u) <= t ? 1u : 0u;
  i += ((h.c1 >> 28) | ((h.c2 & 255u) << 4)) <= t ? 1u : 0u;
  i += ((h.c2 >> 8) & 4095u) <= t ? 1u : 0u;
  i += (h.c2 >> 20) <= t ? 1u : 0u;
  return i;
}

// One draw of code t on a line.  Returns 1 when the guessed entry is the answer, 2 when the
// entry before it is (a second window); cold: -1 after one window (it said "after", or "before"
// at entry 0), -2 after two.
EG_HD int32_t Hw2Draw(const HwLine* ln, float f, uint32_t t, uint64_t* id, float* w) {
  const uint32_t i = Hw2Guess(Hw2LoadHead(ln), t);
  const int32_t d = HwCheck(HwLoadWin(ln, i), f, id, w);
  if (d == 0) return 1;
  if (d > 0 || i == 0u) return -1;
  return HwCheck(HwLoadWin(ln, i - 1u), f, id, w) == 0 ? 2 : -2;
}

// The hot part of one draw, as HwSampleHot: false = cold.  *windows = Hw2Draw's answer, or 0 when
// no line was read (r rounded up to the row's total).
EG_HD bool Hw2SampleHot(const HwLine* hw, const WbRec& rec, double u, uint64_t* id, float* w,
                        int32_t* windows) {
  const double r = EG_DMUL(u, (double)rec.total);
  *windows = 0;
  if (!((double)rec.total > r)) return false;
  const float f = WbFloorToFloat(r);
  const uint32_t nbk = WbBuckets(rec.deg);
  const float scale = WbScale(nbk, rec.total);
  const uint32_t j = nbk <= 1u ? 0u : WbBucketOf(f, nbk, scale);
  *windows = Hw2Draw(hw + rec.wb_lo + j, f, Hw2Code(Hw2Pos(f, scale, j)), id, w);
  return *windows > 0;
}

}  // namespace euler_gpu

#endif  // EULER_AMD_CSRC_WB_HW2_H_
