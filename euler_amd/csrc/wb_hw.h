// "Header + window" lines ("HW"): a second format for the buckets of the weight-bucket index
// (wb_index.h), read by hop 2 of the plain-graph fanout step with three requests in two trips.
//
// A draw on an EdgeBlock asks for its line four times: three 16-byte key loads, then the
// dependent 8-byte id.  Beyond the ~2 GiB the address-translation caches reach every request
// pays its own translation, and the chip completes 19.5 G such lines/s; one 16-byte load and
// one dependent 16-byte load of the same line run at 26 G (tools/ubench_block.hip, modes 8 / 9).
// Hop 2 needs neither the drawn edge's number nor all ten keys in registers - it needs ONE
// entry's {sum before, id, sum}.  So a side array holds, for bucket j of a row, the line
// hw[wb_lo(row) + j] (the SAME buckets, scale and block start as wb[]: WbBuckets, WbScale,
// WbBucketOf, WbBlockStart - no second row record):
//
//   word  0        invq   f32   quanta per unit of running sum inside the line (0: degenerate)
//   words 1..2     q[8]   u8    q[k] = min(254, floor((sum[k] - base) * invq)) of entries 0 .. 7;
//                               255 past the row's end
//   word  3        base   f32   the exact running sum before entry 0 (0 at the row's start)
//   words 4+3i ..  entry i = {id (2 words), sum (f32)}, i = 0 .. 8: up to NINE consecutive edges
//                               from the first one that reaches into the bucket; past the row's
//                               end sum = +inf, id = 0
//   word  31       the flat index of entry 0 (not read by the draw)
//
// Entry i's exact {sum before, id, sum} is the 4-byte-aligned 16-byte WINDOW at word 3 + 3 i:
// the sum of entry i - 1 (for i = 0 the header's last word) sits right before entry i.
//
//   draw:  header (words 0..3)  ->  t = floor((f - base) * invq) clamped to [0, 254]
//          guess i = #{k < 8 : q[k] <= t}                               (0 .. 8)
//          window i             ->  accept iff !(before > f) && sum > f  (WbPickKeys' compares)
//                                   weight = sum -rn- before
//          The builder quantises with the very operations of the guess and both round down, so
//          sum[k] <= f implies q[k] <= t: a guess is never too LOW, and when f shares a quantum
//          with a boundary it is one too high.  The draw therefore asks, together with window
//          i, for the 12 bytes before it - {sum before, id} of entry i - 1, whose sum is the
//          window's first word - and accepts entry i - 1 by the same test when window i
//          says "before".  Header, then {12 bytes, window} in ONE dependent trip: three
//          requests where a block needs four (a second, dependent window for the lanes whose
//          guess was off makes the whole wave wait a third trip: measured slower).
//          Anything else is COLD: the caller replays RandomSelect over the flat running sums,
//          as for a block that does not bracket its draw.
//
// The keys decide, never the layout: an accepted entry is the first edge of the row whose
// running sum exceeds f (sums are non-decreasing), whatever the header guessed; +inf padding
// cannot be accepted because f < the row's total = the last real sum.  A guess is one too high
// for ~1 % of the draws on i.i.d. uniform weights (1/254 of the line's range per boundary) and
// further off only when several sums share a quantum.  Nine entries
// instead of ten: a row of exactly 10 edges sends the draws of its last edge the cold way, and
// a bucket overflows when more than nine edges reach into it - the builder counts both.
//
// Everything here is __host__ __device__ per item: tests/csrc/hw_check.hip runs the same
// source on the CPU against the oracle (`pytest -m "not gpu"`).
#ifndef EULER_AMD_CSRC_WB_HW_H_
#define EULER_AMD_CSRC_WB_HW_H_

#include "wb_index.h"

namespace euler_gpu {

constexpr uint32_t kHwEntries = 9;
constexpr uint32_t kHwQMax = 254;       // largest quantised offset of a real entry; 255 = padding

struct alignas(128) HwLine { uint32_t w[32]; };
static_assert(sizeof(HwLine) == 128, "HwLine must be one 128-byte line");

struct alignas(16) HwHead { uint32_t invq, q0, q1, base; };
// 16 bytes at a 4-byte boundary (one request; gfx950 loads them with one dwordx4)
struct __attribute__((packed, aligned(4))) HwWin { uint32_t before, id_lo, id_hi, sum; };

EG_HD float HwAsFloat(uint32_t x) { return __builtin_bit_cast(float, x); }
EG_HD uint32_t HwAsBits(float x) { return __builtin_bit_cast(uint32_t, x); }

// Line of bucket j of a row (lo = first flat edge, deg > 0 edges, total = last running sum).
// Returns true when the bucket OVERFLOWS its line: some draw that maps to bucket j has its
// answer beyond the nine entries (it will take the cold path).
EG_HD bool HwBuildLine(const float* prefix_w, const uint64_t* nbr, uint32_t lo, uint32_t deg,
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
  const float base = s == 0u ? 0.f : prefix_w[lo + s - 1u];
  // the quantum: 254 steps from base to the sum of the last real entry among the first eight
  const uint32_t nreal = deg - s < 8u ? deg - s : 8u;
  const float range = EG_FSUB(prefix_w[lo + s + nreal - 1u], base);
  float invq = EG_FDIV((float)kHwQMax, range);
  if (!(invq > 0.f) || !(invq < __builtin_huge_valf())) invq = 0.f;   // range 0 / NaN / tiny
  uint32_t q[2] = {0u, 0u};
  for (uint32_t k = 0; k < 8u; ++k) {
    uint32_t v = 255u;
    if (s + k < deg) {
      const float t = EG_FMUL(EG_FSUB(prefix_w[lo + s + k], base), invq);
      v = !(t >= 0.f) ? 0u : (t < (float)kHwQMax ? (uint32_t)t : kHwQMax);
    }
    q[k >> 2] |= v << (8u * (k & 3u));
  }
  out->w[0] = HwAsBits(invq); out->w[1] = q[0]; out->w[2] = q[1]; out->w[3] = HwAsBits(base);
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

EG_HD HwHead HwLoadHead(const HwLine* ln) { return *reinterpret_cast<const HwHead*>(ln->w); }

// the 12 bytes before window i: {sum before, id} of entry i - 1 (for i = 0: header words, unused)
struct __attribute__((packed, aligned(4))) HwPre { uint32_t before, id_lo, id_hi; };
EG_HD HwPre HwLoadPre(const HwLine* ln, uint32_t i) {
  return *reinterpret_cast<const HwPre*>(ln->w + 3u * i);
}

EG_HD HwWin HwLoadWin(const HwLine* ln, uint32_t i) {
  return *reinterpret_cast<const HwWin*>(ln->w + 3u + 3u * i);
}

// the ONE candidate entry a header names for the (rounded-down) draw f
EG_HD uint32_t HwGuess(const HwHead& h, float f) {
  const float t = EG_FMUL(EG_FSUB(f, HwAsFloat(h.base)), HwAsFloat(h.invq));
  const uint32_t ti = !(t >= 0.f) ? 0u : (t < (float)kHwQMax ? (uint32_t)t : kHwQMax);
  uint32_t i = 0;
  i += ((h.q0) & 255u) <= ti ? 1u : 0u;
  i += ((h.q0 >> 8) & 255u) <= ti ? 1u : 0u;
  i += ((h.q0 >> 16) & 255u) <= ti ? 1u : 0u;
  i += (h.q0 >> 24) <= ti ? 1u : 0u;
  i += ((h.q1) & 255u) <= ti ? 1u : 0u;
  i += ((h.q1 >> 8) & 255u) <= ti ? 1u : 0u;
  i += ((h.q1 >> 16) & 255u) <= ti ? 1u : 0u;
  i += (h.q1 >> 24) <= ti ? 1u : 0u;
  return i;
}

// A window against the draw: 0 = its keys bracket f (id / weight set), -1 = the answer lies
// before the entry, +1 = after it.
EG_HD int32_t HwCheck(const HwWin& x, float f, uint64_t* id, float* w) {
  // (no early return: every word of the window is used on every path, so it stays ONE load)
  const float before = HwAsFloat(x.before), sum = HwAsFloat(x.sum);
  const int32_t d = before > f ? -1 : (!(sum > f) ? 1 : 0);
  *id = d == 0 ? ((uint64_t)x.id_lo | ((uint64_t)x.id_hi << 32)) : *id;
  *w = d == 0 ? EG_FSUB(sum, before) : *w;
  return d;
}

// The guessed window and the 12 bytes before it against the draw: 0 = entry i or entry i - 1
// brackets f (id / weight set), else HwCheck's answer for window i.  Entry i - 1's window is
// {pre.before, pre.id, win.before}.
EG_HD int32_t HwPick(const HwPre& pre, const HwWin& win, uint32_t i, float f, uint64_t* id, float* w) {
  const int32_t d = HwCheck(win, f, id, w);
  // (d < 0: the sum of entry i - 1 = win.before > f already)
  const bool prev = d < 0 && i != 0u && !(HwAsFloat(pre.before) > f);
  *id = prev ? ((uint64_t)pre.id_lo | ((uint64_t)pre.id_hi << 32)) : *id;
  *w = prev ? EG_FSUB(HwAsFloat(win.before), HwAsFloat(pre.before)) : *w;
  return prev ? 0 : d;
}

// One draw on a line.  Returns 1 when the guessed entry is the answer, 2 when the entry before
// it is, -1 when the draw is cold.
EG_HD int32_t HwDraw(const HwLine* ln, float f, uint64_t* id, float* w) {
  const uint32_t i = HwGuess(HwLoadHead(ln), f);
  const HwWin win = HwLoadWin(ln, i);
  const int32_t d = HwCheck(win, f, id, w);
  if (d == 0) return 1;
  return HwPick(HwLoadPre(ln, i), win, i, f, id, w) == 0 ? 2 : -1;
}

// The hot part of one draw, as WbSampleHot: false = cold (r rounded up to the row's total, or
// the guessed entry and the one before it did not settle it) - the caller replays RandomSelect.
EG_HD bool HwSampleHot(const HwLine* hw, const WbRec& rec, double u, uint64_t* id, float* w,
                       int32_t* windows) {
  const double r = EG_DMUL(u, (double)rec.total);
  *windows = 0;
  if (!((double)rec.total > r)) return false;
  const float f = WbFloorToFloat(r);
  const uint32_t nbk = WbBuckets(rec.deg);
  const uint32_t j = nbk <= 1u ? 0u : WbBucketOf(f, nbk, WbScale(nbk, rec.total));
  const int32_t n = HwDraw(hw + rec.wb_lo + j, f, id, w);
  *windows = n < 0 ? 2 : n;
  return n > 0;
}

}  // namespace euler_gpu

#endif  // EULER_AMD_CSRC_WB_HW_H_
