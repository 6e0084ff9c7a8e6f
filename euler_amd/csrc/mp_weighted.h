// Edge-weighted message passing: the arithmetic of ONE destination - its N adjacent columns
// over the updates of its segment - shared by the weighted segment reduces of mp_kernels.hip
// (fp32) and mp_half_kernels.hip (bf16 / fp16 storage), and by tests/csrc/mp_weighted_check.cc,
// which compiles it with the host compiler.
//
// Destination r reduces, in input order, the values fl(x[g(p)][c] * w[p][c / dh]) of the updates
// p of its segment (gcn_conv.py:50-51 and appnp_conv.py:54-55: norm_i * norm_j * x_j;
// gat_conv.py:71 and agnn_conv.py:54: x_j * alpha).  The product and the sum are TWO correctly
// rounded fp32 operations - never an FMA, whose single rounding has other bits than the
// composition scatter_(op, gather(x, g) * w, dst): on the device the __fmul_rn / __fadd_rn
// intrinsics (which the compiler may not contract), on the host plain operators in a translation
// unit built with -ffp-contract=off.  Mean divides the sum by (segment length + 1e-7f), the
// weights do not enter the denominator (scatter_mean of the message, mp_ops.py:65-69); max
// starts from -1e9 (scatter_op.cc:78), add and mean from 0.
//
// The loads are issued eight (then four, then one) updates at a time - positions, then row
// numbers and weights, then the rows - and the products are folded in afterwards, in input
// order, so the latencies of a batch overlap while every column keeps its order.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EG_MPW_HD __host__ __device__ __forceinline__
#else
#define EG_MPW_HD inline
#endif
#if defined(__clang__)
#define EG_MPW_UNROLL _Pragma("unroll")
#else
#define EG_MPW_UNROLL
#endif

namespace euler_gpu {

EG_MPW_HD float MpwMul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmul_rn(a, b);
#else
  return a * b;
#endif
}

EG_MPW_HD float MpwAdd(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(a, b);
#else
  return a + b;
#endif
}

EG_MPW_HD float MpwDiv(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}

// Which update a grouped position is, and which row of the table it reads:
// perm (nullptr: identity) maps the p-th grouped update to its original position - the row of
// the weight array; gsrc (nullptr: the position itself) holds the gather indices, int32
// (gstride 1) or the low words of int64 ids (gstride 2), clamped to row_max.
struct MpwIndex {
  const uint32_t* perm;
  const int32_t* gsrc;
  int32_t gstride;
  uint32_t row_max;
  EG_MPW_HD int64_t Pos(int64_t p) const { return perm ? (int64_t)perm[p] : p; }
  EG_MPW_HD int64_t Row(int64_t pos) const {
    if (!gsrc) return pos;
    const uint32_t g = (uint32_t)gsrc[pos * gstride];
    return (int32_t)(g < row_max ? g : row_max);
  }
};

// K updates starting at grouped position p: all loads first, then the ordered fold.
template <int MODE, int N, int K, typename Ops>
EG_MPW_HD void MpwBatch(const Ops& o, int64_t p, float acc[N]) {
  int64_t pos[K], row[K];
  float w[K];
  typename Ops::Raw v[K];
EG_MPW_UNROLL
  for (int x = 0; x < K; ++x) pos[x] = o.Pos(p + x);
EG_MPW_UNROLL
  for (int x = 0; x < K; ++x) { row[x] = o.Row(pos[x]); w[x] = o.Weight(pos[x]); }
EG_MPW_UNROLL
  for (int x = 0; x < K; ++x) v[x] = o.Load(row[x]);
EG_MPW_UNROLL
  for (int x = 0; x < K; ++x) {
    float f[N];
    o.Widen(v[x], f);
EG_MPW_UNROLL
    for (int k = 0; k < N; ++k) {
      const float m = MpwMul(f[k], w[x]);
      if (MODE == 1) acc[k] = m > acc[k] ? m : acc[k];
      else acc[k] = MpwAdd(acc[k], m);
    }
  }
}

// acc[0..N) = the reduce (MODE 0 add, 1 max, 2 mean) of destination columns over the grouped
// positions [b, en).  Ops supplies: Raw (what one load of the N columns returns), Pos(p),
// Row(pos), Weight(pos) - the weight of these N columns' head, widened to fp32 -, Load(row) and
// Widen(raw, f[N]).
template <int MODE, int N, typename Ops>
EG_MPW_HD void WeightedReduceRow(const Ops& o, int64_t b, int64_t en, float acc[N]) {
  const float init = MODE == 1 ? (float)-1e9 : 0.f;
  for (int k = 0; k < N; ++k) acc[k] = init;
  int64_t p = b;
  for (; p + 8 <= en; p += 8) MpwBatch<MODE, N, 8>(o, p, acc);
  for (; p + 4 <= en; p += 4) MpwBatch<MODE, N, 4>(o, p, acc);
  for (; p < en; ++p) MpwBatch<MODE, N, 1>(o, p, acc);
  if (MODE == 2) {
    const float denom = MpwAdd((float)(en - b), 1e-7f);
    for (int k = 0; k < N; ++k) acc[k] = MpwDiv(acc[k], denom);
  }
}

}  // namespace euler_gpu
