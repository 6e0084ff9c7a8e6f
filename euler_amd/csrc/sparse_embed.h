// Sparse-feature embedding lookup (ShallowEncoder: get_sparse_feature +
// tf.nn.embedding_lookup_sparse(table, sp, None, combiner), tf_euler/python/utils/encoders.py:146-170):
// the arithmetic of ONE node - N adjacent columns of its output row - shared by the kernels of
// feature_kernels.hip and by tests/csrc/sparse_embed_check.cc, which compiles this file with the
// host compiler.  Every operation is a correctly rounded fp32 add, divide or square root (on the
// device the __f*_rn forms / the IEEE sqrt the compiler expands, on the host plain operators and
// sqrtf in a translation unit built with -ffp-contract=off), an integer operation or a
// comparison: host and device return the same bits by construction.
//
// ENTRY LIST of a node: the values v[0 .. len) of its uint64 slot; len == 0 (unknown node, empty
// slot, slot id outside the table) gives [default_value] when there is a default, else [].
// RANGE RULE: an entry v >= n_rows (UNSIGNED: values at or above 2^63 included) names no row.  It
// is left out of the sum and of the count; the default value obeys the rule too.
// SUM: the counted rows, widened exactly to fp32, in stored order, one add per entry: the first
// counted row is taken as it is (not added to 0), every later one is one MpwAdd.
// COMBINERS, cnt = the number of counted entries: sum; mean = sum / (float)cnt;
// sqrtn = sum / sqrtf((float)cnt); cnt == 0 gives a zero row, with no division.
//
// The rows of K entries are loaded before the first of them is added; the adds keep stored order.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <math.h>
#endif

#include "half_cvt.h"
#include "mp_weighted.h"

namespace euler_gpu {

constexpr int kSeSum = 0, kSeMean = 1, kSeSqrtn = 2;
#if defined(EULER_GPU_SE_UNROLL)
constexpr int kSeUnroll = EULER_GPU_SE_UNROLL;   // an experiment's build (make EXTRA=-D...)
#else
constexpr int kSeUnroll = 4;                     // rows in flight per lane before the first add
#endif

EG_MPW_HD float SeSqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_sqrtf(x);        // the correctly rounded expansion (never the native form)
#else
  return sqrtf(x);
#endif
}

// What the sum is divided by; never called with cnt == 0.
EG_MPW_HD float SeDenominator(int32_t cnt, int32_t combiner) {
  return combiner == kSeMean ? (float)cnt : SeSqrt((float)cnt);
}

// Folds the entries j = 0 .. m - 1 of `o` into acc[0..N) / *cnt, K rows at a time.
// Ops supplies: Raw (what one load of the N columns returns), Entry(j) - the j-th entry, callable
// for every j below m rounded up to K -, Load(row) and Widen(raw, f[N]).  The K loads are issued
// without a branch between them: an entry that is not counted loads row 0 (n_rows >= 1) and its
// value is dropped.
template <int N, int K, typename Ops>
EG_MPW_HD void SeFold(const Ops& o, int32_t m, uint64_t n_rows, float acc[N], int32_t* cnt) {
  for (int32_t j0 = 0; j0 < m; j0 += K) {
    uint64_t id[K];
    bool ok[K];
    typename Ops::Raw v[K];
EG_MPW_UNROLL
    for (int x = 0; x < K; ++x) {
      id[x] = o.Entry(j0 + x);
      ok[x] = j0 + x < m && id[x] < n_rows;
    }
EG_MPW_UNROLL
    for (int x = 0; x < K; ++x) v[x] = o.Load(ok[x] ? (int64_t)id[x] : 0);
EG_MPW_UNROLL
    for (int x = 0; x < K; ++x) {
      if (!ok[x]) continue;
      float f[N];
      o.Widen(v[x], f);
      if (*cnt == 0) {
EG_MPW_UNROLL
        for (int k = 0; k < N; ++k) acc[k] = f[k];
      } else {
EG_MPW_UNROLL
        for (int k = 0; k < N; ++k) acc[k] = MpwAdd(acc[k], f[k]);
      }
      ++*cnt;
    }
  }
}

// The combiner over the folded sum: acc[0..N) becomes the output columns.
template <int N>
EG_MPW_HD void SeFinish(float acc[N], int32_t cnt, int32_t combiner) {
  if (cnt == 0) {
EG_MPW_UNROLL
    for (int k = 0; k < N; ++k) acc[k] = 0.f;
    return;
  }
  if (combiner == kSeSum) return;
  const float d = SeDenominator(cnt, combiner);
EG_MPW_UNROLL
  for (int k = 0; k < N; ++k) acc[k] = MpwDiv(acc[k], d);
}

// Lanes per node: the power of two in 1..64 that covers the row's `chunks` (16-byte pieces on the
// vector path, elements on the scalar one); wider rows loop.
inline int32_t SeGroupLanes(int64_t chunks) {
  int32_t g = 1;
  while (g < 64 && g < chunks) g <<= 1;
  return g;
}

}  // namespace euler_gpu
