// The fragment steps of pool_aggregate on the matrix units of gfx950, shared by pool_aggregate_kernels.hip
// and its backward (pool_aggregate_backward_kernels.hip): the 8 elements a lane holds of a K chunk of
// 32 - loaded from a row, multiplied - the staging of W^T and the wave-level fence of the fold's
// staging rows.  The layouts are stated in mp_pool.h.  Device code: include it from a .hip file only.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"
#include "mp_pool.h"

namespace euler_gpu {
namespace {

typedef float PoolAcc __attribute__((ext_vector_type(4)));
typedef uint32_t PoolWords __attribute__((ext_vector_type(4)));
typedef __bf16 PoolBf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 PoolF16x8 __attribute__((ext_vector_type(8)));

constexpr int kPoolBatch = 4;             // K chunks whose A loads are issued together

// 16-byte words of the 8 elements a lane holds of a chunk
template <int DT>
constexpr int PoolFragWords() { return DT == kF32 ? 2 : 1; }

// The 8 elements k .. k + 8 of the row at element offset `at` (< 0: no row), +0 from d on
template <int DT, bool VEC>
__device__ __forceinline__ void PoolLoadA(const void* table, int64_t at, int32_t k, int32_t d, PoolWords* w) {
  const PoolWords zero = {0u, 0u, 0u, 0u};
  if constexpr (DT == kF32) {
    const uint32_t* p = static_cast<const uint32_t*>(table);
    if constexpr (VEC) {
      w[0] = (at >= 0 && k < d) ? *reinterpret_cast<const PoolWords*>(p + at + k) : zero;
      w[1] = (at >= 0 && k + 4 < d) ? *reinterpret_cast<const PoolWords*>(p + at + k + 4) : zero;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) w[j / 4][j % 4] = (at >= 0 && k + j < d) ? p[at + k + j] : 0u;
    }
  } else {
    const uint16_t* p = static_cast<const uint16_t*>(table);
    if constexpr (VEC) {
      w[0] = (at >= 0 && k < d) ? *reinterpret_cast<const PoolWords*>(p + at + k) : zero;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t lo = (at >= 0 && k + 2 * j < d) ? p[at + k + 2 * j] : 0u;
        const uint32_t hi = (at >= 0 && k + 2 * j + 1 < d) ? p[at + k + 2 * j + 1] : 0u;
        w[0][j] = lo | (hi << 16);
      }
    }
  }
}

// acc += A(16 x 32) B(32 x 16) for one chunk, from the 8 elements each lane holds of A and of B
template <int DT>
__device__ __forceinline__ PoolAcc PoolMma(const PoolWords* a, const PoolWords* b, PoolAcc acc) {
  if constexpr (DT == kBF16) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(PoolBf16x8, a[0]),
                                                   __builtin_bit_cast(PoolBf16x8, b[0]), acc, 0, 0, 0);
  } else if constexpr (DT == kF16) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(PoolF16x8, a[0]),
                                                  __builtin_bit_cast(PoolF16x8, b[0]), acc, 0, 0, 0);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(BitsF32(a[j / 4][j % 4]), BitsF32(b[j / 4][j % 4]), acc, 0, 0, 0);
    return acc;
  }
}

// a wave's own LDS writes before its own LDS reads (and the reverse)
__device__ __forceinline__ void PoolWaveFence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// W^T of columns f0 .. f0 + 16 NT and of K tile kt into wt[c][k]; +0 beyond F and d
// (Args: the forward's or the backward's argument block - weight, d, f and the plan)
template <int DT, int NT, class Args>
__device__ __forceinline__ void PoolStageW(const Args& a, int32_t f0, int32_t kt, void* wt) {
  constexpr int kCols = 16 * NT;
  const int32_t k_base = kt * a.plan.k_tile, total = kCols * a.plan.k_tile;
  for (int32_t i = threadIdx.x; i < total; i += blockDim.x) {
    const int32_t c = i % kCols, k = i / kCols;
    const bool live = k_base + k < a.d && f0 + c < a.f;
    const int64_t at = (int64_t)(k_base + k) * a.f + f0 + c;
    if constexpr (DT == kF32)
      static_cast<uint32_t*>(wt)[c * a.plan.k_stride + k] = live ? static_cast<const uint32_t*>(a.weight)[at] : 0u;
    else
      static_cast<uint16_t*>(wt)[c * a.plan.k_stride + k] = live ? static_cast<const uint16_t*>(a.weight)[at] : (uint16_t)0;
  }
}

extern __shared__ __align__(16) unsigned char pool_lds[];

}  // namespace
}  // namespace euler_gpu
