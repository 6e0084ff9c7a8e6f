// The fragment steps of the reduce-then-dense family on the matrix units of gfx950, shared by
// aggregate_dense_kernels.hip and aggregate_gru_kernels.hip: the 8 elements a lane holds of a K
// chunk of 32 - loaded from a row, folded in fp32, narrowed into an operand, multiplied.  The
// layouts are stated in mp_pool.h and mp_dense.h.  Device code: include it from a .hip file only.
#pragma once

#include <hip/hip_runtime.h>

#include "mp_dense.h"

namespace euler_gpu {

typedef float DenseAcc __attribute__((ext_vector_type(4)));
typedef uint32_t DenseWords __attribute__((ext_vector_type(4)));
typedef __bf16 DenseBf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 DenseF16x8 __attribute__((ext_vector_type(8)));

constexpr int kDenseChunks = kDenseFoldTile / kPoolChunk;     // chunks of a fold tile

// 16-byte words of the 8 elements a lane holds of a chunk
template <int DT>
constexpr int DenseFragWords() { return DT == kF32 ? 2 : 1; }
// positions whose loads are issued together: 64 registers of rows in flight (element loads of
// 16-bit rows: half of that, their unpacked halves need registers of their own)
template <int DT, bool VEC>
constexpr int DenseBatch() { return DT == kF32 || !VEC ? 2 : 4; }

// The 8 elements k .. k + 8 of the row at element offset `at` (< 0: no row), +0 from d on: the
// load rules of PoolLoadA
template <int DT, bool VEC>
__device__ __forceinline__ void DenseLoadA(const void* table, int64_t at, int32_t k, int32_t d, DenseWords* w) {
  const DenseWords zero = {0u, 0u, 0u, 0u};
  if constexpr (DT == kF32) {
    const uint32_t* p = static_cast<const uint32_t*>(table);
    if constexpr (VEC) {
      w[0] = (at >= 0 && k < d) ? *reinterpret_cast<const DenseWords*>(p + at + k) : zero;
      w[1] = (at >= 0 && k + 4 < d) ? *reinterpret_cast<const DenseWords*>(p + at + k + 4) : zero;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) w[j / 4][j % 4] = (at >= 0 && k + j < d) ? p[at + k + j] : 0u;
    }
  } else {
    const uint16_t* p = static_cast<const uint16_t*>(table);
    if constexpr (VEC) {
      w[0] = (at >= 0 && k < d) ? *reinterpret_cast<const DenseWords*>(p + at + k) : zero;
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

// W^T of columns f0 .. f0 + 16 NT and of k_base .. k_base + k_len of w [k_all, f_all] into wt; +0
// beyond f_all and k_all
template <int DT, int NT>
__device__ __forceinline__ void DenseStageW(const void* w, int32_t k_all, int32_t f_all, int32_t f0, int32_t k_base,
                                            int32_t k_len, int32_t stride, unsigned char* wt) {
  constexpr int kCols = 16 * NT;
  constexpr int kEsz = DT == kF32 ? 4 : 2;
  const int32_t total = kCols * k_len;
  for (int32_t i = threadIdx.x; i < total; i += blockDim.x) {
    const int32_t c = i % kCols, k = i / kCols;
    const bool live = k_base + k < k_all && f0 + c < f_all;
    const int64_t at = (int64_t)(k_base + k) * f_all + f0 + c;
    unsigned char* to = wt + DenseWtByte(c, k * kEsz, stride);
    if constexpr (DT == kF32)
      *reinterpret_cast<uint32_t*>(to) = live ? static_cast<const uint32_t*>(w)[at] : 0u;
    else
      *reinterpret_cast<uint16_t*>(to) = live ? static_cast<const uint16_t*>(w)[at] : (uint16_t)0;
  }
}

// acc += A(16 x 32) B(32 x 16) for one chunk, from the 8 elements each lane holds of A and of B
template <int DT>
__device__ __forceinline__ DenseAcc DenseMma(const DenseWords* a, const DenseWords* b, DenseAcc acc) {
  if constexpr (DT == kBF16) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(DenseBf16x8, a[0]),
                                                   __builtin_bit_cast(DenseBf16x8, b[0]), acc, 0, 0, 0);
  } else if constexpr (DT == kF16) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(DenseF16x8, a[0]),
                                                  __builtin_bit_cast(DenseF16x8, b[0]), acc, 0, 0, 0);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(BitsF32(a[j / 4][j % 4]), BitsF32(b[j / 4][j % 4]), acc, 0, 0, 0);
    return acc;
  }
}

// acc[n] += a (one chunk) x the chunk at byte kb of the NT fragments of wt
template <int DT, int NT>
__device__ __forceinline__ void DenseChunkMma(const DenseWords* a, const unsigned char* wt, int32_t stride, int32_t kb,
                                              int32_t c, DenseAcc* acc) {
  constexpr int FW = DenseFragWords<DT>();
#pragma unroll
  for (int n = 0; n < NT; ++n) {          // (columns from F on are +0 in LDS: no branch here)
    DenseWords bw[FW];
#pragma unroll
    for (int q = 0; q < FW; ++q)
      bw[q] = *reinterpret_cast<const DenseWords*>(wt + DenseWtByte(n * 16 + c, kb + 16 * q, stride));
    acc[n] = DenseMma<DT>(a, bw, acc[n]);
  }
}

// fold[0 .. 8) += the 8 widened elements of w, each add rounded on its own; scale: times s first
template <int DT>
__device__ __forceinline__ void DenseFoldAdd(const DenseWords* w, float* fold, bool scale, float s) {
  float v[8];
  if constexpr (DT == kF32) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = BitsF32(w[j / 4][j % 4]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) Widen2<DT>(w[0][j], &v[2 * j], &v[2 * j + 1]);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) fold[j] = MpwAdd(fold[j], scale ? MpwMul(s, v[j]) : v[j]);
}

// the finished fold of a chunk as its A fragment: the mean's division, then the one narrowing
template <int DT>
__device__ __forceinline__ void DenseFragment(const float* fold, bool mean, float denom, DenseWords* w) {
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = mean ? MpwDiv(fold[j], denom) : fold[j];
  if constexpr (DT == kF32) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j / 4][j % 4] = F32Bits(v[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) w[0][j] = Narrow2<DT>(v[2 * j], v[2 * j + 1]);
  }
}

}  // namespace euler_gpu
