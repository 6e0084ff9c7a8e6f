// The fragment steps mask_aggregate_kernels.hip and mask_attention_kernels.hip share: the B fragment
// of a chunk read from the staged feature tile, and one element of a root row.  The layouts are
// stated in mp_mask.h.  Device code: include it from a .hip file only.
#pragma once

#include <hip/hip_runtime.h>

#include "mp_dense_frag.h"
#include "mp_mask.h"

namespace euler_gpu {

// The B fragment(s) of column 16 nf + c for the chunk at candidate kc of the block
template <int DT>
__device__ __forceinline__ void MaskLoadB(const unsigned char* lds, int32_t stride, int32_t kc, int32_t nf, int32_t c,
                                          int32_t g, DenseWords* bw) {
  if constexpr (DT == kF32) {
    const unsigned char* at = lds + (kc + g) * stride + (16 * nf + c) * 4;
#pragma unroll
    for (int j = 0; j < 8; ++j) bw[j / 4][j % 4] = *reinterpret_cast<const uint32_t*>(at + 4 * j * stride);
  } else {
    bw[0] = *reinterpret_cast<const DenseWords*>(lds + MaskXtByte(16 * nf + c, (kc + 8 * g) * 2, stride));
  }
}

template <int DT>
__device__ __forceinline__ float MaskRoot(const void* root, int64_t at) {
  return TkWiden<DT>(DT == kF32 ? static_cast<const uint32_t*>(root)[at]
                                : (uint32_t)static_cast<const uint16_t*>(root)[at]);
}

}  // namespace euler_gpu
