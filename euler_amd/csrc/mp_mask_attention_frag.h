// The steps mask_attention_kernels.hip and mask_attention_backward_kernels.hip share: the argument
// block of the forward, the staging of a candidate block (the head's slice of z and its scores), a
// lane's mask words, its bit and its scores of a chunk, and the hardware exp.  The layouts are stated
// in mp_mask.h and mp_mask_attention.h.  Device code: include it from a .hip file only.
#pragma once

#include <hip/hip_runtime.h>

#include "mp_mask_attention.h"
#include "mp_mask_frag.h"
#include "mp_rows.h"

namespace euler_gpu {

struct MaskAttArgs {
  const uint64_t* mask;
  const void* z;
  const float* s_src;
  const float* s_nb;
  const void* root;
  const float* s_root;
  void* out;
  int64_t batch;
  int32_t n, m, d, dh, heads, relu, out_f32, words, waves;
  float slope;
  MaskAttPlan plan;
};

template <int DT>
constexpr int AttBlockWords() { return (DT == kF32 ? kMaskBlock32 : kMaskBlock16) / 64; }

// The block's slice of the head's columns of z into LDS: MaskStage with the row stride d apart from
// the column bound dh.  Rows c0 + k < m of batch row b and columns f0 + f < dh of the head; +0 else
template <int DT, int NT, bool VEC>
__device__ __forceinline__ void AttStage(const MaskAttArgs& a, int64_t row0, int32_t col0, int32_t c0, int32_t f0,
                                         unsigned char* lds) {
  constexpr int kPieces = 2 * NT;                  // pieces of 8 columns in the column tile
  const int32_t stride = a.plan.stride;
  if constexpr (DT == kF32) {
    const int32_t total = a.plan.kb * kPieces;
    for (int32_t i = threadIdx.x; i < total; i += blockDim.x) {
      const int32_t fb = i % kPieces, k = i / kPieces;
      DenseWords r[2];
      DenseLoadA<DT, VEC>(a.z, c0 + k < a.m ? (row0 + c0 + k) * a.d + col0 : -1, f0 + 8 * fb, a.dh, r);
      DenseWords* to = reinterpret_cast<DenseWords*>(lds + k * stride + fb * 32);
      to[0] = r[0];
      to[1] = r[1];
    }
  } else {
    const int32_t total = (a.plan.kb / 8) * kPieces;
    for (int32_t i = threadIdx.x; i < total; i += blockDim.x) {
      const int32_t fb = i % kPieces, kblk = i / kPieces;
      DenseWords r[8];                             // r[k][p]: columns 2 p, 2 p + 1 of candidate k
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int32_t c = c0 + 8 * kblk + k;
        DenseLoadA<DT, VEC>(a.z, c < a.m ? (row0 + c) * a.d + col0 : -1, f0 + 8 * fb, a.dh, &r[k]);
      }
#pragma unroll
      for (int f = 0; f < 8; ++f) {                // column f of the block: candidates 2 q, 2 q + 1 per word
        DenseWords t;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t lo = r[2 * q][f / 2], hi = r[2 * q + 1][f / 2];
          t[q] = f % 2 == 0 ? (lo & 0xffffu) | (hi << 16) : (lo >> 16) | (hi & 0xffff0000u);
        }
        *reinterpret_cast<DenseWords*>(lds + MaskXtByte(8 * fb + f, 16 * kblk, stride)) = t;
      }
    }
  }
}

// The head's scores of the block's candidates into LDS, in candidate order; +0 from m on
__device__ __forceinline__ void AttStageScores(const MaskAttArgs& a, int64_t row0, int32_t h, int32_t c0, float* sc) {
  for (int32_t i = threadIdx.x; i < a.plan.kb; i += blockDim.x)
    sc[i] = c0 + i < a.m ? a.s_nb[(row0 + c0 + i) * a.heads + h] : 0.f;
}

// this lane's words of the block that starts at word w0, stray bits cleared
template <int KW>
__device__ __forceinline__ void AttLoadWords(const uint64_t* const* mrow, int32_t w0, int32_t live, int32_t words,
                                             uint64_t tail, uint64_t (*word)[KW]) {
#pragma unroll
  for (int q = 0; q < kMaskRuns; ++q)
#pragma unroll
    for (int w = 0; w < KW; ++w) {
      word[q][w] = (mrow[q] && w < live) ? mrow[q][w0 + w] : 0ull;
      if (w0 + w == words - 1) word[q][w] &= tail;
    }
}

// Element j of lane group g's fragment of a chunk is candidate 8 g + j of the chunk (fp32: 4 j + g):
// its bit of the chunk's 32, and its score
template <int DT>
__device__ __forceinline__ bool AttBit(uint32_t half, int32_t g, int j) {
  return ((half >> (DT == kF32 ? 4 * j + g : 8 * g + j)) & 1u) != 0u;
}

template <int DT>
__device__ __forceinline__ void AttScores(const float* sc, int32_t kc, int32_t g, float* s) {
  if constexpr (DT == kF32) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = sc[kc + 4 * j + g];
  } else {
    const DenseAcc* at = reinterpret_cast<const DenseAcc*>(sc + kc + 8 * g);
    const DenseAcc lo = at[0], hi = at[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) { s[j] = lo[j]; s[4 + j] = hi[j]; }
  }
}

// exp(e - shift) by the hardware exp2
__device__ __forceinline__ float AttExp(float e, float shift) {
  return __builtin_amdgcn_exp2f(MpwMul(MpwSub(e, shift), kMaskAttLog2e));
}

}  // namespace euler_gpu
