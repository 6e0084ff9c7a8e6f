// Kernels 2 and 3 of the fused dense backward (mp_dense_backward.h) on the matrix units of gfx950, shared by
// aggregate_dense_backward_kernels.hip and pool_aggregate_backward_kernels.hip: out = X W^T from W in its
// natural layout, the slab-wise X^T Y with its LDS transpose, and the ordered sum of the slab partials.
// The weight kernel takes its X rows one per step row (GATHER false: row r of x, the dense layer's A | root)
// or through an index array (GATHER true: row g[r] of a table under the RANGE RULE of mp_pool.h, an index
// outside the table being a row of +0 - the pooling layer's positions).  Device code: include it from a
// .hip file only.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"
#include "mp_dense_backward.h"
#include "mp_dense_frag.h"

namespace euler_gpu {
namespace {

template <int DT>
__device__ __forceinline__ float DenseBwdGrad(const void* grad, int32_t grad_f32, int64_t at) {
  if (DT == kF32 || grad_f32) return static_cast<const float*>(grad)[at];
  return TkWiden<DT>((uint32_t)static_cast<const uint16_t*>(grad)[at]);
}

template <int DT>
__device__ __forceinline__ void DenseBwdPut(void* out, int64_t at, float v) {
  if constexpr (DT == kF32) static_cast<float*>(out)[at] = v;
  else static_cast<uint16_t*>(out)[at] = HalfCvt<DT>::Narrow(v);
}

extern __shared__ __align__(16) unsigned char dense_bwd_lds[];

// ---- kernel 2: out[r] = X[r] W^T, W [n_all, k_all] in its natural layout --------------------------
struct DenseBwdRowsArgs {
  const void* x;                        // [size, k_all] of the table's dtype: dZ
  const void* w;                        // [n_all, k_all]
  int32_t k_all, n_all, size;
  const int64_t* seg_ptr; int64_t count, e;
  int32_t mean, extra;                  // mean: divide by DenseDenominator(len + extra)
  float* out32;                         // [size, n_all] fp32 | NULL: d_agg
  void* out_dt;                         // [size, n_all] of the table's dtype | NULL: d_root
  float scale; int32_t has_scale;       // of out_dt
  DensePlan plan;
};

// rows n0 .. n0 + 16 NT of w [n_all, k_all] as the columns of wt, k32 elements each; +0 beyond both extents
template <int DT, int NT>
__device__ __forceinline__ void DenseBwdStageRows(const void* w, int32_t n_all, int32_t k_all, int32_t n0, int32_t k32,
                                                  int32_t stride, unsigned char* wt) {
  constexpr int kEsz = DT == kF32 ? 4 : 2;
  const int32_t total = 16 * NT * k32;
  for (int32_t i = threadIdx.x; i < total; i += blockDim.x) {
    const int32_t k = i % k32, c = i / k32;
    const bool live = n0 + c < n_all && k < k_all;
    const int64_t at = (int64_t)(n0 + c) * k_all + k;
    unsigned char* to = wt + DenseWtByte(c, k * kEsz, stride);
    if constexpr (DT == kF32)
      *reinterpret_cast<uint32_t*>(to) = live ? static_cast<const uint32_t*>(w)[at] : 0u;
    else
      *reinterpret_cast<uint16_t*>(to) = live ? static_cast<const uint16_t*>(w)[at] : (uint16_t)0;
  }
}

template <int DT, int NT, bool VEC>
__global__ __launch_bounds__(64 * kDenseWaves, 2) void DenseBwdRowsKernel(const DenseBwdRowsArgs a) {
  constexpr int FW = DenseFragWords<DT>();
  constexpr int kEsz = DT == kF32 ? 4 : 2;
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  const int32_t k32 = (a.k_all + kPoolChunk - 1) / kPoolChunk * kPoolChunk;
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kDenseWaves - 1) / kDenseWaves;

  for (int32_t np = 0; np < a.plan.f_passes; ++np) {
    const int32_t n0 = np * 16 * NT;
    __syncthreads();
    DenseBwdStageRows<DT, NT>(a.w, a.n_all, a.k_all, n0, k32, a.plan.stride_n, dense_bwd_lds);
    __syncthreads();
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
      const int64_t r0 = (grp * kDenseWaves + wave) * kPoolTile;
      const int32_t nr = r0 >= a.size ? 0 : (a.size - r0 < kPoolTile ? (int32_t)(a.size - r0) : kPoolTile);
      if (nr == 0) continue;
      const int64_t x_at = c < nr ? (r0 + c) * a.k_all : -1;
      DenseAcc acc[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[n] = DenseAcc{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
      for (int32_t k0 = 0; k0 < k32; k0 += kDenseFoldTile) {
        const int32_t live = (k32 - k0) / kPoolChunk < kDenseChunks ? (k32 - k0) / kPoolChunk : kDenseChunks;
        DenseWords rw[kDenseChunks][FW];
#pragma unroll
        for (int x = 0; x < kDenseChunks; ++x)
          DenseLoadA<DT, VEC>(a.x, x_at, k0 + x * kPoolChunk + 8 * g, a.k_all, rw[x]);
#pragma unroll
        for (int x = 0; x < kDenseChunks; ++x)
          if (x < live)
            DenseChunkMma<DT, NT>(rw[x], dense_bwd_lds, a.plan.stride_n, (k0 + x * kPoolChunk + 8 * g) * kEsz, c, acc);
      }
      // the denominators of the four destinations this lane holds in the accumulator layout
      float den[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        den[i] = 1.f;
        if (a.mean && 4 * g + i < nr) {
          int64_t b = 0, en = 0;
          TkSegment(a.seg_ptr, a.count, a.e, r0 + 4 * g + i, &b, &en);
          den[i] = DenseDenominator(en - b + a.extra);
        }
      }
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int32_t col = n0 + 16 * n + c;
        if (col >= a.n_all) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int32_t ri = 4 * g + i;
          if (ri >= nr) continue;
          const int64_t at = (r0 + ri) * a.n_all + col;
          const float v = a.mean ? MpwDiv(acc[n][i], den[i]) : acc[n][i];
          if (a.out32) a.out32[at] = v;
          if (a.out_dt) DenseBwdPut<DT>(a.out_dt, at, a.has_scale ? MpwMul(a.scale, v) : v);
        }
      }
    }
  }
}

template <int DT, int NT>
int DenseBwdRowsLoads(hipStream_t st, const DenseBwdRowsArgs& a) {
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kDenseWaves - 1) / kDenseWaves;
  const dim3 grid((unsigned)(groups > kDenseMaxBlocks ? kDenseMaxBlocks : groups)), block(64 * kDenseWaves);
  if (PoolVectorLoads(a.k_all, (uintptr_t)a.x, DT == kF32))
    hipLaunchKernelGGL((DenseBwdRowsKernel<DT, NT, true>), grid, block, (size_t)a.plan.lds_bytes, st, a);
  else
    hipLaunchKernelGGL((DenseBwdRowsKernel<DT, NT, false>), grid, block, (size_t)a.plan.lds_bytes, st, a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DT>
int DenseBwdRows(hipStream_t st, const DenseBwdRowsArgs& a) {
  switch (a.plan.nt) {
    case 1: return DenseBwdRowsLoads<DT, 1>(st, a);
    case 2: return DenseBwdRowsLoads<DT, 2>(st, a);
    case 4: return DenseBwdRowsLoads<DT, 4>(st, a);
    default: return DenseBwdRowsLoads<DT, 8>(st, a);
  }
}

// ---- kernel 3: partial[slab][k][f] = sum over the slab's r of X[r][k] Y[r][f] ----------------------
struct DenseBwdWeightArgs {
  const void* x; int32_t kx, vec_x;     // [size, kx]: A | root; GATHER: the table [x_rows, kx]
  const void* y; int32_t fy, vec_y;     // [size, fy]: dZ
  int32_t size, slab_rows, slabs;
  float* partial;                       // [slabs, kx, fy]
  float* bias_partial;                  // [slabs, fy] | NULL
  const void* gather; int32_t is_ids;   // GATHER: step row r reads row TkRow(gather, is_ids, r, x_rows) of x
  int64_t x_rows;
};

// byte of destination r (of a step) of column col in a transposed tile
__device__ __forceinline__ uint32_t DenseBwdTileByte(int32_t col, int32_t rb, int32_t stride) {
  return (uint32_t)(col * stride + (((rb >> 4) ^ ((col >> 3) & 3)) << 4) + (rb & 15));
}

template <int DT>
__device__ __forceinline__ void DenseBwdLoad8(const void* p, bool vec, int64_t at, int32_t k, int32_t all, DenseWords* w) {
  if (vec) DenseLoadA<DT, true>(p, at, k, all, w);
  else DenseLoadA<DT, false>(p, at, k, all, w);
}

// element offset of the X row of step row r (< r_end, else no row: -1)
template <bool GATHER>
__device__ __forceinline__ int64_t DenseBwdRowAt(const DenseBwdWeightArgs& a, int64_t r, int64_t r_end) {
  if (r >= r_end) return -1;
  if constexpr (GATHER) {
    const int64_t row = TkRow(a.gather, a.is_ids, r, a.x_rows);
    return row < 0 ? -1 : row * a.kx;
  } else {
    return r * a.kx;
  }
}

// the 8 elements a thread loaded of row r, columns c8 .. c8 + 8, into their columns of a transposed tile
template <int DT>
__device__ __forceinline__ void DenseBwdSpread(const DenseWords* w, int32_t c8, int32_t r, int32_t stride, unsigned char* t) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if constexpr (DT == kF32)
      *reinterpret_cast<uint32_t*>(t + DenseBwdTileByte(c8 + j, 4 * r, stride)) = w[j / 4][j % 4];
    else
      *reinterpret_cast<uint16_t*>(t + DenseBwdTileByte(c8 + j, 2 * r, stride)) = (uint16_t)(w[0][j / 2] >> (16 * (j % 2)));
  }
}

// the operand fragment of column col: its 8 consecutive destinations from 8 g
template <int DT>
__device__ __forceinline__ void DenseBwdFrag(const unsigned char* t, int32_t col, int32_t g, int32_t stride, DenseWords* w) {
  constexpr int FW = DenseFragWords<DT>();
  constexpr int kEsz = DT == kF32 ? 4 : 2;
#pragma unroll
  for (int q = 0; q < FW; ++q)
    w[q] = *reinterpret_cast<const DenseWords*>(t + DenseBwdTileByte(col, 8 * g * kEsz + 16 * q, stride));
}

template <int DT, bool GATHER>
__global__ __launch_bounds__(64 * kDenseWaves) void DenseBwdWeightKernel(const DenseBwdWeightArgs a) {
  constexpr int FW = DenseFragWords<DT>();
  constexpr int kStride = kDenseBwdStep * (DT == kF32 ? 4 : 2) + 16;
  constexpr int NF = kDenseBwdTile / 16;
  __shared__ __align__(16) unsigned char tx[kDenseBwdTile * kStride];
  __shared__ __align__(16) unsigned char ty[kDenseBwdTile * kStride];
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  const int32_t lr = threadIdx.x >> 3, c8 = (threadIdx.x & 7) * 8;     // the row and columns this thread loads
  const int32_t kts = (a.kx + kDenseBwdTile - 1) / kDenseBwdTile, fts = (a.fy + kDenseBwdTile - 1) / kDenseBwdTile;
  const int64_t jobs = (int64_t)a.slabs * kts * fts;
  const uint32_t one = DT == kF32 ? 0x3f800000u : (DT == kBF16 ? 0x3f803f80u : 0x3c003c00u);
  const DenseWords ones[2] = {{one, one, one, one}, {one, one, one, one}};

  for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int32_t slab = (int32_t)(job / (kts * fts)), rem = (int32_t)(job % (kts * fts));
    const int32_t k0 = rem / fts * kDenseBwdTile, f0 = rem % fts * kDenseBwdTile;
    const int64_t r_begin = (int64_t)slab * a.slab_rows;
    const int64_t r_end = r_begin + a.slab_rows < a.size ? r_begin + a.slab_rows : a.size;
    const bool with_bias = a.bias_partial != nullptr && k0 == 0 && wave == 0;
    DenseAcc acc[NF], acc_b[NF];
#pragma unroll
    for (int n = 0; n < NF; ++n) acc[n] = acc_b[n] = DenseAcc{0.f, 0.f, 0.f, 0.f};
    DenseWords wx[FW], wy[FW];
    {
      const int64_t r = r_begin + lr;
      DenseBwdLoad8<DT>(a.x, a.vec_x != 0, DenseBwdRowAt<GATHER>(a, r, r_end), k0 + c8, a.kx, wx);
      DenseBwdLoad8<DT>(a.y, a.vec_y != 0, r < r_end ? r * a.fy : -1, f0 + c8, a.fy, wy);
    }
    for (int64_t rs = r_begin; rs < r_end; rs += kDenseBwdStep) {
      __syncthreads();                                      // the previous step's fragments are read
      DenseBwdSpread<DT>(wx, c8, lr, kStride, tx);
      DenseBwdSpread<DT>(wy, c8, lr, kStride, ty);
      __syncthreads();
      if (rs + kDenseBwdStep < r_end) {                     // the next step's loads, ahead of the MFMAs
        const int64_t r = rs + kDenseBwdStep + lr;
        DenseBwdLoad8<DT>(a.x, a.vec_x != 0, DenseBwdRowAt<GATHER>(a, r, r_end), k0 + c8, a.kx, wx);
        DenseBwdLoad8<DT>(a.y, a.vec_y != 0, r < r_end ? r * a.fy : -1, f0 + c8, a.fy, wy);
      }
      DenseWords fa[FW];
      DenseBwdFrag<DT>(tx, 16 * wave + c, g, kStride, fa);
#pragma unroll
      for (int n = 0; n < NF; ++n) {
        DenseWords fb[FW];
        DenseBwdFrag<DT>(ty, 16 * n + c, g, kStride, fb);
        acc[n] = DenseMma<DT>(fa, fb, acc[n]);
        if (with_bias) acc_b[n] = DenseMma<DT>(ones, fb, acc_b[n]);
      }
    }
    // the accumulator holds k = k0 + 16 wave + 4 g + i of column f0 + 16 n + c
#pragma unroll
    for (int n = 0; n < NF; ++n) {
      const int32_t col = f0 + 16 * n + c;
      if (col >= a.fy) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int32_t k = k0 + 16 * wave + 4 * g + i;
        if (k < a.kx) a.partial[((int64_t)slab * a.kx + k) * a.fy + col] = acc[n][i];
      }
      if (with_bias && g == 0) a.bias_partial[(int64_t)slab * a.fy + col] = acc_b[n][0];
    }
  }
}

// out[i] = the partials of element i in increasing slab from +0, rounded once to out's dtype
__global__ __launch_bounds__(256) void DenseBwdSumKernel(const float* partial, int32_t slabs, int64_t n, void* out,
                                                         int32_t out_dtype) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int32_t b = 0; b < slabs; ++b) s = MpwAdd(s, partial[(int64_t)b * n + i]);
    if (out_dtype == EULER_GPU_F32) static_cast<float*>(out)[i] = s;
    else if (out_dtype == EULER_GPU_BF16) static_cast<uint16_t*>(out)[i] = HalfCvt<kBF16>::Narrow(s);
    else static_cast<uint16_t*>(out)[i] = HalfCvt<kF16>::Narrow(s);
  }
}

int DenseBwdSum(hipStream_t st, const float* partial, int64_t slabs, int64_t n, void* out, int32_t out_dtype) {
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(DenseBwdSumKernel, dim3((unsigned)(blocks > kDenseBwdMaxBlocks ? kDenseBwdMaxBlocks : blocks)),
                     dim3(256), 0, st, partial, (int32_t)slabs, n, out, out_dtype);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DT, bool GATHER = false>
int DenseBwdWeight(hipStream_t st, const DenseBwdWeightArgs& a) {
  const int64_t jobs = (int64_t)a.slabs * ((a.kx + kDenseBwdTile - 1) / kDenseBwdTile) *
                       ((a.fy + kDenseBwdTile - 1) / kDenseBwdTile);
  hipLaunchKernelGGL((DenseBwdWeightKernel<DT, GATHER>), dim3((unsigned)(jobs > kDenseBwdMaxBlocks ? kDenseBwdMaxBlocks : jobs)),
                     dim3(64 * kDenseWaves), 0, st, a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

}  // namespace
}  // namespace euler_gpu
