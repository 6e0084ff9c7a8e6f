// Quantised feature row tables for gfx950 (Fp8Rows: mp_fp8.h, fp8_cvt.h) and their C-ABI entry
// points: the column absmax a scale is taken from, the quantiser, and the forward ops that read
// a table - gather and the gather_segment_reduce family.
//
// Contract: an op on (q, scale) is the fp32 op of mp_kernels.hip on x^ = fl(Dec(q) * scale[c]),
// bit for bit (mp_fp8.h).  What changes is the bytes: a gathered row is a quarter of its fp32
// length, half of its bf16 one.
//
// Lane roles follow the 16-bit kernels with the element count per 16-byte access doubled again:
// a lane of the vector kernels owns SIXTEEN adjacent columns (one 16-byte load per gathered row,
// sixteen fp32 accumulators and its sixteen scales in VGPRs, four 16-byte stores of fp32 results
// or two of 16-bit ones), d / 16 lanes a row, 1024 / d rows a wave.  Every other d or alignment
// takes the element kernels, a column per lane.  (The gather has lane shapes of its own.)  No LDS, no scratch; all row offsets in 64 bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "device_fns.h"
#include "device_mem.h"
#include "mp_fp8.h"

namespace euler_gpu {
namespace {

template <int DT>
__device__ __forceinline__ float LoadElem(const void* p, int64_t i) {
  if constexpr (DT == kF32) return static_cast<const float*>(p)[i];
  else return HalfCvt<DT>::Widen(static_cast<const uint16_t*>(p)[i]);
}

// The value as a finished fp32 in a register.  Without it the compiler folds the multiply of
// Fp8Value into the narrowing convert behind it (v_fma_mixlo_f16: a * b + 0), and the +0 it adds
// turns a -0 product into +0: other bits than one rounding of the fp32 result.
__device__ __forceinline__ float Settled(float v) {
  asm("" : "+v"(v));
  return v;
}

template <int DT>
__device__ __forceinline__ void StoreElem(void* p, int64_t i, float v) {
  if constexpr (DT == kF32) static_cast<float*>(p)[i] = v;
  else static_cast<uint16_t*>(p)[i] = HalfCvt<DT>::Narrow(Settled(v));
}

// sixteen results of a lane: four 16-byte stores of fp32, or two of 16-bit values
template <int OUT>
__device__ __forceinline__ void Store16(void* out, int64_t slot, const float f[16]) {
  if constexpr (OUT == kF32) {
    float4* o = static_cast<float4*>(out) + slot * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
  } else {
    float g[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) g[k] = Settled(f[k]);
    uint32_t lo[4], hi[4];
    Narrow8<OUT>(g, lo);
    Narrow8<OUT>(g + 8, hi);
    uint4* o = static_cast<uint4*>(out) + slot * 2;
    o[0] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    o[1] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  }
}

template <bool IS_MAX>
__device__ __forceinline__ void Accumulate16(float acc[16], const float f[16]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (IS_MAX) acc[k] = f[k] > acc[k] ? f[k] : acc[k];
    else acc[k] = __fadd_rn(acc[k], f[k]);
  }
}

__device__ __forceinline__ void LoadScale16(const float* __restrict__ scale, int64_t cl, float s[16]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) s[k] = scale[cl * 16 + k];
}

// ---- column absmax ---------------------------------------------------------------------------
// absmax[c] = max(absmax[c], max over the FINITE x[r, c] of |x[r, c]|): NaN and +-inf are skipped.
// The bit patterns of non-negative floats order as the floats do, so the running maximum is an
// unsigned integer max - exact, and independent of the order of the (vector) atomics.
// blockDim = (64, 4): lanes over adjacent columns, the rows strided over threadIdx.y and the grid.
template <int DT>
__global__ __launch_bounds__(256) void ColumnAbsmaxKernel(const void* __restrict__ x, int64_t n, int64_t d,
                                                          uint32_t* __restrict__ absmax) {
  for (int64_t c = (int64_t)blockIdx.y * 64 + threadIdx.x; c < d; c += (int64_t)gridDim.y * 64) {
    uint32_t m = 0u;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; r < n;
         r += (int64_t)gridDim.x * blockDim.y) {
      const uint32_t a = F32Bits(LoadElem<DT>(x, r * d + c)) & 0x7fffffffu;
      if (a < 0x7f800000u && a > m) m = a;
    }
    if (m != 0u) atomicMax(absmax + c, m);
  }
}

// ---- quantise --------------------------------------------------------------------------------
// q[r, c] = Enc(x[r, c] / scale[c]): an IEEE fp32 division (not a multiply by a reciprocal), then
// the integer encoder of fp8_cvt.h.  One element a lane; runs once per table.
template <int DT>
__global__ __launch_bounds__(256) void QuantizeRowsKernel(const void* __restrict__ x, int64_t n, int64_t d,
                                                          const float* __restrict__ scale,
                                                          uint8_t* __restrict__ q) {
  const int64_t total = n * d;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t c = i % d;
    q[i] = Fp8Enc(__fdiv_rn(LoadElem<DT>(x, i), scale[c]));
  }
}

// ---- gather ----------------------------------------------------------------------------------
// out[i, :] = x^[idx[i], :], N elements a lane (dv = d / N lanes a row).  The lanes of a wave write
// adjacent 16-byte pieces when the output is fp32 and N = 4 (a 4-byte load of four codes, one
// float4 store) or 16-bit and N = 16 (a 16-byte load, two 16-byte stores); N = 1 serves every
// other shape.  (Sixteen fp32 results a lane would be four stores 64 bytes apart: measured slower
// than the bf16 table's gather, which the read side alone does not explain.)
template <int OUT, int N>
__global__ __launch_bounds__(256) void Fp8GatherKernel(const uint8_t* __restrict__ q,
                                                       const float* __restrict__ scale,
                                                       const int32_t* __restrict__ idx, int64_t e, int64_t dv,
                                                       void* __restrict__ out) {
  static_assert((N == 16 && OUT != kF32) || (N == 4 && OUT == kF32) || N == 1, "see above");
  const int64_t total = e * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float s[N];
  int64_t have = -1;      // the lane group whose scales are in s (it stays put when dv divides the stride)
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += stride) {
    const int64_t i = x / dv;
    const int64_t c = x - i * dv;
    const int64_t at = (int64_t)idx[i] * dv + c;
    if constexpr (N == 16) {
      if (c != have) { LoadScale16(scale, c, s); have = c; }
      float f[16];
      Fp8Value16(reinterpret_cast<const uint4*>(q)[at], s, f);
      Store16<OUT>(out, x, f);
    } else if constexpr (N == 4) {
      if (c != have) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = scale[c * 4 + k];
        have = c;
      }
      float f[4];
      Fp8Dec4(reinterpret_cast<const uint32_t*>(q)[at], f);
      static_cast<float4*>(out)[x] = make_float4(__fmul_rn(f[0], s[0]), __fmul_rn(f[1], s[1]),
                                                 __fmul_rn(f[2], s[2]), __fmul_rn(f[3], s[3]));
    } else {
      StoreElem<OUT>(out, x, Fp8Value(q[at], scale[c]));
    }
  }
}

__device__ __forceinline__ int64_t UpdateRow(const MpwIndex& ix, int64_t p) { return ix.Row(ix.Pos(p)); }

// ---- segment reduces -------------------------------------------------------------------------
// SegmentReduceKernel of mp_kernels.hip over an fp8 table: blockDim = (64, 4), a wave-slot per
// output row, one column per lane.  Serves every d the vector kernel does not.
template <int MODE, int OUT>
__global__ __launch_bounds__(256) void SegmentReduceFp8Kernel(
    const uint8_t* __restrict__ q, const float* __restrict__ scale, const SegSpec seg, const MpwIndex ix,
    int64_t d, void* __restrict__ out) {
  constexpr bool IS_MAX = MODE == 1;
  const int lane = threadIdx.x;
  const int32_t size = seg.size;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; r < size;
       r += (int64_t)gridDim.x * blockDim.y) {
    int64_t b, en;
    SegBounds(seg, r, &b, &en);
    const float denom = __fadd_rn((float)(en - b), 1e-7f);
    for (int64_t c = lane; c < d; c += 64) {
      const float sc = scale[c];
      float acc = IS_MAX ? (float)-1e9 : 0.f;
      int64_t p = b;
      // adds in input order; the loads are issued eight at a time
      for (; p + 8 <= en; p += 8) {
        uint8_t v[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) v[x] = q[UpdateRow(ix, p + x) * d + c];
#pragma unroll
        for (int x = 0; x < 8; ++x) {
          const float f = Fp8Value(v[x], sc);
          if (IS_MAX) { if (f > acc) acc = f; }
          else acc = __fadd_rn(acc, f);
        }
      }
      for (; p < en; ++p) {
        const float f = Fp8Value(q[UpdateRow(ix, p) * d + c], sc);
        if (IS_MAX) { if (f > acc) acc = f; }
        else acc = __fadd_rn(acc, f);
      }
      if (MODE == 2) acc = __fdiv_rn(acc, denom);
      StoreElem<OUT>(out, r * d + c, acc);
    }
  }
}

// d % 16 == 0 with d / 16 a divisor of 64 (d = 16 .. 1024): a lane owns sixteen adjacent columns,
// d16 = d / 16 lanes a row, 64 / d16 rows a wave.
template <int MODE, int OUT>
__global__ __launch_bounds__(256) void SegmentReduceFp8Vec16Kernel(
    const uint4* __restrict__ q16, const float* __restrict__ scale, const SegSpec seg, const MpwIndex ix,
    int32_t d16, void* __restrict__ out) {
  constexpr bool IS_MAX = MODE == 1;
  const int32_t size = seg.size;
  const int32_t rows_per_wave = 64 / d16;
  const int32_t sub = threadIdx.x / d16, cl = threadIdx.x - sub * d16;
  const int64_t rows_per_block = (int64_t)blockDim.y * rows_per_wave;
  float s[16];
  LoadScale16(scale, cl, s);
  for (int64_t r = (int64_t)blockIdx.x * rows_per_block + threadIdx.y * rows_per_wave + sub;
       r < size; r += (int64_t)gridDim.x * rows_per_block) {
    int64_t b, en;
    SegBounds(seg, r, &b, &en);
    const float denom = __fadd_rn((float)(en - b), 1e-7f);
    const float init = IS_MAX ? (float)-1e9 : 0.f;
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = init;
    int64_t p = b;
    // the row numbers first, then the eight rows, then the ordered adds
    for (; p + 8 <= en; p += 8) {
      int64_t pos[8], src[8];
#pragma unroll
      for (int x = 0; x < 8; ++x) pos[x] = ix.Pos(p + x);
#pragma unroll
      for (int x = 0; x < 8; ++x) src[x] = ix.Row(pos[x]);
      uint4 v[8];
#pragma unroll
      for (int x = 0; x < 8; ++x) v[x] = q16[src[x] * d16 + cl];
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        float f[16];
        Fp8Value16(v[x], s, f);
        Accumulate16<IS_MAX>(acc, f);
      }
    }
    for (; p + 4 <= en; p += 4) {
      uint4 v[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) v[x] = q16[UpdateRow(ix, p + x) * d16 + cl];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        float f[16];
        Fp8Value16(v[x], s, f);
        Accumulate16<IS_MAX>(acc, f);
      }
    }
    for (; p < en; ++p) {
      float f[16];
      Fp8Value16(q16[UpdateRow(ix, p) * d16 + cl], s, f);
      Accumulate16<IS_MAX>(acc, f);
    }
    if (MODE == 2) {
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[k] = __fdiv_rn(acc[k], denom);
    }
    Store16<OUT>(out, r * d16 + cl, acc);
  }
}

// ---- edge-weighted reduces: WeightedReduceRow of mp_weighted.h over x^ --------------------------
template <int MODE, int OUT>
__global__ __launch_bounds__(256) void WeightedSegmentReduceFp8Kernel(
    const uint8_t* __restrict__ q, const float* __restrict__ scale, const SegSpec seg, const MpwIndex ix,
    int64_t d, void* __restrict__ out, const void* __restrict__ w, const int32_t w_dtype,
    const int32_t heads, const int32_t dh) {
  const int lane = threadIdx.x;
  const int32_t size = seg.size;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; r < size;
       r += (int64_t)gridDim.x * blockDim.y) {
    int64_t b, en;
    SegBounds(seg, r, &b, &en);
    for (int64_t c = lane; c < d; c += 64) {
      const WeightedFp8Ops1 ops{ix, q, d, c, scale[c], w, w_dtype, heads, (int32_t)(c / dh)};
      float acc[1];
      WeightedReduceRow<MODE, 1>(ops, b, en, acc);
      StoreElem<OUT>(out, r * d + c, acc[0]);
    }
  }
}

// the 16-byte-lane form: dh % 16 == 0 so that a lane's sixteen columns lie in one head
template <int MODE, int OUT>
__global__ __launch_bounds__(256) void WeightedSegmentReduceFp8Vec16Kernel(
    const uint4* __restrict__ q16, const float* __restrict__ scale, const SegSpec seg, const MpwIndex ix,
    int32_t d16, void* __restrict__ out, const void* __restrict__ w, const int32_t w_dtype,
    const int32_t heads, const int32_t dh) {
  const int32_t size = seg.size;
  const int32_t rows_per_wave = 64 / d16;
  const int32_t sub = threadIdx.x / d16, cl = threadIdx.x - sub * d16;
  const int64_t rows_per_block = (int64_t)blockDim.y * rows_per_wave;
  WeightedFp8Ops16 ops{ix, q16, d16, cl, w, w_dtype, heads, (cl * 16) / dh, {}};
  LoadScale16(scale, cl, ops.s);
  for (int64_t r = (int64_t)blockIdx.x * rows_per_block + threadIdx.y * rows_per_wave + sub;
       r < size; r += (int64_t)gridDim.x * rows_per_block) {
    int64_t b, en;
    SegBounds(seg, r, &b, &en);
    float acc[16];
    WeightedReduceRow<MODE, 16>(ops, b, en, acc);
    Store16<OUT>(out, r * d16 + cl, acc);
  }
}

template <int MODE, int OUT>
int LaunchReduce(hipStream_t st, const MpReduceCall& c, const SegSpec& seg, const MpwIndex& ix) {
  const uint8_t* q = static_cast<const uint8_t*>(c.params);
  if (!c.weighted) {
    const LaneShape s = RowLaneShape(seg.size, c.d, 16, 0, q, c.out);
    if (s.vec) {
      hipLaunchKernelGGL((SegmentReduceFp8Vec16Kernel<MODE, OUT>), dim3(s.blocks), dim3(64, 4), 0, st,
                         reinterpret_cast<const uint4*>(q), c.fp8_scale, seg, ix, (int32_t)s.dv, c.out);
    } else {
      hipLaunchKernelGGL((SegmentReduceFp8Kernel<MODE, OUT>), dim3(s.blocks), dim3(64, 4), 0, st, q,
                         c.fp8_scale, seg, ix, c.d, c.out);
    }
  } else {
    const int32_t dh = (int32_t)(c.d / c.heads);
    const LaneShape s = RowLaneShape(seg.size, c.d, 16, dh, q, c.out);
    if (s.vec) {
      hipLaunchKernelGGL((WeightedSegmentReduceFp8Vec16Kernel<MODE, OUT>), dim3(s.blocks), dim3(64, 4), 0, st,
                         reinterpret_cast<const uint4*>(q), c.fp8_scale, seg, ix, (int32_t)s.dv, c.out, c.w,
                         c.w_dtype, c.heads, dh);
    } else {
      hipLaunchKernelGGL((WeightedSegmentReduceFp8Kernel<MODE, OUT>), dim3(s.blocks), dim3(64, 4), 0, st, q,
                         c.fp8_scale, seg, ix, c.d, c.out, c.w, c.w_dtype, c.heads, dh);
    }
  }
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

size_t DtypeBytes(int32_t dt) { return dt == EULER_GPU_F32 ? 4 : 2; }

}  // namespace

// c.out_dtype is any of the three (CheckMpReduce)
int ReduceFp8(hipStream_t st, const MpReduceCall& c, const SegSpec& seg, const MpwIndex& ix) {
#define EG_REDUCE(M)                                                                  \
  return c.out_dtype == EULER_GPU_F32    ? LaunchReduce<M, kF32>(st, c, seg, ix)      \
         : c.out_dtype == EULER_GPU_BF16 ? LaunchReduce<M, kBF16>(st, c, seg, ix)     \
                                         : LaunchReduce<M, kF16>(st, c, seg, ix)
  if (c.mode == 0) { EG_REDUCE(0); }
  if (c.mode == 1) { EG_REDUCE(1); }
  EG_REDUCE(2);
#undef EG_REDUCE
}

}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_column_absmax(void* stream, const void* x_dev, int32_t dtype, int64_t n, int64_t d,
                            float* absmax_dev) {
  const auto fail = [](const std::string& why) { return Fail(EULER_GPU_EINVAL, "column_absmax: " + why); };
  if (!KnownDtype(dtype)) return fail("unknown dtype " + std::to_string(dtype) + kDtypeCodes);
  if (n < 0 || d < 0) return fail("bad shape");
  if (n == 0 || d == 0) return EULER_GPU_OK;
  if (!x_dev || !absmax_dev) return fail("null buffer");
  if ((uintptr_t)x_dev % DtypeBytes(dtype) != 0 || (uintptr_t)absmax_dev % 4 != 0)
    return fail("a buffer is not aligned to its type");
  hipStream_t st = (hipStream_t)stream;
  const int64_t by = std::min<int64_t>((d + 63) / 64, 1024);
  const int64_t bx = std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, 8192 / by));
  const dim3 grid((unsigned)bx, (unsigned)by), block(64, 4);
  uint32_t* m = reinterpret_cast<uint32_t*>(absmax_dev);
  if (dtype == EULER_GPU_F32) hipLaunchKernelGGL(ColumnAbsmaxKernel<kF32>, grid, block, 0, st, x_dev, n, d, m);
  else if (dtype == EULER_GPU_BF16) hipLaunchKernelGGL(ColumnAbsmaxKernel<kBF16>, grid, block, 0, st, x_dev, n, d, m);
  else hipLaunchKernelGGL(ColumnAbsmaxKernel<kF16>, grid, block, 0, st, x_dev, n, d, m);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_fp8_quantize_rows(void* stream, const void* x_dev, int32_t dtype, int64_t n, int64_t d,
                                const float* scale_dev, uint8_t* q_dev) {
  const auto fail = [](const std::string& why) { return Fail(EULER_GPU_EINVAL, "fp8_quantize_rows: " + why); };
  if (!KnownDtype(dtype)) return fail("unknown dtype " + std::to_string(dtype) + kDtypeCodes);
  if (n < 0 || d < 0) return fail("bad shape");
  if (n == 0 || d == 0) return EULER_GPU_OK;
  if (!x_dev || !scale_dev || !q_dev) return fail("null buffer");
  if ((uintptr_t)x_dev % DtypeBytes(dtype) != 0 || (uintptr_t)scale_dev % 4 != 0)
    return fail("a buffer is not aligned to its type");
  hipStream_t st = (hipStream_t)stream;
  const int block = 256;
  const dim3 grid(GridFor(n * d, block));
  if (dtype == EULER_GPU_F32)
    hipLaunchKernelGGL(QuantizeRowsKernel<kF32>, grid, dim3(block), 0, st, x_dev, n, d, scale_dev, q_dev);
  else if (dtype == EULER_GPU_BF16)
    hipLaunchKernelGGL(QuantizeRowsKernel<kBF16>, grid, dim3(block), 0, st, x_dev, n, d, scale_dev, q_dev);
  else
    hipLaunchKernelGGL(QuantizeRowsKernel<kF16>, grid, dim3(block), 0, st, x_dev, n, d, scale_dev, q_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_fp8_gather(void* stream, const uint8_t* q_dev, const float* scale_dev,
                         const int32_t* indices_dev, int64_t e, int64_t d, int64_t n_rows, void* out_dev,
                         int32_t out_dtype) {
  (void)n_rows;      // (as euler_gpu_gather: the indices are trusted)
  const auto fail = [](const std::string& why) { return Fail(EULER_GPU_EINVAL, "fp8_gather: " + why); };
  if (!KnownDtype(out_dtype)) return fail("unknown out_dtype " + std::to_string(out_dtype) + kDtypeCodes);
  if (e < 0 || d < 0) return fail("bad shape");
  if (e == 0 || d == 0) return EULER_GPU_OK;
  if (!q_dev || !scale_dev || !indices_dev || !out_dev) return fail("null buffer");
  if ((uintptr_t)out_dev % DtypeBytes(out_dtype) != 0 || (uintptr_t)scale_dev % 4 != 0)
    return fail("a buffer is not aligned to its type");
  hipStream_t st = (hipStream_t)stream;
  const int block = 256;
  // elements a lane: fp32 out 4 (4-byte loads, 16-byte stores), 16-bit out 16 (16-byte loads and stores), else 1
  const bool f32 = out_dtype == EULER_GPU_F32;
  const bool vec = f32 ? d % 4 == 0 && (uintptr_t)q_dev % 4 == 0 && (uintptr_t)out_dev % 16 == 0
                       : d % 16 == 0 && ((uintptr_t)q_dev | (uintptr_t)out_dev) % 16 == 0;
  const int64_t dv = !vec ? d : f32 ? d / 4 : d / 16;
  const dim3 grid(GridFor(e * dv, block));
#define EG_GATHER(OUT, N)                                                                              \
  if (vec) hipLaunchKernelGGL((Fp8GatherKernel<OUT, N>), grid, dim3(block), 0, st, q_dev, scale_dev,   \
                              indices_dev, e, dv, out_dev);                                            \
  else hipLaunchKernelGGL((Fp8GatherKernel<OUT, 1>), grid, dim3(block), 0, st, q_dev, scale_dev,       \
                          indices_dev, e, dv, out_dev)
  if (f32) { EG_GATHER(kF32, 4); }
  else if (out_dtype == EULER_GPU_BF16) { EG_GATHER(kBF16, 16); }
  else { EG_GATHER(kF16, 16); }
#undef EG_GATHER
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_fp8_gather_segment_reduce(void* stream, int32_t mode, const uint8_t* q_dev,
                                        const float* scale_dev, const int32_t* gather_indices_dev,
                                        const int64_t* seg_ptr_dev, int64_t count, int64_t d, int32_t size,
                                        void* out_dev, int32_t out_dtype, const void* w_dev,
                                        int32_t w_dtype, int32_t heads) {
  MpReduceCall c{"fp8_gather_segment_reduce", mode, q_dev, d, size, out_dev};
  c.Fp8(scale_dev, out_dtype).Gather(kGatherOrNull, gather_indices_dev).Segments(seg_ptr_dev, count);
  if (w_dev) c.Weights(w_dev, heads, w_dtype);
  return RunMpReduce((hipStream_t)stream, c);
}

int euler_gpu_fp8_gather_segment_reduce_ids(void* stream, int32_t mode, const uint8_t* q_dev,
                                            const float* scale_dev, int64_t params_rows,
                                            const int64_t* gather_ids_dev, const int64_t* seg_ptr_dev,
                                            int64_t count, int64_t d, int32_t size, void* out_dev,
                                            int32_t out_dtype, const void* w_dev, int32_t w_dtype,
                                            int32_t heads) {
  MpReduceCall c{"fp8_gather_segment_reduce_ids", mode, q_dev, d, size, out_dev};
  c.Fp8(scale_dev, out_dtype).Gather(kGatherIds, gather_ids_dev, params_rows).Segments(seg_ptr_dev, count);
  if (w_dev) c.Weights(w_dev, heads, w_dtype);
  return RunMpReduce((hipStream_t)stream, c);
}

}  // extern "C"
