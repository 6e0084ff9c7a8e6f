// Message passing and dense features over 16-bit storage (bf16 / IEEE fp16) for gfx950, and
// their C-ABI entry points (the *_t entries of euler_gpu.h).
//
// Contract: a typed op on 16-bit input x is the fp32 op of mp_kernels.hip on the widened x
// (widening is exact) - the same fp32 adds in input order, the same compares, the same
// divide by (length + 1e-7f) - and the result is stored as fp32 unchanged or rounded ONCE to
// the storage type (nearest, ties to even).  Nothing is accumulated in 16 bits.  What changes
// is the bytes: these kernels stream HBM, and a row is half as long.
//
// Lane roles follow the fp32 kernels with the element count per 16-byte access doubled: a
// lane of the vector kernels owns EIGHT adjacent columns (one 16-byte load per update row,
// eight fp32 accumulators in VGPRs, one 16-byte store of 16-bit results or two of fp32), d / 8
// lanes a row, 512 / d rows a wave.
#include <hip/hip_runtime.h>

#include "device_fns.h"
#include "device_mem.h"
#include "half_cvt.h"
#include "mp_segments.h"
#include "mp_weighted.h"

namespace euler_gpu {
namespace {

template <int DT>
__device__ __forceinline__ float LoadElem(const void* p, int64_t i) {
  if constexpr (DT == kF32) return static_cast<const float*>(p)[i];
  else return HalfCvt<DT>::Widen(static_cast<const uint16_t*>(p)[i]);
}

template <int DT>
__device__ __forceinline__ void StoreElem(void* p, int64_t i, float v) {
  if constexpr (DT == kF32) static_cast<float*>(p)[i] = v;
  else static_cast<uint16_t*>(p)[i] = HalfCvt<DT>::Narrow(v);
}

template <int DT>
__device__ __forceinline__ void Widen8V(const uint4 v, float f[8]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  Widen8<DT>(w, f);
}

// eight results of a lane: one 16-byte store of 16-bit values, or two of fp32
template <int DT, bool OUT16>
__device__ __forceinline__ void Store8(void* out, int64_t slot, const float f[8]) {
  if constexpr (OUT16) {
    uint32_t w[4];
    Narrow8<DT>(f, w);
    static_cast<uint4*>(out)[slot] = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    float4* o = static_cast<float4*>(out) + slot * 2;
    o[0] = make_float4(f[0], f[1], f[2], f[3]);
    o[1] = make_float4(f[4], f[5], f[6], f[7]);
  }
}

template <bool IS_MAX>
__device__ __forceinline__ void Accumulate8(float acc[8], const float f[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (IS_MAX) acc[k] = f[k] > acc[k] ? f[k] : acc[k];
    else acc[k] = __fadd_rn(acc[k], f[k]);
  }
}

__device__ __forceinline__ int64_t UpdateRow(const uint32_t* perm, const int32_t* gsrc,
                                             int32_t gstride, uint32_t row_max, int64_t p) {
  int64_t src = perm ? (int64_t)perm[p] : p;
  if (gsrc) src = (int32_t)min((uint32_t)gsrc[src * gstride], row_max);
  return src;
}

// SegmentReduceKernel of mp_kernels.hip over 16-bit updates: blockDim = (64, 4), a wave-slot
// per output row, one column per lane.  Serves every d the vector kernel does not.
template <int MODE, int DT, bool OUT16>
__global__ __launch_bounds__(256) void SegmentReduceHalfKernel(
    const uint16_t* __restrict__ upd, const SegSpec seg, const uint32_t* __restrict__ perm,
    const int32_t* __restrict__ gsrc, int64_t d, void* __restrict__ out, const int32_t gstride,
    const uint32_t row_max) {
  constexpr bool IS_MAX = MODE == 1;
  const int lane = threadIdx.x;
  const int32_t size = seg.size;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; r < size;
       r += (int64_t)gridDim.x * blockDim.y) {
    int64_t b, en;
    SegBounds(seg, r, &b, &en);
    const float denom = __fadd_rn((float)(en - b), 1e-7f);
    for (int64_t c = lane; c < d; c += 64) {
      float acc = IS_MAX ? (float)-1e9 : 0.f;
      int64_t p = b;
      // adds in input order; the loads are issued eight at a time
      for (; p + 8 <= en; p += 8) {
        uint16_t v[8];
#pragma unroll
        for (int x = 0; x < 8; ++x)
          v[x] = upd[UpdateRow(perm, gsrc, gstride, row_max, p + x) * d + c];
#pragma unroll
        for (int x = 0; x < 8; ++x) {
          const float f = HalfCvt<DT>::Widen(v[x]);
          if (IS_MAX) { if (f > acc) acc = f; }
          else acc = __fadd_rn(acc, f);
        }
      }
      for (; p < en; ++p) {
        const float f = HalfCvt<DT>::Widen(upd[UpdateRow(perm, gsrc, gstride, row_max, p) * d + c]);
        if (IS_MAX) { if (f > acc) acc = f; }
        else acc = __fadd_rn(acc, f);
      }
      if (MODE == 2) acc = __fdiv_rn(acc, denom);
      StoreElem<OUT16 ? DT : kF32>(out, r * d + c, acc);
    }
  }
}

// d % 8 == 0 with d / 8 a divisor of 64 (d = 8 .. 512): a lane owns eight adjacent columns,
// d8 = d / 8 lanes a row, 64 / d8 rows a wave.
template <int MODE, int DT, bool OUT16>
__global__ __launch_bounds__(256) void SegmentReduceVec8Kernel(
    const uint4* __restrict__ u8, const SegSpec seg, const uint32_t* __restrict__ perm,
    const int32_t* __restrict__ gsrc, int32_t d8, void* __restrict__ out, const int32_t gstride,
    const uint32_t row_max) {
  constexpr bool IS_MAX = MODE == 1;
  const int32_t size = seg.size;
  const int32_t rows_per_wave = 64 / d8;
  const int32_t sub = threadIdx.x / d8, cl = threadIdx.x - sub * d8;
  const int64_t rows_per_block = (int64_t)blockDim.y * rows_per_wave;
  for (int64_t r = (int64_t)blockIdx.x * rows_per_block + threadIdx.y * rows_per_wave + sub;
       r < size; r += (int64_t)gridDim.x * rows_per_block) {
    int64_t b, en;
    SegBounds(seg, r, &b, &en);
    const float denom = __fadd_rn((float)(en - b), 1e-7f);
    const float init = IS_MAX ? (float)-1e9 : 0.f;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = init;
    int64_t p = b;
    // the row numbers first, then the eight rows, then the ordered adds
    for (; p + 8 <= en; p += 8) {
      int64_t src[8];
#pragma unroll
      for (int x = 0; x < 8; ++x) src[x] = perm ? (int64_t)perm[p + x] : p + x;
      if (gsrc) {
#pragma unroll
        for (int x = 0; x < 8; ++x) src[x] = (int32_t)min((uint32_t)gsrc[src[x] * gstride], row_max);
      }
      uint4 v[8];
#pragma unroll
      for (int x = 0; x < 8; ++x) v[x] = u8[src[x] * d8 + cl];
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        float f[8];
        Widen8V<DT>(v[x], f);
        Accumulate8<IS_MAX>(acc, f);
      }
    }
    for (; p + 4 <= en; p += 4) {
      uint4 v[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) v[x] = u8[UpdateRow(perm, gsrc, gstride, row_max, p + x) * d8 + cl];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        float f[8];
        Widen8V<DT>(v[x], f);
        Accumulate8<IS_MAX>(acc, f);
      }
    }
    for (; p < en; ++p) {
      float f[8];
      Widen8V<DT>(u8[UpdateRow(perm, gsrc, gstride, row_max, p) * d8 + cl], f);
      Accumulate8<IS_MAX>(acc, f);
    }
    if (MODE == 2) {
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = __fdiv_rn(acc[k], denom);
    }
    Store8<DT, OUT16>(out, r * d8 + cl, acc);
  }
}

template <int MODE, int DT, bool OUT16>
int LaunchReduce(hipStream_t st, const void* upd, const SegSpec& seg, const MpwIndex& ix, int64_t d,
                 void* out) {
  const LaneShape s = RowLaneShape(seg.size, d, 8, 0, upd, out);
  if (s.vec) {
    hipLaunchKernelGGL((SegmentReduceVec8Kernel<MODE, DT, OUT16>), dim3(s.blocks), dim3(64, 4), 0, st,
                       static_cast<const uint4*>(upd), seg, ix.perm, ix.gsrc, (int32_t)s.dv, out, ix.gstride,
                       ix.row_max);
  } else {
    hipLaunchKernelGGL((SegmentReduceHalfKernel<MODE, DT, OUT16>), dim3(s.blocks), dim3(64, 4), 0, st,
                       static_cast<const uint16_t*>(upd), seg, ix.perm, ix.gsrc, d, out, ix.gstride,
                       ix.row_max);
  }
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

// ---- edge-weighted reduces (the weighted kernels of mp_kernels.hip over 16-bit rows) -----------
// params in bf16 / fp16, w [E, heads] in fp32 or in the dtype of params: both widened exactly,
// the product and the sum in fp32 (WeightedReduceRow of mp_weighted.h), one rounding at the store.
template <int DT>
__device__ __forceinline__ float LoadWeight(const void* w, bool w16, int64_t i) {
  return w16 ? HalfCvt<DT>::Widen(static_cast<const uint16_t*>(w)[i]) : static_cast<const float*>(w)[i];
}

template <int DT>
struct WeightedHalfOps1 {
  using Raw = uint16_t;
  MpwIndex ix;
  const uint16_t* upd; int64_t d; int64_t c;
  const void* w; bool w16; int32_t heads; int32_t head;
  __device__ __forceinline__ int64_t Pos(int64_t p) const { return ix.Pos(p); }
  __device__ __forceinline__ int64_t Row(int64_t pos) const { return ix.Row(pos); }
  __device__ __forceinline__ float Weight(int64_t pos) const { return LoadWeight<DT>(w, w16, pos * heads + head); }
  __device__ __forceinline__ uint16_t Load(int64_t row) const { return upd[row * d + c]; }
  __device__ __forceinline__ void Widen(uint16_t v, float f[1]) const { f[0] = HalfCvt<DT>::Widen(v); }
};

template <int DT>
struct WeightedHalfOps8 {
  using Raw = uint4;
  MpwIndex ix;
  const uint4* u8; int64_t d8; int64_t cl;
  const void* w; bool w16; int32_t heads; int32_t head;
  __device__ __forceinline__ int64_t Pos(int64_t p) const { return ix.Pos(p); }
  __device__ __forceinline__ int64_t Row(int64_t pos) const { return ix.Row(pos); }
  __device__ __forceinline__ float Weight(int64_t pos) const { return LoadWeight<DT>(w, w16, pos * heads + head); }
  __device__ __forceinline__ uint4 Load(int64_t row) const { return u8[row * d8 + cl]; }
  __device__ __forceinline__ void Widen(const uint4& v, float f[8]) const { Widen8V<DT>(v, f); }
};

template <int MODE, int DT, bool OUT16>
__global__ __launch_bounds__(256) void WeightedSegmentReduceHalfKernel(
    const uint16_t* __restrict__ upd, const SegSpec seg, const MpwIndex ix, int64_t d,
    void* __restrict__ out, const void* __restrict__ w, const bool w16, const int32_t heads,
    const int32_t dh) {
  const int lane = threadIdx.x;
  const int32_t size = seg.size;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; r < size;
       r += (int64_t)gridDim.x * blockDim.y) {
    int64_t b, en;
    SegBounds(seg, r, &b, &en);
    for (int64_t c = lane; c < d; c += 64) {
      const WeightedHalfOps1<DT> ops{ix, upd, d, c, w, w16, heads, (int32_t)(c / dh)};
      float acc[1];
      WeightedReduceRow<MODE, 1>(ops, b, en, acc);
      StoreElem<OUT16 ? DT : kF32>(out, r * d + c, acc[0]);
    }
  }
}

// the 16-byte-lane form: d8 = d / 8 lanes a row, and dh % 8 == 0 so that a lane's eight columns
// lie in one head
template <int MODE, int DT, bool OUT16>
__global__ __launch_bounds__(256) void WeightedSegmentReduceVec8Kernel(
    const uint4* __restrict__ u8, const SegSpec seg, const MpwIndex ix, int32_t d8,
    void* __restrict__ out, const void* __restrict__ w, const bool w16, const int32_t heads,
    const int32_t dh) {
  const int32_t size = seg.size;
  const int32_t rows_per_wave = 64 / d8;
  const int32_t sub = threadIdx.x / d8, cl = threadIdx.x - sub * d8;
  const int64_t rows_per_block = (int64_t)blockDim.y * rows_per_wave;
  const WeightedHalfOps8<DT> ops{ix, u8, d8, cl, w, w16, heads, (cl * 8) / dh};
  for (int64_t r = (int64_t)blockIdx.x * rows_per_block + threadIdx.y * rows_per_wave + sub;
       r < size; r += (int64_t)gridDim.x * rows_per_block) {
    int64_t b, en;
    SegBounds(seg, r, &b, &en);
    float acc[8];
    WeightedReduceRow<MODE, 8>(ops, b, en, acc);
    Store8<DT, OUT16>(out, r * d8 + cl, acc);
  }
}

template <int MODE, int DT, bool OUT16>
int LaunchWeightedReduce(hipStream_t st, const void* upd, const SegSpec& seg, const MpwIndex& ix,
                         int64_t d, void* out, const void* w, bool w16, int32_t heads) {
  const int32_t dh = (int32_t)(d / heads);
  const LaneShape s = RowLaneShape(seg.size, d, 8, dh, upd, out);
  if (s.vec) {
    hipLaunchKernelGGL((WeightedSegmentReduceVec8Kernel<MODE, DT, OUT16>), dim3(s.blocks), dim3(64, 4),
                       0, st, static_cast<const uint4*>(upd), seg, ix, (int32_t)s.dv, out, w, w16, heads, dh);
  } else {
    hipLaunchKernelGGL((WeightedSegmentReduceHalfKernel<MODE, DT, OUT16>), dim3(s.blocks), dim3(64, 4),
                       0, st, static_cast<const uint16_t*>(upd), seg, ix, d, out, w, w16, heads, dh);
  }
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

// ---- MPGather ------------------------------------------------------------------------------
// equal storage types: a row copy in the widest unit the shapes allow, no conversion
template <typename V>
__global__ __launch_bounds__(256) void GatherCopyKernel(const V* __restrict__ params,
                                                        const int32_t* __restrict__ idx, int64_t e,
                                                        int64_t dv, V* __restrict__ out) {
  const int64_t total = e * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += stride) {
    const int64_t i = x / dv;
    const int64_t c = x - i * dv;
    out[x] = params[(int64_t)idx[i] * dv + c];
  }
}

// 16-bit rows -> fp32 rows; VEC: eight elements a lane (dv = d / 8), else one (dv = d)
template <int DT, bool VEC>
__global__ __launch_bounds__(256) void GatherWidenKernel(const void* __restrict__ params,
                                                         const int32_t* __restrict__ idx, int64_t e,
                                                         int64_t dv, float* __restrict__ out) {
  const int64_t total = e * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += stride) {
    const int64_t i = x / dv;
    const int64_t c = x - i * dv;
    if constexpr (VEC) {
      float f[8];
      Widen8V<DT>(static_cast<const uint4*>(params)[(int64_t)idx[i] * dv + c], f);
      Store8<DT, false>(out, x, f);
    } else {
      out[x] = LoadElem<DT>(params, (int64_t)idx[i] * dv + c);
    }
  }
}

// ---- dense features ------------------------------------------------------------------------
// DenseFeatureKernel of mp_kernels.hip with the table and the output typed: one lane per
// output element.  `table` is the graph's value array in its storage type.
template <int IN, int OUT>
__global__ __launch_bounds__(256) void DenseFeatureTypedKernel(
    const GraphView g, const void* __restrict__ table, const uint64_t* __restrict__ nodes, int64_t n,
    int32_t fid, int32_t dim, void* __restrict__ out) {
  const int64_t total = n * (int64_t)dim;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < total; s += stride) {
    const int64_t j = s / dim;
    const int32_t c = (int32_t)(s - j * dim);
    int64_t at = -1;
    const int64_t row = FindRow(g, nodes[j]);
    if (row >= 0 && fid >= 0 && fid < g.n_float) {
      const int32_t* idx = g.feat_idx + (g.feat_uniform ? 0 : row * g.n_float);
      const int32_t pre = fid == 0 ? 0 : idx[fid - 1];
      const int32_t now = idx[fid];
      if (c < now - pre) at = (g.feat_uniform ? row * g.feat_stride : g.feat_ptr[row]) + pre + c;
    }
    if constexpr (IN == OUT && IN != kF32) {      // the stored bits as they are
      static_cast<uint16_t*>(out)[s] = at >= 0 ? static_cast<const uint16_t*>(table)[at] : (uint16_t)0;
    } else {
      StoreElem<OUT>(out, s, at >= 0 ? LoadElem<IN>(table, at) : 0.f);
    }
  }
}

// 16-byte lanes over a 16-bit table: eight elements a lane.  dim % 8 == 0, fixed-stride table
// whose rows and slots start on 16-byte boundaries (feat_uniform, stride % 8 == 0, slot begin
// % 8 == 0 - so every slot's length is a multiple of 8 and a lane is inside a slot or past it).
template <int DT, bool OUT16>
__global__ __launch_bounds__(256) void DenseFeatureVec8Kernel(
    const GraphView g, const uint16_t* __restrict__ table, const uint64_t* __restrict__ nodes,
    int64_t n, int32_t fid, int32_t dv /* dim / 8 */, void* __restrict__ out) {
  const int32_t pre = fid == 0 ? 0 : g.feat_idx[fid - 1];
  const int32_t len = g.feat_idx[fid] - pre;
  const uint32_t total = (uint32_t)(n * dv);
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < total; s += stride) {
    const uint32_t j = s / (uint32_t)dv;
    const int32_t c = (int32_t)(s - j * (uint32_t)dv) * 8;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    const int64_t row = FindRow(g, nodes[j]);
    if (row >= 0 && c < len) {      // (then c + 7 < len)
      v = *reinterpret_cast<const uint4*>(table + row * g.feat_stride + pre + c);
    }
    if constexpr (OUT16) {
      static_cast<uint4*>(out)[s] = v;
    } else {
      float f[8];
      Widen8V<DT>(v, f);
      Store8<DT, false>(out, s, f);
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256) void NarrowTableKernel(const float* __restrict__ in, int64_t n,
                                                         uint16_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = HalfCvt<DT>::Narrow(in[i]);
}

}  // namespace

// c.in_dtype is bf16 or fp16, c.out_dtype fp32 or c.in_dtype (CheckMpReduce)
#define EG_BY_MODE_DTYPE(LAUNCH)                \
  if (c.in_dtype == EULER_GPU_BF16) {           \
    if (c.mode == 0) { LAUNCH(0, kBF16); }      \
    if (c.mode == 1) { LAUNCH(1, kBF16); }      \
    LAUNCH(2, kBF16);                           \
  }                                             \
  if (c.mode == 0) { LAUNCH(0, kF16); }         \
  if (c.mode == 1) { LAUNCH(1, kF16); }         \
  LAUNCH(2, kF16)

int ReduceHalf(hipStream_t st, const MpReduceCall& c, const SegSpec& seg, const MpwIndex& ix) {
#define EG_REDUCE(M, DT)                                                                     \
  return c.out_dtype == EULER_GPU_F32 ? LaunchReduce<M, DT, false>(st, c.params, seg, ix, c.d, c.out) \
                                      : LaunchReduce<M, DT, true>(st, c.params, seg, ix, c.d, c.out)
  EG_BY_MODE_DTYPE(EG_REDUCE);
#undef EG_REDUCE
}

int WeightedReduceHalf(hipStream_t st, const MpReduceCall& c, const SegSpec& seg, const MpwIndex& ix) {
  const bool w16 = c.w_dtype != EULER_GPU_F32;
#define EG_WREDUCE(M, DT)                                                                               \
  return c.out_dtype == EULER_GPU_F32                                                                   \
             ? LaunchWeightedReduce<M, DT, false>(st, c.params, seg, ix, c.d, c.out, c.w, w16, c.heads) \
             : LaunchWeightedReduce<M, DT, true>(st, c.params, seg, ix, c.d, c.out, c.w, w16, c.heads)
  EG_BY_MODE_DTYPE(EG_WREDUCE);
#undef EG_WREDUCE
}
#undef EG_BY_MODE_DTYPE

}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_gather_t(void* stream, const void* params_dev, int32_t in_dtype,
                       const int32_t* indices_dev, int64_t e, int64_t d, int64_t n_params,
                       void* out_dev, int32_t out_dtype) {
  if (!KnownDtype(in_dtype))
    return Fail(EULER_GPU_EINVAL, "gather: unknown dtype " + std::to_string(in_dtype) + kDtypeCodes);
  if (out_dtype != EULER_GPU_F32 && out_dtype != in_dtype)
    return Fail(EULER_GPU_EINVAL, "gather: out_dtype " + std::to_string(out_dtype) +
                                      " is neither fp32 nor the input's dtype");
  if (in_dtype == EULER_GPU_F32)
    return euler_gpu_gather(stream, static_cast<const float*>(params_dev), indices_dev, e, d, n_params,
                            static_cast<float*>(out_dev));
  if (e < 0 || d < 0) return Fail(EULER_GPU_EINVAL, "gather: bad shape");
  if (e == 0 || d == 0) return EULER_GPU_OK;
  if (!params_dev || !indices_dev || !out_dev) return Fail(EULER_GPU_EINVAL, "gather: null buffer");
  if ((uintptr_t)params_dev % 2 != 0 || (uintptr_t)out_dev % 2 != 0)
    return Fail(EULER_GPU_EINVAL, "gather: 16-bit data must be 2-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int block = 256;
  const uintptr_t both = (uintptr_t)params_dev | (uintptr_t)out_dev;
  if (out_dtype == in_dtype) {
    if (d % 8 == 0 && both % 16 == 0) {
      hipLaunchKernelGGL(GatherCopyKernel<uint4>, dim3(GridFor(e * d / 8, block)), dim3(block), 0, st,
                         static_cast<const uint4*>(params_dev), indices_dev, e, d / 8,
                         static_cast<uint4*>(out_dev));
    } else if (d % 2 == 0 && both % 4 == 0) {
      hipLaunchKernelGGL(GatherCopyKernel<uint32_t>, dim3(GridFor(e * d / 2, block)), dim3(block), 0, st,
                         static_cast<const uint32_t*>(params_dev), indices_dev, e, d / 2,
                         static_cast<uint32_t*>(out_dev));
    } else {
      hipLaunchKernelGGL(GatherCopyKernel<uint16_t>, dim3(GridFor(e * d, block)), dim3(block), 0, st,
                         static_cast<const uint16_t*>(params_dev), indices_dev, e, d,
                         static_cast<uint16_t*>(out_dev));
    }
  } else {
    const bool vec = d % 8 == 0 && both % 16 == 0;
    const int64_t dv = vec ? d / 8 : d;
    const dim3 grid(GridFor(e * dv, block));
    float* o = static_cast<float*>(out_dev);
    if (in_dtype == EULER_GPU_BF16) {
      if (vec) hipLaunchKernelGGL((GatherWidenKernel<kBF16, true>), grid, dim3(block), 0, st, params_dev, indices_dev, e, dv, o);
      else hipLaunchKernelGGL((GatherWidenKernel<kBF16, false>), grid, dim3(block), 0, st, params_dev, indices_dev, e, dv, o);
    } else {
      if (vec) hipLaunchKernelGGL((GatherWidenKernel<kF16, true>), grid, dim3(block), 0, st, params_dev, indices_dev, e, dv, o);
      else hipLaunchKernelGGL((GatherWidenKernel<kF16, false>), grid, dim3(block), 0, st, params_dev, indices_dev, e, dv, o);
    }
  }
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_scatter_t(void* stream, int32_t mode, const void* updates_dev, int32_t in_dtype,
                        const int32_t* indices_dev, int64_t e, int64_t d, int32_t size,
                        void* out_dev, int32_t out_dtype) {
  return RunMpReduce((hipStream_t)stream, MpReduceCall{"scatter", mode, updates_dev, d, size, out_dev}
                                              .Typed(in_dtype, out_dtype).Keys(indices_dev, e));
}

int euler_gpu_gather_scatter_t(void* stream, int32_t mode, const void* params_dev, int32_t in_dtype,
                               const int32_t* gather_indices_dev, const int32_t* scatter_indices_dev,
                               int64_t e, int64_t d, int32_t size, void* out_dev, int32_t out_dtype) {
  return RunMpReduce((hipStream_t)stream,
                     MpReduceCall{"gather_scatter", mode, params_dev, d, size, out_dev}
                         .Typed(in_dtype, out_dtype).Gather(kGatherNeeded, gather_indices_dev)
                         .Keys(scatter_indices_dev, e));
}

int euler_gpu_gather_segment_reduce_t(void* stream, int32_t mode, const void* params_dev, int32_t in_dtype,
                                      const int32_t* gather_indices_dev, const int64_t* seg_ptr_dev,
                                      int64_t count, int64_t d, int32_t size, void* out_dev,
                                      int32_t out_dtype) {
  return RunMpReduce((hipStream_t)stream,
                     MpReduceCall{"gather_segment_reduce", mode, params_dev, d, size, out_dev}
                         .Typed(in_dtype, out_dtype).Gather(kGatherOrNull, gather_indices_dev)
                         .Segments(seg_ptr_dev, count));
}

int euler_gpu_gather_segment_reduce_ids_t(void* stream, int32_t mode, const void* params_dev,
                                          int32_t in_dtype, int64_t params_rows,
                                          const int64_t* gather_ids_dev, const int64_t* seg_ptr_dev,
                                          int64_t count, int64_t d, int32_t size, void* out_dev,
                                          int32_t out_dtype) {
  return RunMpReduce((hipStream_t)stream,
                     MpReduceCall{"gather_segment_reduce_ids", mode, params_dev, d, size, out_dev}
                         .Typed(in_dtype, out_dtype).Gather(kGatherIds, gather_ids_dev, params_rows)
                         .Segments(seg_ptr_dev, count));
}

int euler_gpu_gather_scatter_w_t(void* stream, int32_t mode, const void* params_dev, int32_t in_dtype,
                                 const int32_t* gather_indices_dev, const int32_t* scatter_indices_dev,
                                 int64_t e, int64_t d, int32_t size, void* out_dev, int32_t out_dtype,
                                 const void* w_dev, int32_t w_dtype, int32_t heads) {
  return RunMpReduce((hipStream_t)stream,
                     MpReduceCall{"gather_scatter_w", mode, params_dev, d, size, out_dev}
                         .Typed(in_dtype, out_dtype).Gather(kGatherOrNull, gather_indices_dev)
                         .Keys(scatter_indices_dev, e).Weights(w_dev, heads, w_dtype));
}

int euler_gpu_gather_segment_reduce_w_t(void* stream, int32_t mode, const void* params_dev, int32_t in_dtype,
                                        const int32_t* gather_indices_dev, const int64_t* seg_ptr_dev,
                                        int64_t count, int64_t d, int32_t size, void* out_dev,
                                        int32_t out_dtype, const void* w_dev, int32_t w_dtype,
                                        int32_t heads) {
  return RunMpReduce((hipStream_t)stream,
                     MpReduceCall{"gather_segment_reduce_w", mode, params_dev, d, size, out_dev}
                         .Typed(in_dtype, out_dtype).Gather(kGatherOrNull, gather_indices_dev)
                         .Segments(seg_ptr_dev, count).Weights(w_dev, heads, w_dtype));
}

int euler_gpu_gather_segment_reduce_ids_w_t(void* stream, int32_t mode, const void* params_dev,
                                            int32_t in_dtype, int64_t params_rows,
                                            const int64_t* gather_ids_dev, const int64_t* seg_ptr_dev,
                                            int64_t count, int64_t d, int32_t size, void* out_dev,
                                            int32_t out_dtype, const void* w_dev, int32_t w_dtype,
                                            int32_t heads) {
  return RunMpReduce((hipStream_t)stream,
                     MpReduceCall{"gather_segment_reduce_ids_w", mode, params_dev, d, size, out_dev}
                         .Typed(in_dtype, out_dtype).Gather(kGatherIds, gather_ids_dev, params_rows)
                         .Segments(seg_ptr_dev, count).Weights(w_dev, heads, w_dtype));
}

int32_t euler_gpu_graph_dense_feature_dtype(const euler_gpu_graph* g) {
  return g ? g->feat_dtype : -1;
}

int euler_gpu_graph_set_dense_feature_dtype(euler_gpu_graph* g, void* stream, int32_t dtype) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "set_dense_feature_dtype: null graph");
  if (!KnownDtype(dtype))
    return Fail(EULER_GPU_EINVAL, "set_dense_feature_dtype: unknown dtype " + std::to_string(dtype) + kDtypeCodes);
  if (g->feat_dtype == dtype) return EULER_GPU_OK;
  if (g->feat_dtype != EULER_GPU_F32)
    return Fail(EULER_GPU_EINVAL, "set_dense_feature_dtype: the table is already stored in 16 bits "
                                  "(the fp32 values are gone)");
  if (g->shards > 1)
    return Fail(EULER_GPU_EINVAL, "set_dense_feature_dtype: not on a shard of a sharded graph");
  const GraphView& v = g->view;
  if (v.n_float <= 0 || !v.feat_ptr || !v.feat_idx)
    return Fail(EULER_GPU_EINVAL, "set_dense_feature_dtype: the graph has no dense features");
  DeviceGuard dg(g->device);
  hipStream_t st = (hipStream_t)stream;
  int64_t total = 0;
  EG_HIP(hipMemcpyAsync(&total, v.feat_ptr + v.n_rows, 8, hipMemcpyDeviceToHost, st));
  std::vector<int32_t> ends((size_t)v.n_float);
  EG_HIP(hipMemcpyAsync(ends.data(), v.feat_idx, ends.size() * 4, hipMemcpyDeviceToHost, st));
  EG_HIP(hipStreamSynchronize(st));
  AllocList a("set_dense_feature_dtype: ");
  uint16_t* table = a.Alloc<uint16_t>((size_t)total);
  if (!table) return a.rc;
  if (total > 0) {
    const int block = 256;
    if (dtype == EULER_GPU_BF16)
      hipLaunchKernelGGL(NarrowTableKernel<kBF16>, dim3(GridFor(total, block)), dim3(block), 0, st,
                         v.feat_val, total, table);
    else
      hipLaunchKernelGGL(NarrowTableKernel<kF16>, dim3(GridFor(total, block)), dim3(block), 0, st,
                         v.feat_val, total, table);
  }
  // (a device-wide wait: no launch on any stream may still read the fp32 table)
  const hipError_t le = hipGetLastError();
  const hipError_t se = le == hipSuccess ? hipDeviceSynchronize() : le;
  if (se != hipSuccess) {
    a.Release();
    return Fail(EULER_GPU_EHIP, std::string("set_dense_feature_dtype: ") + hipGetErrorString(se));
  }
  const void* old = v.feat_val;
  auto it = std::find_if(g->allocations.begin(), g->allocations.end(),
                         [old](const std::pair<void*, int64_t>& x) { return x.first == old; });
  if (it != g->allocations.end()) {
    (void)hipFree(it->first);
    g->bytes -= it->second;
    g->allocations.erase(it);
  }
  g->bytes += a.HandOver(&g->allocations);
  bool aligned8 = v.feat_uniform != 0 && v.feat_stride % 8 == 0;
  for (int32_t f = 0; aligned8 && f + 1 < v.n_float; ++f) aligned8 = ends[(size_t)f] % 8 == 0;
  g->view.feat_val = nullptr;
  g->feat16 = table;
  g->feat_dtype = dtype;
  g->feat_slot_aligned8 = aligned8;
  return EULER_GPU_OK;
}

int euler_gpu_get_dense_feature_t(const euler_gpu_graph* g, void* stream, const uint64_t* nodes_dev,
                                  int64_t n, int32_t fid, int32_t dim, void* out_dev, int32_t out_dtype) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "get_dense_feature: null graph");
  const int32_t in_dtype = g->feat_dtype;
  if (!KnownDtype(out_dtype))
    return Fail(EULER_GPU_EINVAL, "get_dense_feature: unknown dtype " + std::to_string(out_dtype) + kDtypeCodes);
  // an fp32 table serves every output type (one rounding at the store); a 16-bit one fp32 or its own
  if (in_dtype != EULER_GPU_F32 && out_dtype != EULER_GPU_F32 && out_dtype != in_dtype)
    return Fail(EULER_GPU_EINVAL, "get_dense_feature: out_dtype " + std::to_string(out_dtype) +
                                      " is neither fp32 nor the table's dtype");
  if (in_dtype == EULER_GPU_F32 && out_dtype == EULER_GPU_F32)
    return euler_gpu_get_dense_feature(g, stream, nodes_dev, n, fid, dim, static_cast<float*>(out_dev));
  if (n < 0 || dim < 0) return Fail(EULER_GPU_EINVAL, "get_dense_feature: bad n/dim");
  if (n == 0 || dim == 0) return EULER_GPU_OK;
  if (!nodes_dev || !out_dev) return Fail(EULER_GPU_EINVAL, "get_dense_feature: null buffer");
  const int block = 256;
  hipStream_t st = (hipStream_t)stream;
  const GraphView& v = g->view;
  const dim3 grid(GridFor(n * (int64_t)dim, block));
#define EG_FEAT(IN, OUT, TABLE)                                                                      \
  hipLaunchKernelGGL((DenseFeatureTypedKernel<IN, OUT>), grid, dim3(block), 0, st, v,                \
                     static_cast<const void*>(TABLE), nodes_dev, n, fid, dim, out_dev)
  if (in_dtype == EULER_GPU_F32) {
    if (out_dtype == EULER_GPU_BF16) EG_FEAT(kF32, kBF16, v.feat_val);
    else EG_FEAT(kF32, kF16, v.feat_val);
  } else {
    const bool out16 = out_dtype != EULER_GPU_F32;
    const bool vec8 = v.feat_uniform && fid >= 0 && fid < v.n_float && dim % 8 == 0 &&
                      g->feat_slot_aligned8 && ((uintptr_t)out_dev % 16 == 0) &&
                      n * (int64_t)(dim / 8) < GridForU32Limit(block);  // its loop counts in uint32_t
    const uint16_t* t16 = static_cast<const uint16_t*>(g->feat16);
    if (vec8) {
      const dim3 vgrid(GridFor(n * (int64_t)(dim / 8), block));
#define EG_FEAT8(DT, O16)                                                                            \
  hipLaunchKernelGGL((DenseFeatureVec8Kernel<DT, O16>), vgrid, dim3(block), 0, st, v, t16, nodes_dev, \
                     n, fid, dim / 8, out_dev)
      if (in_dtype == EULER_GPU_BF16) { if (out16) EG_FEAT8(kBF16, true); else EG_FEAT8(kBF16, false); }
      else { if (out16) EG_FEAT8(kF16, true); else EG_FEAT8(kF16, false); }
#undef EG_FEAT8
    } else if (in_dtype == EULER_GPU_BF16) {
      if (out16) EG_FEAT(kBF16, kBF16, t16); else EG_FEAT(kBF16, kF32, t16);
    } else {
      if (out16) EG_FEAT(kF16, kF16, t16); else EG_FEAT(kF16, kF32, t16);
    }
  }
#undef EG_FEAT
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

}  // extern "C"
