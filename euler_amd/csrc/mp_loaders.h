// What one lane loads of a table row in the reduces over a Loader {Raw, Load(row), Widen(raw, f)}
// (gcn_norm_kernels.hip, neighbor_reduce_kernels.hip): a column (fp32 or 16-bit), four fp32
// columns, eight 16-bit columns; the root term of their epilogue, and the store of one element.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "half_cvt.h"

namespace euler_gpu {

struct LoadF32x1 {
  using Raw = float;
  const float* x; int64_t d; int64_t c;
  __device__ __forceinline__ float Load(int64_t row) const { return x[row * d + c]; }
  __device__ __forceinline__ void Widen(float v, float* f) const { f[0] = v; }
};

struct LoadF32x4 {
  using Raw = float4;
  const float4* x4; int64_t d4; int64_t cl;
  __device__ __forceinline__ float4 Load(int64_t row) const { return x4[row * d4 + cl]; }
  __device__ __forceinline__ void Widen(const float4& v, float* f) const {
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  }
};

template <int DT>
struct LoadH16x1 {
  using Raw = uint16_t;
  const uint16_t* x; int64_t d; int64_t c;
  __device__ __forceinline__ uint16_t Load(int64_t row) const { return x[row * d + c]; }
  __device__ __forceinline__ void Widen(uint16_t v, float* f) const { f[0] = HalfCvt<DT>::Widen(v); }
};

template <int DT>
struct LoadH16x8 {
  using Raw = uint4;
  const uint4* x8; int64_t d8; int64_t cl;
  __device__ __forceinline__ uint4 Load(int64_t row) const { return x8[row * d8 + cl]; }
  __device__ __forceinline__ void Widen(const uint4& v, float* f) const {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    Widen8<DT>(w, f);
  }
};

// the one-column loader of a storage type
template <int DT> struct ElemLoader { using type = LoadH16x1<DT>; };
template <> struct ElemLoader<kF32> { using type = LoadF32x1; };

// the root term: [size, d] in fp32 (root32) or in the 16-bit type DT; nullptr: no epilogue
struct GcnRoot {
  const void* p;
  bool root32;
  float agg_scale, root_scale;
};

template <int DT>
__device__ __forceinline__ float RootElem(const GcnRoot& R, int64_t i) {
  if constexpr (DT == kF32) {
    return static_cast<const float*>(R.p)[i];
  } else {
    if (R.root32) return static_cast<const float*>(R.p)[i];
    return HalfCvt<DT>::Widen(static_cast<const uint16_t*>(R.p)[i]);
  }
}

// the eight root elements of vector slot `slot` of a 16-bit reduce (16-byte loads)
template <int DT>
__device__ __forceinline__ void RootElems8(const GcnRoot& R, int64_t slot, float root[8]) {
  if (R.root32) {
    const float4 lo = static_cast<const float4*>(R.p)[slot * 2], hi = static_cast<const float4*>(R.p)[slot * 2 + 1];
    root[0] = lo.x; root[1] = lo.y; root[2] = lo.z; root[3] = lo.w;
    root[4] = hi.x; root[5] = hi.y; root[6] = hi.z; root[7] = hi.w;
  } else {
    const uint4 v = static_cast<const uint4*>(R.p)[slot];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    Widen8<DT>(w, root);
  }
}

template <int DT, bool OUT16>
__device__ __forceinline__ void StoreOne(void* out, int64_t i, float v) {
  if constexpr (OUT16 && DT != kF32) static_cast<uint16_t*>(out)[i] = HalfCvt<DT>::Narrow(v);
  else static_cast<float*>(out)[i] = v;
}

// the eight columns of vector slot `slot`: one 16-byte store in 16 bits, two in fp32
template <int DT, bool OUT16>
__device__ __forceinline__ void StoreEight(void* out, int64_t slot, const float acc[8]) {
  if constexpr (OUT16) {
    uint32_t w[4];
    Narrow8<DT>(acc, w);
    static_cast<uint4*>(out)[slot] = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    float4* o = static_cast<float4*>(out) + slot * 2;
    o[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    o[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
}

}  // namespace euler_gpu
