// Quantised feature row tables (Fp8Rows): q [N, d] of e4m3fn codes (fp8_cvt.h) and scale [d]
// fp32, one per COLUMN.  The dequantised value is x^[r, c] = fl(Dec(q[r, c]) * scale[c]) - one
// correctly rounded fp32 multiply, never contracted into the add that follows - and an op on the
// table is the fp32 op of mp_kernels.hip on x^: the same adds in input order, the same compares,
// the same divide, stored as fp32 unchanged or rounded once to bf16 / fp16.
//
// Why the scale is per column: a random row read is bounded by the requests and lines it touches
// (DESIGN 4.2), so a scale beside every row would cost a cold line per row; d scales a table are
// read once and stay in registers.  A 128-d row is then exactly one 128-byte line.
//
// This header: the lane's arithmetic - sixteen codes of one 16-byte load (or one code) to fp32 -
// and the Ops of WeightedReduceRow (mp_weighted.h) over such rows; the kernels that assign lanes
// are in fp8_rows_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fp8_cvt.h"
#include "half_cvt.h"
#include "mp_segments.h"
#include "mp_weighted.h"

namespace euler_gpu {

// x^ of one code
__device__ __forceinline__ float Fp8Value(uint8_t code, float scale) {
  return __fmul_rn(Fp8Dec(code), scale);
}

// x^ of the sixteen codes of a 16-byte load; s = the lane's sixteen column scales
__device__ __forceinline__ void Fp8Value16(const uint4& v, const float s[16], float f[16]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  Fp8Dec16(w, f);
#pragma unroll
  for (int k = 0; k < 16; ++k) f[k] = __fmul_rn(f[k], s[k]);
}

// a weight of [E, heads] in fp32 (dt 0), bf16 (1) or fp16 (2), widened exactly
__device__ __forceinline__ float Fp8LoadWeight(const void* w, int32_t dt, int64_t i) {
  if (dt == kF32) return static_cast<const float*>(w)[i];
  const uint16_t h = static_cast<const uint16_t*>(w)[i];
  return dt == kBF16 ? HalfCvt<kBF16>::Widen(h) : HalfCvt<kF16>::Widen(h);
}

struct WeightedFp8Ops1 {
  using Raw = uint8_t;
  MpwIndex ix;
  const uint8_t* q; int64_t d; int64_t c; float scale;
  const void* w; int32_t w_dtype; int32_t heads; int32_t head;
  __device__ __forceinline__ int64_t Pos(int64_t p) const { return ix.Pos(p); }
  __device__ __forceinline__ int64_t Row(int64_t pos) const { return ix.Row(pos); }
  __device__ __forceinline__ float Weight(int64_t pos) const { return Fp8LoadWeight(w, w_dtype, pos * heads + head); }
  __device__ __forceinline__ uint8_t Load(int64_t row) const { return q[row * d + c]; }
  __device__ __forceinline__ void Widen(uint8_t v, float f[1]) const { f[0] = Fp8Value(v, scale); }
};

struct WeightedFp8Ops16 {
  using Raw = uint4;
  MpwIndex ix;
  const uint4* q16; int64_t d16; int64_t cl;
  const void* w; int32_t w_dtype; int32_t heads; int32_t head;
  float s[16];                                  // the lane's sixteen scales
  __device__ __forceinline__ int64_t Pos(int64_t p) const { return ix.Pos(p); }
  __device__ __forceinline__ int64_t Row(int64_t pos) const { return ix.Row(pos); }
  __device__ __forceinline__ float Weight(int64_t pos) const { return Fp8LoadWeight(w, w_dtype, pos * heads + head); }
  __device__ __forceinline__ uint4 Load(int64_t row) const { return q16[row * d16 + cl]; }
  __device__ __forceinline__ void Widen(const uint4& v, float f[16]) const { Fp8Value16(v, s, f); }
};

#pragma GCC visibility push(hidden)
// fp8_rows_kernels.hip: the launchers over an Fp8Rows table (c checked, seg and ix built);
// c.params = q, c.fp8_scale = scale, c.out_dtype any of the three, c.weighted with c.w_dtype
int ReduceFp8(hipStream_t st, const MpReduceCall& c, const SegSpec& seg, const MpwIndex& ix);
#pragma GCC visibility pop

}  // namespace euler_gpu
