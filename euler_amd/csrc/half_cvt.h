// Conversions between fp32 and the two 16-bit storage formats of the message-passing and
// dense-feature kernels (bf16, IEEE fp16).  Widening is exact; narrowing rounds to nearest,
// ties to even, NaN -> quiet NaN (sign kept), overflow -> inf, fp16 subnormals produced and
// read.  The HOST forms are plain integer C++ (tests/csrc/half_cvt_check.cc pins them against
// torch's CPU conversions); the DEVICE forms are casts the compiler lowers to the gfx950
// convert instructions (v_cvt_pk_bf16_f32, v_cvt_f16_f32, v_cvt_f32_f16), which round the same
// way - finite values and infinities have the same bits on both sides, and a NaN comes out
// quiet with its sign.  tests/test_half_cvt_gpu.py pins the device forms against the same CPU
// conversions on the same patterns (tests/half_edges.py: every 16-bit pattern widened; ties,
// subnormals of both formats, overflow, inf and NaN narrowed), and
// tests/test_half_store_edges_gpu.py every op's own 16-bit store at those edges.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EG_CVT_HD __host__ __device__ __forceinline__
#else
#define EG_CVT_HD inline
#endif

namespace euler_gpu {

// storage types of a typed entry point (EULER_GPU_F32 / _BF16 / _F16 of euler_gpu.h)
constexpr int kF32 = 0, kBF16 = 1, kF16 = 2;

EG_CVT_HD uint32_t F32Bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
EG_CVT_HD float BitsF32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// ---- integer forms (the definition; what the host runs) ----------------------------------
EG_CVT_HD float Bf16ToF32Int(uint16_t h) { return BitsF32((uint32_t)h << 16); }

EG_CVT_HD uint16_t F32ToBf16Int(float f) {
  uint32_t u = F32Bits(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);   // NaN: quiet bit
  u += 0x7fffu + ((u >> 16) & 1u);              // ties to even; a carry out of the mantissa
  return (uint16_t)(u >> 16);                   // steps the exponent (up to inf)
}

EG_CVT_HD float F16ToF32Int(uint16_t h) {
  const uint32_t sign = ((uint32_t)h & 0x8000u) << 16;
  const uint32_t e = (h >> 10) & 31u;
  uint32_t m = h & 0x3ffu;
  if (e == 31u) return BitsF32(sign | 0x7f800000u | (m ? 0x400000u : 0u) | (m << 13));
  if (e == 0u) {
    if (m == 0u) return BitsF32(sign);
    int shift = 0;                              // subnormal: m * 2^-24, normalised
    while (!(m & 0x400u)) { m <<= 1; ++shift; }
    return BitsF32(sign | ((uint32_t)(113 - shift) << 23) | ((m & 0x3ffu) << 13));
  }
  return BitsF32(sign | ((e + 112u) << 23) | (m << 13));
}

EG_CVT_HD uint16_t F32ToF16Int(float f) {
  const uint32_t u = F32Bits(f);
  const uint32_t sign = (u >> 16) & 0x8000u;
  const uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((a >> 13) & 0x1ffu));   // quiet NaN
  if (a >= 0x38800000u) {                       // >= 2^-14: a normal fp16 (or inf)
    uint32_t r = a - 0x38000000u;               // exponent bias 127 -> 15
    r += 0xfffu + ((r >> 13) & 1u);
    r >>= 13;
    return (uint16_t)(sign | (r >= 0x7c00u ? 0x7c00u : r));
  }
  if (a <= 0x33000000u) return (uint16_t)sign;  // <= 2^-25 (the tie with 0 goes to even 0)
  const uint32_t m = (a & 0x7fffffu) | 0x800000u;
  const uint32_t shift = 126u - (a >> 23);      // 14 .. 24: value = m * 2^(e - 150) in units of 2^-24
  uint32_t r = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
  if (rem > half || (rem == half && (r & 1u))) ++r;      // (0x400 = the smallest normal)
  return (uint16_t)(sign | r);
}

// ---- what the kernels call ----------------------------------------------------------------
template <int DT> struct HalfCvt;

template <> struct HalfCvt<kBF16> {
  static EG_CVT_HD float Widen(uint16_t h) { return Bf16ToF32Int(h); }        // a shift
  static EG_CVT_HD uint16_t Narrow(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __bf16 b = (__bf16)f;
    uint16_t r; __builtin_memcpy(&r, &b, 2); return r;
#else
    return F32ToBf16Int(f);
#endif
  }
};

template <> struct HalfCvt<kF16> {
  static EG_CVT_HD float Widen(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    _Float16 x; __builtin_memcpy(&x, &h, 2); return (float)x;
#else
    return F16ToF32Int(h);
#endif
  }
  static EG_CVT_HD uint16_t Narrow(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    const _Float16 x = (_Float16)f;
    uint16_t r; __builtin_memcpy(&r, &x, 2); return r;
#else
    return F32ToF16Int(f);
#endif
  }
};

// Packed forms: a 32-bit word holds elements (2 i, 2 i + 1) little endian, a 16-byte load
// eight elements.
template <int DT>
EG_CVT_HD void Widen2(uint32_t w, float* lo, float* hi) {
  *lo = HalfCvt<DT>::Widen((uint16_t)(w & 0xffffu));
  *hi = HalfCvt<DT>::Widen((uint16_t)(w >> 16));
}
template <>
EG_CVT_HD void Widen2<kBF16>(uint32_t w, float* lo, float* hi) {
  *lo = BitsF32(w << 16);
  *hi = BitsF32(w & 0xffff0000u);
}

template <int DT>
EG_CVT_HD uint32_t Narrow2(float lo, float hi) {
  return (uint32_t)HalfCvt<DT>::Narrow(lo) | ((uint32_t)HalfCvt<DT>::Narrow(hi) << 16);
}

template <int DT>
EG_CVT_HD void Widen8(const uint32_t w[4], float f[8]) {
  for (int i = 0; i < 4; ++i) Widen2<DT>(w[i], &f[2 * i], &f[2 * i + 1]);
}

template <int DT>
EG_CVT_HD void Narrow8(const float f[8], uint32_t w[4]) {
  for (int i = 0; i < 4; ++i) w[i] = Narrow2<DT>(f[2 * i], f[2 * i + 1]);
}

}  // namespace euler_gpu
