// Conversions between fp32 and the 8-bit storage format of the quantised feature row tables
// (Fp8Rows: mp_fp8.h, fp8_rows_kernels.hip): OCP e4m3fn - 1 sign, 4 exponent (bias 7) and 3
// mantissa bits, no infinities, one NaN per sign (0x7f / 0xff), subnormals m * 2^-9, largest
// finite value 448 (0x7e).  This is the encoding gfx950 converts in hardware, not the fnuz one
// of gfx942.
//
//   Dec(code): the exact fp32 value of the code; 0x80 is -0; 0x7f / 0xff a NaN (the integer form: a
//              quiet one with the code's sign; of the hardware's only NaN-ness is relied on).
//   Enc(f):    f clamped to [-448, 448] (so +-inf and everything past 448 saturate and the NaN
//              code is never an overflow), then rounded to nearest, ties to even, subnormals
//              produced (the tie at 2^-10 goes to 0).  NaN -> 0x7f | sign, -0 -> 0x80.
//
// The integer forms are the definition (tests/csrc/fp8_cvt_check.cc pins them against torch's
// CPU float8_e4m3fn on tests/fp8_edges.py).  On the device DECODE - the hot direction, one per
// gathered element - is the hardware convert (v_cvt_pk_f32_fp8: two codes of a 32-bit word per
// instruction); ENCODE runs once per table and is the integer form on the device too, so its
// bits do not depend on the convert's saturation mode.  tests/test_fp8_rows_gpu.py pins both
// on the device against the same CPU conversions.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EG_FP8_HD __host__ __device__ __forceinline__
#else
#define EG_FP8_HD inline
#endif

namespace euler_gpu {

constexpr float kFp8Max = 448.0f;

EG_FP8_HD uint32_t Fp8F32Bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
EG_FP8_HD float Fp8BitsF32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// ---- integer forms (the definition; what the host runs) ----------------------------------
EG_FP8_HD float Fp8ToF32Int(uint8_t c) {
  const uint32_t sign = ((uint32_t)c & 0x80u) << 24;
  const uint32_t e = (c >> 3) & 15u;
  uint32_t m = c & 7u;
  if (e == 15u && m == 7u) return Fp8BitsF32(sign | 0x7fc00000u);
  if (e == 0u) {
    if (m == 0u) return Fp8BitsF32(sign);
    int shift = 0;                              // subnormal: m * 2^-9, normalised
    while (!(m & 8u)) { m <<= 1; ++shift; }
    return Fp8BitsF32(sign | ((uint32_t)(121 - shift) << 23) | ((m & 7u) << 20));
  }
  return Fp8BitsF32(sign | ((e + 120u) << 23) | (m << 20));      // exponent bias 7 -> 127
}

EG_FP8_HD uint8_t F32ToFp8Int(float f) {
  const uint32_t u = Fp8F32Bits(f);
  const uint32_t sign = (u >> 24) & 0x80u;
  const uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint8_t)(sign | 0x7fu);           // NaN
  if (a >= 0x43e00000u) return (uint8_t)(sign | 0x7eu);          // >= 448 (inf too): saturates
  if (a >= 0x3c800000u) {                       // >= 2^-6: a normal e4m3
    uint32_t r = a - (120u << 23);
    r += 0x7ffffu + ((r >> 20) & 1u);           // ties to even; a carry steps the exponent
    return (uint8_t)(sign | (r >> 20));         // (at most 0x7e: a < 448)
  }
  if (a <= 0x3a800000u) return (uint8_t)sign;   // <= 2^-10 (the tie with 0 goes to even 0)
  const uint32_t m = (a & 0x7fffffu) | 0x800000u;
  const uint32_t shift = 141u - (a >> 23);      // 21 .. 24: value = m * 2^(e - 150) in units of 2^-9
  uint32_t r = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
  if (rem > half || (rem == half && (r & 1u))) ++r;      // (0x08 = the smallest normal)
  return (uint8_t)(sign | r);
}

// ---- what the kernels call ----------------------------------------------------------------
EG_FP8_HD uint8_t Fp8Enc(float f) { return F32ToFp8Int(f); }

// one code
EG_FP8_HD float Fp8Dec(uint8_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_cvt_pk_f32_fp8((int)(uint32_t)c, false)[0];
#else
  return Fp8ToF32Int(c);
#endif
}

// a 32-bit word holds codes (4 i .. 4 i + 3) little endian, a 16-byte load sixteen codes
EG_FP8_HD void Fp8Dec4(uint32_t w, float f[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo[0]; f[1] = lo[1]; f[2] = hi[0]; f[3] = hi[1];
#else
  for (int i = 0; i < 4; ++i) f[i] = Fp8ToF32Int((uint8_t)(w >> (8 * i)));
#endif
}

EG_FP8_HD void Fp8Dec16(const uint32_t w[4], float f[16]) {
  for (int i = 0; i < 4; ++i) Fp8Dec4(w[i], f + 4 * i);
}

}  // namespace euler_gpu
