// TEST INFRASTRUCTURE (not product code): the host forms of euler_amd/csrc/half_cvt.h over
// arrays, so that `pytest -m "not gpu"` (tests/test_half_cvt_host.py) can pin them against
// torch's CPU conversions.  The scalar entry points run the integer definitions, the packed
// ones the 2- and 8-element forms the kernels use.  Compiled on demand by the test.
#include <stdint.h>

#include "half_cvt.h"

using namespace euler_gpu;

extern "C" {

// dt: 1 = bf16, 2 = fp16
void hcv_widen(int dt, const uint16_t* in, int64_t n, float* out) {
  for (int64_t i = 0; i < n; ++i)
    out[i] = dt == kBF16 ? HalfCvt<kBF16>::Widen(in[i]) : HalfCvt<kF16>::Widen(in[i]);
}

void hcv_narrow(int dt, const float* in, int64_t n, uint16_t* out) {
  for (int64_t i = 0; i < n; ++i)
    out[i] = dt == kBF16 ? HalfCvt<kBF16>::Narrow(in[i]) : HalfCvt<kF16>::Narrow(in[i]);
}

// n % 8 == 0
void hcv_widen8(int dt, const uint16_t* in, int64_t n, float* out) {
  for (int64_t i = 0; i < n; i += 8) {
    uint32_t w[4];
    for (int k = 0; k < 4; ++k) w[k] = (uint32_t)in[i + 2 * k] | ((uint32_t)in[i + 2 * k + 1] << 16);
    if (dt == kBF16) Widen8<kBF16>(w, out + i); else Widen8<kF16>(w, out + i);
  }
}

void hcv_narrow8(int dt, const float* in, int64_t n, uint16_t* out) {
  for (int64_t i = 0; i < n; i += 8) {
    uint32_t w[4];
    if (dt == kBF16) Narrow8<kBF16>(in + i, w); else Narrow8<kF16>(in + i, w);
    for (int k = 0; k < 4; ++k) {
      out[i + 2 * k] = (uint16_t)(w[k] & 0xffffu);
      out[i + 2 * k + 1] = (uint16_t)(w[k] >> 16);
    }
  }
}

}  // extern "C"
