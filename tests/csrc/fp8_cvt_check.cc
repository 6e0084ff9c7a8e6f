// TEST INFRASTRUCTURE (not product code): the host forms of euler_amd/csrc/fp8_cvt.h over arrays,
// so that `pytest -m "not gpu"` (tests/test_fp8_cvt_host.py) can pin them against torch's CPU
// float8_e4m3fn conversions.  The scalar entry points run the integer definitions, the packed one
// the 16-code form the kernels use.  Compiled on demand by the test.
#include <stdint.h>

#include "fp8_cvt.h"

using namespace euler_gpu;

extern "C" {

void f8_dec(const uint8_t* in, int64_t n, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = Fp8Dec(in[i]);
}

// n % 16 == 0
void f8_dec16(const uint8_t* in, int64_t n, float* out) {
  for (int64_t i = 0; i < n; i += 16) {
    uint32_t w[4];
    for (int k = 0; k < 4; ++k)
      w[k] = (uint32_t)in[i + 4 * k] | ((uint32_t)in[i + 4 * k + 1] << 8) |
             ((uint32_t)in[i + 4 * k + 2] << 16) | ((uint32_t)in[i + 4 * k + 3] << 24);
    Fp8Dec16(w, out + i);
  }
}

void f8_enc(const float* in, int64_t n, uint8_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = Fp8Enc(in[i]);
}

}  // extern "C"
