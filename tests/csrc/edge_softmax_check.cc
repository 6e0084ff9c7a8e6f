// Host build of the softmax arithmetic (euler_amd/csrc/mp_softmax.h) for
// tests/test_edge_softmax_host.py: the same pieces the kernels call, with the lanes of a block
// emulated by arrays.  Built with -ffp-contract=off.  The float64 exp of <math.h> is used ONLY
// as the yardstick of smx_exp_error.
#include <math.h>
#include <stdint.h>

#include <vector>

#include "mp_softmax.h"

using namespace euler_gpu;

namespace {

// the combine tree of the header over w emulated partials: 4 runs, a butterfly inside each
// (every lane computes s_l + s_(l ^ off), as the shuffles do), then SmxCombine4
template <typename Op>
float Combine(std::vector<float> s, int64_t w, bool is_max, Op op) {
  const int64_t run = w / 4;
  for (int64_t off = run / 2; off >= 1; off /= 2) {
    std::vector<float> next(s.size());
    for (int64_t l = 0; l < w; ++l) next[l] = op(s[l], s[(l / run) * run + ((l % run) ^ off)]);
    s = next;
  }
  if (is_max) return SmxMax(SmxMax(s[0], s[run]), SmxMax(s[2 * run], s[3 * run]));
  return SmxCombine4(s[0], s[run], s[2 * run], s[3 * run]);
}

}  // namespace

extern "C" {

float smx_floor() { return kSmxExpFloor; }

void smx_exp(const float* d, int64_t n, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = ExpNonPositive(d[i]);
}

// the largest error of ExpNonPositive over the negative floats with bit patterns lo, lo + stride,
// ... <= hi, in ulps of the exact value; *worst = the bit pattern where it occurs
double smx_exp_error(uint32_t lo, uint32_t hi, uint32_t stride, uint32_t* worst) {
  double big = 0;
  for (uint64_t b = lo; b <= hi; b += stride) {
    const float d = BitsF32((uint32_t)b);
    const double exact = exp((double)d);
    int ex;
    frexp(exact, &ex);                                  // exact = f * 2^ex, f in [0.5, 1)
    const double err = fabs((double)ExpNonPositive(d) - exact) / ldexp(1.0, ex - 1 - 23);
    if (err > big) { big = err; *worst = (uint32_t)b; }
  }
  return big;
}

// one segment: x [n, heads] -> y, in the order of the header (n <= kSmxShort: one lane a head)
int smx_forward(const float* x, int64_t n, int32_t heads, float* y) {
  if (heads < 1 || n < 0) return -1;
  for (int32_t h = 0; h < heads; ++h) {
    const auto ld = [&](int64_t p) { return x[p * heads + h]; };
    if (n == 0) continue;
    if (n <= kSmxShort) {
      float a[kSmxShort], o[kSmxShort];
      for (int64_t p = 0; p < n; ++p) a[p] = ld(p);
      SmxShortForward<kSmxShort>(a, (int32_t)n, o);
      for (int64_t p = 0; p < n; ++p) y[p * heads + h] = o[p];
      continue;
    }
    const int64_t w = kSmxBlock / SmxHeadsPerWave(heads);
    std::vector<float> part(w);
    for (int64_t l = 0; l < w; ++l) part[l] = SmxLaneMax(ld, l, w, n);
    const float m = Combine(part, w, true, [](float a, float b) { return SmxMax(a, b); });
    for (int64_t l = 0; l < w; ++l) part[l] = SmxLaneExpSum(ld, m, l, w, n);
    const float s = Combine(part, w, false, [](float a, float b) { return MpwAdd(a, b); });
    for (int64_t p = 0; p < n; ++p) y[p * heads + h] = SmxForwardValue(ld(p), m, s);
  }
  return 0;
}

int smx_backward(const float* y, const float* g, int64_t n, int32_t heads, float* gx) {
  if (heads < 1 || n < 0) return -1;
  for (int32_t h = 0; h < heads; ++h) {
    const auto ly = [&](int64_t p) { return y[p * heads + h]; };
    const auto lg = [&](int64_t p) { return g[p * heads + h]; };
    if (n == 0) continue;
    if (n <= kSmxShort) {
      float a[kSmxShort], b[kSmxShort], o[kSmxShort];
      for (int64_t p = 0; p < n; ++p) { a[p] = ly(p); b[p] = lg(p); }
      SmxShortBackward<kSmxShort>(a, b, (int32_t)n, o);
      for (int64_t p = 0; p < n; ++p) gx[p * heads + h] = o[p];
      continue;
    }
    const int64_t w = kSmxBlock / SmxHeadsPerWave(heads);
    std::vector<float> part(w);
    for (int64_t l = 0; l < w; ++l) part[l] = SmxLaneDotSum(ly, lg, l, w, n);
    const float t = Combine(part, w, false, [](float a, float b) { return MpwAdd(a, b); });
    for (int64_t p = 0; p < n; ++p) gx[p * heads + h] = SmxBackwardValue(ly(p), lg(p), t);
  }
  return 0;
}

}  // extern "C"
