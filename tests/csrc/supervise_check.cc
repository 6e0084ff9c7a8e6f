// Host build of the per-element arithmetic of the fused supervised loss head
// (euler_amd/csrc/supervise.h) for tests/test_supervise_host.py: the same functions the kernels
// call, over plain host arrays - the element, the row sum in the order c = 0 .. C - 1, the 256
// partials of the total by skip-gram's tree, the counts, the two histograms and the gradient.
// Built with -ffp-contract=off.
#include <stdint.h>

#include "supervise.h"

using namespace euler_gpu;

namespace {

// for off = 32 .. 1: s = s + s[lane ^ off]
float Run64(const float* row_loss, int32_t run, int64_t b) {
  float s[64], n[64];
  for (int32_t l = 0; l < 64; ++l) s[l] = SgLanePartial(row_loss, run * 64 + l, b);
  for (int32_t off = 32; off > 0; off >>= 1) {
    for (int32_t l = 0; l < 64; ++l) n[l] = MpwAdd(s[l], s[l ^ off]);
    for (int32_t l = 0; l < 64; ++l) s[l] = n[l];
  }
  return s[0];
}

}  // namespace

extern "C" {

void sv_term(const float* x, const float* z, int64_t n, int32_t general, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = general ? SvTermGeneral(x[i], z[i]) : SvTerm(x[i], z[i]);
}
void sv_sg_term(const float* x, int64_t n, int32_t positive, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = SgTerm(x[i], positive != 0);
}
void sv_sigmoid(const float* x, int64_t n, float* out) { for (int64_t i = 0; i < n; ++i) out[i] = SgSigmoid(x[i]); }
void sv_predict(const float* p, int64_t n, int32_t* out) { for (int64_t i = 0; i < n; ++i) out[i] = SvPredict(p[i]); }
void sv_thresholds(int32_t t, float* out) { for (int32_t i = 0; i < t; ++i) out[i] = SvThreshold(i, t); }
void sv_bucket(const float* p, int64_t n, int32_t t, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = SvBucket(p[i], t);
}

// the whole forward over fp32 host arrays; prob, diff and hist may be null; counts and hist are added to
void sv_forward(const float* x, const float* z, int64_t b, int64_t c, int32_t t, float* prob, float* diff,
                float* row_loss, float* loss, int64_t* counts, int64_t* hist) {
  for (int64_t r = 0; r < b; ++r) {
    float sum = 0.f;
    for (int64_t j = 0; j < c; ++j) {
      const SvElem e = SvElement(x[r * c + j], z[r * c + j]);
      sum = SvRowAdd(sum, e.term, j == 0);
      if (prob) prob[r * c + j] = e.p;
      if (diff) diff[r * c + j] = e.diff;
      counts[0] += e.label && e.pred;
      counts[1] += !e.label && e.pred;
      counts[2] += e.label && !e.pred;
      counts[3] += e.correct;
      if (hist) hist[(e.label ? 0 : t + 1) + SvBucket(e.p, t)] += 1;
    }
    row_loss[r] = sum;
  }
  counts[4] += b * c;
  *loss = SgFinish(SmxCombine4(Run64(row_loss, 0, b), Run64(row_loss, 1, b), Run64(row_loss, 2, b),
                               Run64(row_loss, 3, b)), b, c, 0);
}

void sv_grad(const float* diff, float g, int64_t b, int64_t c, float* out) {
  const float gs = SvScale(g, b, c);
  for (int64_t i = 0; i < b * c; ++i) out[i] = SvGrad(gs, diff[i]);
}

}  // extern "C"
