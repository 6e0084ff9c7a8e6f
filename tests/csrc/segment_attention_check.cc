// Host build of the fused attention arithmetic (euler_amd/csrc/mp_attention.h and, through it,
// mp_softmax.h) for tests/test_segment_attention_host.py: the same pieces the kernels call, with the
// lanes of a wave or block emulated by arrays.  Built with -ffp-contract=off.  fp32 tables, int64
// gather rows (clamped to the last row, as the kernels do), destinations by seg_ptr.
// With -DSEGMENT_ATTENTION_CHECK_MAIN the file is a program of its own (for a sanitizer build):
// it runs the lengths, head counts and widths of the host test on pseudo-random data.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "mp_attention.h"

using namespace euler_gpu;

namespace {

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

// DOT of mp_attention.h over the dh columns a[0 .. dh), b[0 .. dh): L emulated partials, a butterfly
float Dot(const float* a, const float* b, int64_t dh) {
  const int32_t v = AttChunk(dh), lanes = AttLanes(dh);
  const int64_t chunks = dh / v;
  std::vector<float> s(lanes, 0.f);
  for (int32_t l = 0; l < lanes; ++l)
    for (int64_t j = l; j < chunks; j += lanes)
      s[l] = v == 4 ? AttChunkDot<4>(a + j * 4, b + j * 4, s[l]) : AttChunkDot<1>(a + j, b + j, s[l]);
  for (int32_t off = lanes / 2; off >= 1; off /= 2) {
    std::vector<float> next(lanes);
    for (int32_t l = 0; l < lanes; ++l) next[l] = MpwAdd(s[l], s[l ^ off]);
    s = next;
  }
  return s[0];
}

// the softmax (g == nullptr) or its gradient on y = x of one segment, head h of heads, in place
// positions b .. b + n of the [*, heads] arrays
void Softmax(const float* x, const float* g, int64_t b, int64_t n, int32_t h, int32_t heads, float* out) {
  const auto lx = [&](int64_t p) { return x[(b + p) * heads + h]; };
  const auto lg = [&](int64_t p) { return g[(b + p) * heads + h]; };
  if (n == 0) return;
  if (n <= kSmxShort) {
    float a[kSmxShort], c[kSmxShort], o[kSmxShort];
    for (int64_t p = 0; p < n; ++p) { a[p] = lx(p); c[p] = g ? lg(p) : 0.f; }
    if (g) SmxShortBackward<kSmxShort>(a, c, (int32_t)n, o);
    else SmxShortForward<kSmxShort>(a, (int32_t)n, o);
    for (int64_t p = 0; p < n; ++p) out[(b + p) * heads + h] = o[p];
    return;
  }
  const int64_t w = kSmxBlock / SmxHeadsPerWave(heads);
  std::vector<float> part(w);
  const auto add = [](float a, float c) { return MpwAdd(a, c); };
  if (g) {
    for (int64_t l = 0; l < w; ++l) part[l] = SmxLaneDotSum(lx, lg, l, w, n);
    const float t = Combine(part, w, false, add);
    for (int64_t p = 0; p < n; ++p) out[(b + p) * heads + h] = SmxBackwardValue(lx(p), lg(p), t);
    return;
  }
  for (int64_t l = 0; l < w; ++l) part[l] = SmxLaneMax(lx, l, w, n);
  const float m = Combine(part, w, true, [](float a, float c) { return SmxMax(a, c); });
  for (int64_t l = 0; l < w; ++l) part[l] = SmxLaneExpSum(lx, m, l, w, n);
  const float s = Combine(part, w, false, add);
  for (int64_t p = 0; p < n; ++p) out[(b + p) * heads + h] = SmxForwardValue(lx(p), m, s);
}

int64_t Row(const int64_t* gi, int64_t p, int64_t rows) {
  const uint32_t g = (uint32_t)gi[p];
  return g < (uint32_t)(rows - 1) ? g : rows - 1;
}

}  // namespace

extern "C" {

// the lane layout of DOT for a head of dh columns, as the kernels and Dot() above take it
int32_t att_chunk(int64_t dh) { return AttChunk(dh); }
int32_t att_lanes(int64_t dh) { return AttLanes(dh); }

// kind 0 dot (q, k [*, d]), 1 additive (q, k [*, heads]; q may be null); v null: v is k.
// Writes logits and alpha [e, heads] (0 outside the span of seg_ptr) and out [size, dv].
int att_forward(int32_t kind, const float* q, int64_t q_rows, const int32_t* q_index, const float* k,
                int64_t k_rows, const float* v, int64_t v_rows, const int64_t* gi, const int64_t* seg_ptr,
                int32_t size, int64_t e, int64_t d, int64_t dv, int32_t heads, float scale, float slope,
                float* logits, float* alpha, float* out) {
  if (heads < 1 || d % heads || dv % heads) return -1;
  if (!v) { v = k; v_rows = k_rows; }
  const int64_t dh = d / heads, dvh = dv / heads;
  for (int64_t i = 0; i < e * heads; ++i) logits[i] = alpha[i] = 0.f;
  for (int32_t r = 0; r < size; ++r) {
    const int64_t b = seg_ptr[r], n = seg_ptr[r + 1] - b;
    int64_t qr = q_index ? q_index[r] : r;
    if (q && qr > q_rows - 1) qr = q_rows - 1;
    for (int64_t p = b; p < b + n; ++p)
      for (int32_t h = 0; h < heads; ++h) {
        const int64_t g = Row(gi, p, k_rows);
        logits[p * heads + h] = kind == kAttDot
            ? AttDotLogit(Dot(q + qr * d + h * dh, k + g * d + h * dh, dh), scale)
            : AttAdditiveLogit(q ? q[qr * heads + h] : 0.f, k[g * heads + h], slope);
      }
    for (int32_t h = 0; h < heads; ++h) Softmax(logits, nullptr, b, n, h, heads, alpha);
    for (int64_t c = 0; c < dv; ++c) {
      float acc = 0.f;
      for (int64_t p = b; p < b + n; ++p)
        acc = AttFold(acc, v[Row(gi, p, v_rows) * dv + c], alpha[p * heads + c / dvh]);
      out[r * dv + c] = acc;
    }
  }
  return 0;
}

// the destination side of the backward: ds [e, heads], dq_dst [size, d]
int att_backward(int32_t kind, const float* q, int64_t q_rows, const int32_t* q_index, const float* k,
                 int64_t k_rows, const float* v, int64_t v_rows, const int64_t* gi, const int64_t* seg_ptr,
                 int32_t size, int64_t e, int64_t d, int64_t dv, int32_t heads, float scale, float slope,
                 const float* alpha, const float* grad, float* ds, float* dq_dst) {
  if (heads < 1 || d % heads || dv % heads) return -1;
  if (!v) { v = k; v_rows = k_rows; }
  const int64_t dh = d / heads, dvh = dv / heads;
  std::vector<float> da((size_t)(e * heads), 0.f);
  for (int64_t i = 0; i < e * heads; ++i) ds[i] = 0.f;
  for (int32_t r = 0; r < size; ++r) {
    const int64_t b = seg_ptr[r], n = seg_ptr[r + 1] - b;
    int64_t qr = q_index ? q_index[r] : r;
    if (q && qr > q_rows - 1) qr = q_rows - 1;
    for (int64_t p = b; p < b + n; ++p)
      for (int32_t h = 0; h < heads; ++h)
        da[p * heads + h] = Dot(grad + (int64_t)r * dv + h * dvh, v + Row(gi, p, v_rows) * dv + h * dvh, dvh);
    for (int32_t h = 0; h < heads; ++h) Softmax(alpha, da.data(), b, n, h, heads, ds);
    for (int64_t p = b; p < b + n; ++p)
      for (int32_t h = 0; h < heads; ++h) {
        float& x = ds[p * heads + h];
        x = kind == kAttDot ? MpwMul(scale, x)
                            : AttAdditiveGrad(x, q ? q[qr * heads + h] : 0.f, k[Row(gi, p, k_rows) * heads + h], slope);
      }
    for (int64_t c = 0; c < d; ++c) {
      float acc = 0.f;
      for (int64_t p = b; p < b + n; ++p)
        acc = kind == kAttDot ? AttFold(acc, k[Row(gi, p, k_rows) * d + c], ds[p * heads + c / dh])
                              : MpwAdd(acc, ds[p * heads + c]);
      dq_dst[r * d + c] = acc;
    }
  }
  return 0;
}

}  // extern "C"

#ifdef SEGMENT_ATTENTION_CHECK_MAIN
namespace {
uint32_t state = 12345u;
float Rand() {           // uniform in [-1, 1)
  state = state * 1664525u + 1013904223u;
  return (float)(state >> 8) / 8388608.0f - 1.0f;
}
}  // namespace

int main() {
  const int64_t lens[] = {0, 1, 7, 16, 17, 32, 33, 300};
  const int32_t heads_of[] = {1, 3, 4, 8};
  const int64_t widths[] = {1, 4, 5, 32};
  int runs = 0;
  for (int32_t heads : heads_of)
    for (int64_t dh : widths)
      for (int32_t kind = 0; kind < 2; ++kind)
        for (int shared = 0; shared < 2; ++shared) {
          if (kind == 1 && shared) continue;
          const int32_t size = 8;
          const int64_t rows = 37, d = kind ? heads : heads * dh, dv = shared ? d : heads * dh;
          std::vector<int64_t> sp(size + 1, 0);
          for (int r = 0; r < size; ++r) sp[r + 1] = sp[r] + lens[r];
          const int64_t e = sp[size];
          std::vector<float> q((size_t)(size * d)), k((size_t)(rows * d)), v((size_t)(rows * dv)), g((size_t)(size * dv));
          for (auto& x : q) x = Rand();
          for (auto& x : k) x = Rand();
          for (auto& x : v) x = Rand();
          for (auto& x : g) x = Rand();
          std::vector<int64_t> gi((size_t)e);
          for (auto& x : gi) { state = state * 1664525u + 1013904223u; x = (state >> 8) % (rows + 2); }
          std::vector<int32_t> qi(size);
          for (int r = 0; r < size; ++r) qi[r] = r / 2;
          std::vector<float> lg((size_t)(e * heads)), al(lg.size()), ds(lg.size()), out((size_t)(size * dv)), dq((size_t)(size * d));
          const float* vp = shared ? nullptr : v.data();
          if (att_forward(kind, q.data(), size, qi.data(), k.data(), rows, vp, rows, gi.data(), sp.data(), size, e, d,
                          dv, heads, 0.3f, 0.2f, lg.data(), al.data(), out.data()) != 0) return 1;
          if (att_backward(kind, q.data(), size, qi.data(), k.data(), rows, vp, rows, gi.data(), sp.data(), size, e,
                           d, dv, heads, 0.3f, 0.2f, al.data(), g.data(), ds.data(), dq.data()) != 0) return 1;
          for (int r = 0; r < size; ++r)
            for (int32_t h = 0; h < heads; ++h) {
              double s = 0;
              for (int64_t p = sp[r]; p < sp[r + 1]; ++p) s += al[p * heads + h];
              if (lens[r] > 0 && (s < 0.999 || s > 1.001)) { printf("alpha does not sum to 1\n"); return 2; }
            }
          ++runs;
        }
  printf("segment_attention_check: %d runs ok\n", runs);
  return 0;
}
#endif
