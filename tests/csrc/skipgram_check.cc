// Host build of the per-lane arithmetic of the fused skip-gram loss head
// (euler_amd/csrc/skipgram.h) for tests/test_skipgram_host.py: the same lane functions the
// kernels call, over plain host arrays, with the L lanes of a pair row run one after the other
// and combined by the butterfly the header states, and the 256 partials of the total by its
// tree.  Also the error of Log1pUnit and of the softplus against libm's float64.  Built with
// -ffp-contract=off.
#include <math.h>
#include <stdint.h>

#include "skipgram.h"

using namespace euler_gpu;

namespace {

template <int V>
struct HostRow {
  const float* p;          // the row's first column, or nullptr for a row the range rule removed
  bool ok;
  void Chunk(int32_t j, float f[V]) const {
    for (int k = 0; k < V; ++k) f[k] = ok ? p[(int64_t)j * V + k] : 0.f;
  }
};

template <int V>
HostRow<V> Open(const float* table, int64_t id, int64_t rows, int64_t d) {
  const bool ok = KgInRange(id, rows);
  return HostRow<V>{ok ? table + id * d : nullptr, ok};
}

template <int V>
struct HostOut {           // a lane's columns of an output row
  float* p;
  void Get(int32_t j, float f[V]) const { for (int k = 0; k < V; ++k) f[k] = p[(int64_t)j * V + k]; }
  void Put(int32_t j, const float f[V]) { for (int k = 0; k < V; ++k) p[(int64_t)j * V + k] = f[k]; }
};

// for off = L / 2 .. 1: s = s + s[lane ^ off]; every lane ends with the same bits
template <typename F>
float Sum(int32_t lanes, F lane_part) {
  float s[64], n[64];
  for (int32_t l = 0; l < lanes; ++l) s[l] = lane_part(l);
  for (int32_t off = lanes >> 1; off > 0; off >>= 1) {
    for (int32_t l = 0; l < lanes; ++l) n[l] = MpwAdd(s[l], s[l ^ off]);
    for (int32_t l = 0; l < lanes; ++l) s[l] = n[l];
  }
  return s[0];
}

struct Args {
  const float* target; int64_t target_rows;
  const float* context; int64_t context_rows;
  const int64_t* src; const int64_t* pos; const int64_t* neg;
  int64_t b, p, k, d;
  int64_t ContextId(int64_t t, int64_t j) const { return j < p ? pos[t * p + j] : neg[t * k + (j - p)]; }
};

// the total of the header: 256 partials, a butterfly inside each run of 64, (S0 + S1) + (S2 + S3)
float Total(const float* row_loss, int64_t b) {
  float run[kSgPartials / 64];
  for (int32_t r = 0; r < kSgPartials / 64; ++r)
    run[r] = Sum(64, [&](int32_t l) { return SgLanePartial(row_loss, r * 64 + l, b); });
  return SmxCombine4(run[0], run[1], run[2], run[3]);
}

template <int V>
void Forward(const Args& a, float* logits, int32_t* rank, float* row_loss, float* loss) {
  const int32_t chunks = (int32_t)(a.d / V), lanes = 1 << KgLogLanes(chunks);
  const int64_t n = a.p + a.k;
  for (int64_t t = 0; t < a.b; ++t) {
    const HostRow<V> tr = Open<V>(a.target, a.src[t], a.target_rows, a.d);
    auto dot = [&](int64_t j) {
      const HostRow<V> c = Open<V>(a.context, a.ContextId(t, j), a.context_rows, a.d);
      return Sum(lanes, [&](int32_t l) { return SgLaneDot<V>(tr, c, l, lanes, chunks); });
    };
    const float x_last = dot(a.p - 1);
    SgRowState st;
    st.Start(a.p, x_last);
    for (int64_t j = 0; j < n; ++j) {
      const float x = j == a.p - 1 ? x_last : dot(j);
      st.Add(x);
      logits[t * n + j] = x;
    }
    rank[t] = st.rank;
    row_loss[t] = st.sum;
  }
  *loss = SgFinish(Total(row_loss, a.b), a.b, a.p, a.k);
}

template <int V>
void Backward(const Args& a, const float* logits, float g, float* g_src, float* g_pos, float* g_neg) {
  const int32_t chunks = (int32_t)(a.d / V), lanes = 1 << KgLogLanes(chunks);
  const int64_t n = a.p + a.k;
  const float gs = MpwDiv(g, SgCount(a.b, a.p, a.k));
  for (int64_t t = 0; t < a.b; ++t) {
    const HostRow<V> tr = Open<V>(a.target, a.src[t], a.target_rows, a.d);
    HostOut<V> acc{g_src + t * a.d};
    for (int64_t c = 0; c < a.d; ++c) acc.p[c] = 0.f;
    for (int64_t j = 0; j < n; ++j) {
      const HostRow<V> c = Open<V>(a.context, a.ContextId(t, j), a.context_rows, a.d);
      const float cj = SgCoef(gs, logits[t * n + j], j < a.p);
      HostOut<V> oc{j < a.p ? g_pos + (t * a.p + j) * a.d : g_neg + (t * a.k + (j - a.p)) * a.d};
      for (int32_t l = 0; l < lanes; ++l) SgLaneGrad<V>(cj, c.ok, tr, c, acc, oc, l, lanes, chunks);
    }
    for (int32_t l = 0; l < lanes; ++l) SgLaneSrcGrad<V>(tr.ok, acc, acc, l, lanes, chunks);
  }
}

// |got - exact| in ulps of the exact value (2^-149, the spacing of the denormals, below 2^-126)
double UlpError(float got, double exact) {
  int ex;
  frexp(exact, &ex);                                  // exact = f * 2^ex, f in [0.5, 1)
  return fabs((double)got - exact) / ldexp(1.0, ex - 1 - 23 < -149 ? -149 : ex - 1 - 23);
}

}  // namespace

extern "C" {

// V of the order for fp32 tables at these addresses (the rule the launcher applies)
int sg_chunk_width(int64_t d, const float* target, const float* context) {
  return KgChunkWidth(d, (uintptr_t)target, true, (uintptr_t)context, true);
}

void sg_log1p(const float* e, int64_t n, float* out) { for (int64_t i = 0; i < n; ++i) out[i] = Log1pUnit(e[i]); }
void sg_term(const float* x, int64_t n, int32_t positive, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = SgTerm(x[i], positive != 0);
}
void sg_sigmoid(const float* x, int64_t n, float* out) { for (int64_t i = 0; i < n; ++i) out[i] = SgSigmoid(x[i]); }
void sg_coef(float gs, const float* x, int64_t n, int32_t positive, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = SgCoef(gs, x[i], positive != 0);
}
float sg_total(const float* row_loss, int64_t b, int64_t p, int64_t k) { return SgFinish(Total(row_loss, b), b, p, k); }

// the largest error of Log1pUnit over the floats e > 0 with bit patterns lo, lo + stride, ... <= hi
// (hi <= the pattern of 1.0f), in ulps of the exact value; *worst = the pattern where it occurs
double sg_log1p_error(uint32_t lo, uint32_t hi, uint32_t stride, uint32_t* worst) {
  double big = 0;
  for (uint64_t b = lo; b <= hi; b += stride) {
    const float e = BitsF32((uint32_t)b);
    if (!(e > 0.f)) continue;
    const double err = UlpError(Log1pUnit(e), log1p((double)e));
    if (err > big) { big = err; *worst = (uint32_t)b; }
  }
  return big;
}

// the largest error of the softplus of a logit x <= 0, max(x, 0) + Log1pUnit(ExpNonPositive(-|x|)),
// against log1p(exp(x)), over the negative floats with bit patterns lo, lo + stride, ... <= hi.
// Where x >= kSmxExpFloor: in ulps of the exact value (the return value, *worst its pattern);
// below it the result is +0 and *abs_below takes the largest exact value met there.
double sg_softplus_error(uint32_t lo, uint32_t hi, uint32_t stride, uint32_t* worst, double* abs_below) {
  double big = 0;
  for (uint64_t b = lo; b <= hi; b += stride) {
    const float x = BitsF32((uint32_t)b);
    if (!(x <= 0.f)) continue;
    const double exact = log1p(exp((double)x));
    const float got = SgTerm(x, false);
    if (x >= kSmxExpFloor) {
      const double err = UlpError(got, exact);
      if (err > big) { big = err; *worst = (uint32_t)b; }
    } else {
      if (got != 0.f) return -1.0;
      if (exact > *abs_below) *abs_below = exact;
    }
  }
  return big;
}

// The forward (logits_in == nullptr) or the gradient of b pair rows over fp32 host tables.  v: the
// chunk width to use (1, 4, 8 with d % v == 0), or 0 for sg_chunk_width of the two tables.
int sg_pairs(int32_t v, const float* target, int64_t target_rows, const float* context, int64_t context_rows,
             const int64_t* src, const int64_t* pos, const int64_t* neg, int64_t b, int64_t p, int64_t k, int64_t d,
             float* logits, int32_t* rank, float* row_loss, float* loss, const float* logits_in, float g,
             float* g_src, float* g_pos, float* g_neg) {
  if (d < 1 || p < 1 || k < 0 || b < 0) return -1;
  if (v == 0) v = sg_chunk_width(d, target, context);
  if ((v != 1 && v != 4 && v != 8) || d % v != 0) return -1;
  const Args a{target, target_rows, context, context_rows, src, pos, neg, b, p, k, d};
  if (!logits_in) {
    if (v == 8) Forward<8>(a, logits, rank, row_loss, loss);
    else if (v == 4) Forward<4>(a, logits, rank, row_loss, loss);
    else Forward<1>(a, logits, rank, row_loss, loss);
  } else {
    if (v == 8) Backward<8>(a, logits_in, g, g_src, g_pos, g_neg);
    else if (v == 4) Backward<4>(a, logits_in, g, g_src, g_pos, g_neg);
    else Backward<1>(a, logits_in, g, g_src, g_pos, g_neg);
  }
  return 0;
}

}  // extern "C"
