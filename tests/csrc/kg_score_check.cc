// Host build of the per-lane arithmetic of the fused triple scoring (euler_amd/csrc/kg_score.h)
// for tests/test_triple_score_host.py: the same lane functions the kernels call, over plain host
// arrays, with the L lanes of a task run one after the other and combined by the butterfly the
// header states.  Built with -ffp-contract=off.
#include <stdint.h>

#include "kg_score.h"

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
struct HostAcc {           // gy of one row, kept in its output row
  float* p;
  void Get(int32_t j, float f[V]) const { for (int k = 0; k < V; ++k) f[k] = p[(int64_t)j * V + k]; }
  void Put(int32_t j, const float f[V]) { for (int k = 0; k < V; ++k) p[(int64_t)j * V + k] = f[k]; }
};

struct Task {
  int32_t kind, lanes, chunks;
  bool normalize;
  // for off = L / 2 .. 1: s = s + s[lane ^ off]; every lane ends with the same bits
  template <typename F>
  float Sum(F lane_part) const {
    float s[64], n[64];
    for (int32_t l = 0; l < lanes; ++l) s[l] = lane_part(l);
    for (int32_t off = lanes >> 1; off > 0; off >>= 1) {
      for (int32_t l = 0; l < lanes; ++l) n[l] = MpwAdd(s[l], s[l ^ off]);
      for (int32_t l = 0; l < lanes; ++l) s[l] = n[l];
    }
    return s[0];
  }
  template <int V>
  void Norm(const HostRow<V>& x, float* ss, float* inv) const {
    *ss = normalize ? Sum([&](int32_t l) { return KgLaneSumSq<V>(x, l, lanes, chunks); }) : 0.f;
    *inv = KgInv(*ss, normalize);
  }
  template <int V>
  float Terms(const HostRow<V>& a, float ia, const HostRow<V>& r, float ir, const HostRow<V>& c, float ic) const {
    return Sum([&](int32_t l) { return KgLaneScore<V>(kind, a, ia, r, ir, c, ic, l, lanes, chunks); });
  }
  template <int V>
  void ScoreGrad(float g, const HostRow<V>& a, float ia, const HostRow<V>& r, float ir, const HostRow<V>& c,
                 float ic, HostAcc<V>& ga, HostAcc<V>& gr, HostAcc<V>& gc) const {
    const float s = kind == kKgTransL2 ? Terms<V>(a, ia, r, ir, c, ic) : 0.f;
    const float gs = KgScale(kind, g, s);
    for (int32_t l = 0; l < lanes; ++l)
      KgLaneScoreGrad<V>(kind, gs, a, ia, r, ir, c, ic, ga, gr, gc, l, lanes, chunks);
  }
  template <int V>
  void RowGrad(const HostRow<V>& x, float ss, float inv, HostAcc<V>& gy) const {
    const float dot = normalize ? Sum([&](int32_t l) { return KgLaneDot<V>(x, inv, gy, l, lanes, chunks); }) : 0.f;
    for (int32_t l = 0; l < lanes; ++l)
      KgLaneRowGrad<V>(x.ok, normalize, x, ss, inv, dot, gy, gy, l, lanes, chunks);
  }
};

struct Args {
  int32_t kind, normalize, corrupt;
  const float* ent; int64_t ent_rows;
  const float* rel; int64_t rel_rows;
  const int64_t* src; const int64_t* rel_id; const int64_t* dst; const int64_t* neg;
  int64_t b, k, d;
};

template <int V>
void Forward(const Args& a, float* pos, float* neg_out) {
  const int32_t chunks = (int32_t)(a.d / V);
  const Task T{a.kind, 1 << KgLogLanes(chunks), chunks, a.normalize != 0};
  const int64_t kp = a.corrupt == kKgBoth ? 2 * a.k : a.k;
  for (int64_t t = 0; t < a.b; ++t) {
    const HostRow<V> h = Open<V>(a.ent, a.src[t], a.ent_rows, a.d), r = Open<V>(a.rel, a.rel_id[t], a.rel_rows, a.d),
                     tl = Open<V>(a.ent, a.dst[t], a.ent_rows, a.d);
    float ss, ih, ir, it, in;
    T.Norm<V>(h, &ss, &ih);
    T.Norm<V>(r, &ss, &ir);
    T.Norm<V>(tl, &ss, &it);
    pos[t] = KgFinish(a.kind, T.Terms<V>(h, ih, r, ir, tl, it));
    for (int64_t k = 0; k < a.k; ++k) {
      const HostRow<V> n = Open<V>(a.ent, a.neg[t * a.k + k], a.ent_rows, a.d);
      T.Norm<V>(n, &ss, &in);
      if (a.corrupt != kKgTail) neg_out[t * kp + k] = KgFinish(a.kind, T.Terms<V>(n, in, r, ir, tl, it));
      if (a.corrupt != kKgFront)
        neg_out[t * kp + (a.corrupt == kKgBoth ? a.k : 0) + k] = KgFinish(a.kind, T.Terms<V>(h, ih, r, ir, n, in));
    }
  }
}

template <int V>
void Backward(const Args& a, const float* g_pos, const float* g_neg, float* g_src, float* g_rel, float* g_dst,
              float* g_neg_rows) {
  const int32_t chunks = (int32_t)(a.d / V);
  const Task T{a.kind, 1 << KgLogLanes(chunks), chunks, a.normalize != 0};
  const int64_t kp = a.corrupt == kKgBoth ? 2 * a.k : a.k;
  for (int64_t t = 0; t < a.b; ++t) {
    const HostRow<V> h = Open<V>(a.ent, a.src[t], a.ent_rows, a.d), r = Open<V>(a.rel, a.rel_id[t], a.rel_rows, a.d),
                     tl = Open<V>(a.ent, a.dst[t], a.ent_rows, a.d);
    float ssh, ssr, sst, ssn, ih, ir, it, in;
    T.Norm<V>(h, &ssh, &ih);
    T.Norm<V>(r, &ssr, &ir);
    T.Norm<V>(tl, &sst, &it);
    HostAcc<V> gh{g_src + t * a.d}, gr{g_rel + t * a.d}, gt{g_dst + t * a.d};
    for (int64_t c = 0; c < a.d; ++c) gh.p[c] = gr.p[c] = gt.p[c] = 0.f;
    T.ScoreGrad<V>(g_pos[t], h, ih, r, ir, tl, it, gh, gr, gt);
    for (int64_t k = 0; k < a.k; ++k) {
      const HostRow<V> n = Open<V>(a.ent, a.neg[t * a.k + k], a.ent_rows, a.d);
      T.Norm<V>(n, &ssn, &in);
      HostAcc<V> gn{g_neg_rows + (t * a.k + k) * a.d};
      for (int64_t c = 0; c < a.d; ++c) gn.p[c] = 0.f;
      if (a.corrupt != kKgTail) T.ScoreGrad<V>(g_neg[t * kp + k], n, in, r, ir, tl, it, gn, gr, gt);
      if (a.corrupt != kKgFront)
        T.ScoreGrad<V>(g_neg[t * kp + (a.corrupt == kKgBoth ? a.k : 0) + k], h, ih, r, ir, n, in, gh, gr, gn);
      T.RowGrad<V>(n, ssn, in, gn);
    }
    T.RowGrad<V>(h, ssh, ih, gh);
    T.RowGrad<V>(r, ssr, ir, gr);
    T.RowGrad<V>(tl, sst, it, gt);
  }
}

}  // namespace

// V of the order for fp32 tables at these addresses (the rule the launcher applies)
extern "C" int kg_chunk_width(int64_t d, const float* ent, const float* rel) {
  return KgChunkWidth(d, (uintptr_t)ent, true, (uintptr_t)rel, true);
}

// The forward (g_pos == nullptr) or the gradient of b triples over fp32 host tables.  v: the
// chunk width to use (1, 4, 8 with d % v == 0), or 0 for kg_chunk_width of the two tables.
extern "C" int kg_triple(int32_t kind, int32_t normalize, int32_t corrupt, int32_t v, const float* ent,
                         int64_t ent_rows, const float* rel, int64_t rel_rows, const int64_t* src,
                         const int64_t* rel_id, const int64_t* dst, const int64_t* neg, int64_t b, int64_t k,
                         int64_t d, float* pos, float* neg_out, const float* g_pos, const float* g_neg,
                         float* g_src, float* g_rel, float* g_dst, float* g_neg_rows) {
  if (kind < 0 || kind > 2 || corrupt < 0 || corrupt > 2 || d < 1) return -1;
  if (v == 0) v = kg_chunk_width(d, ent, rel);
  if ((v != 1 && v != 4 && v != 8) || d % v != 0) return -1;
  const Args a{kind, normalize, corrupt, ent, ent_rows, rel, rel_rows, src, rel_id, dst, neg, b, k, d};
  if (!g_pos) {
    if (v == 8) Forward<8>(a, pos, neg_out);
    else if (v == 4) Forward<4>(a, pos, neg_out);
    else Forward<1>(a, pos, neg_out);
  } else {
    if (v == 8) Backward<8>(a, g_pos, g_neg, g_src, g_rel, g_dst, g_neg_rows);
    else if (v == 4) Backward<4>(a, g_pos, g_neg, g_src, g_rel, g_dst, g_neg_rows);
    else Backward<1>(a, g_pos, g_neg, g_src, g_rel, g_dst, g_neg_rows);
  }
  return 0;
}
