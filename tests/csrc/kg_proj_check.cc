// Host build of the per-lane arithmetic of triple scoring with the TransH / TransD projections
// (euler_amd/csrc/kg_proj.h) for tests/test_triple_score_proj_host.py: the same lane functions
// the kernels call, over plain host arrays, with the L lanes of a task run one after the other
// and combined by the butterfly kg_score.h states.  Built with -ffp-contract=off.
#include <stdint.h>

#include "kg_proj.h"

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

struct Args {
  int32_t proj, kind, corrupt;
  const float* ent; const float* ent_aux; int64_t ent_rows;
  const float* rel; const float* rel_aux; int64_t rel_rows;
  const int64_t* src; const int64_t* rel_id; const int64_t* dst; const int64_t* neg;
  int64_t b, k, d;
};

template <int V>
struct Task {
  using View = KgProjRow<V, HostRow<V>, HostRow<V>>;
  const Args& a;
  int32_t lanes, chunks;
  HostRow<V> r, w;         // rel[rel_id]; hyper[rel_id] or rel_transfer[rel_id]
  float ssr, ir, ssw, iw;

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
  template <typename Row>
  void Norm(const Row& x, float* ss, float* inv) const {
    *ss = Sum([&](int32_t l) { return KgLaneSumSq<V>(x, l, lanes, chunks); });
    *inv = KgInv(*ss, true);
  }
  Task(const Args& args, int64_t t) : a(args) {
    chunks = (int32_t)(a.d / V);
    lanes = 1 << KgLogLanes(chunks);
    r = Open<V>(a.rel, a.rel_id[t], a.rel_rows, a.d);
    w = Open<V>(a.rel_aux, a.rel_id[t], a.rel_rows, a.d);
    Norm(r, &ssr, &ir);
    ssw = 0.f;
    iw = 1.f;
    if (a.proj == kKgProjHyper) Norm(w, &ssw, &iw);
  }

  struct Ent {             // an entity row and what its projection gives
    HostRow<V> x, a;
    float p, ss, inv;
  };
  Ent Project(int64_t id) const {
    Ent e;
    e.x = Open<V>(a.ent, id, a.ent_rows, a.d);
    e.a = HostRow<V>{nullptr, false};
    if (a.proj == kKgProjHyper) {
      e.p = Sum([&](int32_t l) { return KgLaneProjDot<V>(e.x, w, iw, l, lanes, chunks); });
      e.ss = 0.f;
      e.inv = 1.f;
    } else {
      e.a = Open<V>(a.ent_aux, id, a.ent_rows, a.d);
      e.p = Sum([&](int32_t l) { return KgLaneProjDot<V>(e.x, e.a, 1.f, l, lanes, chunks); });
      const View z{e.x, w, 1.f, e.p, false};
      Norm(z, &e.ss, &e.inv);
    }
    return e;
  }
  View Projected(const Ent& e) const { return View{e.x, w, iw, e.p, a.proj == kKgProjHyper}; }

  float Terms(const Ent& x, const Ent& c) const {
    const View xv = Projected(x), cv = Projected(c);
    return Sum([&](int32_t l) { return KgLaneScore<V>(a.kind, xv, x.inv, r, ir, cv, c.inv, l, lanes, chunks); });
  }
  void ScoreGrad(float g, const Ent& x, const Ent& c, HostAcc<V>& gx, HostAcc<V>& gr, HostAcc<V>& gc) const {
    const float s = a.kind == kKgTransL2 ? Terms(x, c) : 0.f;
    const float gs = KgScale(a.kind, g, s);
    const View xv = Projected(x), cv = Projected(c);
    for (int32_t l = 0; l < lanes; ++l)
      KgLaneScoreGrad<V>(a.kind, gs, xv, x.inv, r, ir, cv, c.inv, gx, gr, gc, l, lanes, chunks);
  }
  // an entity row with gy complete (in its output row) goes through its projection
  void Through(const Ent& e, HostAcc<V>& gy, float* out_aux, HostAcc<V>& gaux) const {
    if (a.proj == kKgProjHyper) {
      const KgAccRow<V, HostAcc<V>> gr{gy};
      const float q = Sum([&](int32_t l) { return KgLaneProjDot<V>(gr, w, iw, l, lanes, chunks); });
      for (int32_t l = 0; l < lanes; ++l) KgLaneHyperGrad<V>(e.x.ok, e.x, w, iw, e.p, q, gy, gy, gaux, l, lanes, chunks);
    } else {
      const View z{e.x, w, 1.f, e.p, false};
      const float dot = Sum([&](int32_t l) { return KgLaneDot<V>(z, e.inv, gy, l, lanes, chunks); });
      for (int32_t l = 0; l < lanes; ++l) KgLaneRowGrad<V>(true, true, z, e.ss, e.inv, dot, gy, gy, l, lanes, chunks);
      const KgAccRow<V, HostAcc<V>> gr{gy};
      const float q = Sum([&](int32_t l) { return KgLaneProjDot<V>(gr, w, 1.f, l, lanes, chunks); });
      HostAcc<V> oa{out_aux};
      for (int32_t l = 0; l < lanes; ++l)
        KgLaneTransferGrad<V>(e.x.ok, e.x, e.a, e.p, q, gy, gy, oa, gaux, l, lanes, chunks);
    }
  }
  // gy -> gx of a normalised row (rel, hyper)
  void RowGrad(const HostRow<V>& x, float ss, float inv, HostAcc<V>& gy) const {
    const float dot = Sum([&](int32_t l) { return KgLaneDot<V>(x, inv, gy, l, lanes, chunks); });
    for (int32_t l = 0; l < lanes; ++l) KgLaneRowGrad<V>(x.ok, true, x, ss, inv, dot, gy, gy, l, lanes, chunks);
  }
};

template <int V>
void Forward(const Args& a, float* pos, float* neg_out) {
  const int64_t kp = a.corrupt == kKgBoth ? 2 * a.k : a.k;
  for (int64_t t = 0; t < a.b; ++t) {
    const Task<V> T(a, t);
    const auto h = T.Project(a.src[t]), tl = T.Project(a.dst[t]);
    pos[t] = KgFinish(a.kind, T.Terms(h, tl));
    for (int64_t k = 0; k < a.k; ++k) {
      const auto n = T.Project(a.neg[t * a.k + k]);
      if (a.corrupt != kKgTail) neg_out[t * kp + k] = KgFinish(a.kind, T.Terms(n, tl));
      if (a.corrupt != kKgFront)
        neg_out[t * kp + (a.corrupt == kKgBoth ? a.k : 0) + k] = KgFinish(a.kind, T.Terms(h, n));
    }
  }
}

struct Grads {
  const float* g_pos; const float* g_neg;
  float* g_src; float* g_rel; float* g_dst; float* g_neg_rows;
  float* g_rel_aux; float* g_src_aux; float* g_dst_aux; float* g_neg_aux_rows;
};

template <int V>
void Backward(const Args& a, const Grads& g) {
  const int64_t kp = a.corrupt == kKgBoth ? 2 * a.k : a.k;
  const bool aux = a.proj == kKgProjTransfer;
  for (int64_t t = 0; t < a.b; ++t) {
    const Task<V> T(a, t);
    const auto h = T.Project(a.src[t]), tl = T.Project(a.dst[t]);
    HostAcc<V> gh{g.g_src + t * a.d}, gr{g.g_rel + t * a.d}, gt{g.g_dst + t * a.d}, gw{g.g_rel_aux + t * a.d};
    for (int64_t c = 0; c < a.d; ++c) gh.p[c] = gr.p[c] = gt.p[c] = gw.p[c] = 0.f;
    T.ScoreGrad(g.g_pos[t], h, tl, gh, gr, gt);
    for (int64_t k = 0; k < a.k; ++k) {
      const auto n = T.Project(a.neg[t * a.k + k]);
      HostAcc<V> gn{g.g_neg_rows + (t * a.k + k) * a.d};
      for (int64_t c = 0; c < a.d; ++c) gn.p[c] = 0.f;
      if (a.corrupt != kKgTail) T.ScoreGrad(g.g_neg[t * kp + k], n, tl, gn, gr, gt);
      if (a.corrupt != kKgFront) T.ScoreGrad(g.g_neg[t * kp + (a.corrupt == kKgBoth ? a.k : 0) + k], h, n, gh, gr, gn);
      T.Through(n, gn, aux ? g.g_neg_aux_rows + (t * a.k + k) * a.d : nullptr, gw);
    }
    T.Through(h, gh, aux ? g.g_src_aux + t * a.d : nullptr, gw);
    T.Through(tl, gt, aux ? g.g_dst_aux + t * a.d : nullptr, gw);
    T.RowGrad(T.r, T.ssr, T.ir, gr);
    if (a.proj == kKgProjHyper) {
      T.RowGrad(T.w, T.ssw, T.iw, gw);
    } else {
      for (int32_t l = 0; l < T.lanes; ++l)
        KgLaneRowGrad<V>(T.w.ok, false, T.w, 0.f, 1.f, 0.f, gw, gw, l, T.lanes, T.chunks);
    }
  }
}

}  // namespace

// V of the order for fp32 tables at these addresses (the rule the launcher applies); ent_aux may be null
extern "C" int kg_proj_chunk_width(int64_t d, const float* ent, const float* ent_aux, const float* rel,
                                   const float* rel_aux) {
  return KgProjChunkWidth(d, (uintptr_t)ent, (uintptr_t)ent_aux, true, (uintptr_t)rel, (uintptr_t)rel_aux, true);
}

// The forward (g_pos == nullptr) or the gradient of b triples over fp32 host tables.  v: the
// chunk width to use (1, 4, 8 with d % v == 0), or 0 for kg_proj_chunk_width of the tables.
extern "C" int kg_proj_triple(int32_t proj, int32_t kind, int32_t corrupt, int32_t v, const float* ent,
                              const float* ent_aux, int64_t ent_rows, const float* rel, const float* rel_aux,
                              int64_t rel_rows, const int64_t* src, const int64_t* rel_id, const int64_t* dst,
                              const int64_t* neg, int64_t b, int64_t k, int64_t d, float* pos, float* neg_out,
                              const float* g_pos, const float* g_neg, float* g_src, float* g_rel, float* g_dst,
                              float* g_neg_rows, float* g_rel_aux, float* g_src_aux, float* g_dst_aux,
                              float* g_neg_aux_rows) {
  if (proj < 1 || proj > 2 || kind < 0 || kind > 1 || corrupt < 0 || corrupt > 2 || d < 1) return -1;
  if (!rel_aux || (proj == kKgProjTransfer) != (ent_aux != nullptr)) return -1;
  if (v == 0) v = kg_proj_chunk_width(d, ent, ent_aux, rel, rel_aux);
  if ((v != 1 && v != 4 && v != 8) || d % v != 0) return -1;
  const Args a{proj, kind, corrupt, ent, ent_aux, ent_rows, rel, rel_aux, rel_rows, src, rel_id, dst, neg, b, k, d};
  if (!g_pos) {
    if (v == 8) Forward<8>(a, pos, neg_out);
    else if (v == 4) Forward<4>(a, pos, neg_out);
    else Forward<1>(a, pos, neg_out);
  } else {
    const Grads g{g_pos, g_neg, g_src, g_rel, g_dst, g_neg_rows, g_rel_aux, g_src_aux, g_dst_aux, g_neg_aux_rows};
    if (v == 8) Backward<8>(a, g);
    else if (v == 4) Backward<4>(a, g);
    else Backward<1>(a, g);
  }
  return 0;
}
