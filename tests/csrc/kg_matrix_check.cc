// Host build of the arithmetic of triple scoring with TransR's matrix projection
// (euler_amd/csrc/kg_matrix.h) for tests/test_triple_score_matrix_host.py: the same lane functions
// and register rows (KgmRegs, KgmStep, KgmRowDot) the kernels use, over plain host arrays, with
// the L lanes of a task run one after the other and combined by the butterfly kg_score.h states.
// Built with -ffp-contract=off.
#include <stdint.h>

#include <vector>

#include "kg_matrix.h"

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
struct HostOut {           // an output row
  float* p;
  void Put(int32_t j, const float f[V]) { for (int k = 0; k < V; ++k) p[(int64_t)j * V + k] = f[k]; }
};

struct Args {
  int32_t kind, corrupt;
  const float* ent; int64_t ent_rows, de;
  const float* rel; int64_t rel_rows, dr;
  const float* matrix;
  const int64_t* src; const int64_t* rel_id; const int64_t* dst; const int64_t* neg;
  int64_t b, k;
};

template <int V>
struct Lanes {             // a projected row (or its gy): the registers of each of the L lanes
  KgmRegs<V> lane[64];
  float ss, inv;
  bool ok;                 // the entity id names a row
  const float* x;
};

template <int V>
struct Task {
  const Args& a;
  int32_t lanes, log_l, chunks;
  HostRow<V> r;
  const float* m;          // M_rho, or nullptr
  float ssr, ir;
  std::vector<float> zero;

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
  Task(const Args& args, int64_t t) : a(args), zero(args.dr, 0.f) {
    chunks = (int32_t)(a.dr / V);
    log_l = KgLogLanes(chunks);
    lanes = 1 << log_l;
    const bool ok = KgInRange(a.rel_id[t], a.rel_rows);
    r = HostRow<V>{ok ? a.rel + a.rel_id[t] * a.dr : nullptr, ok};
    m = ok ? a.matrix + a.rel_id[t] * a.de * a.dr : nullptr;
    ssr = Sum([&](int32_t l) { return KgLaneSumSq<V>(r, l, lanes, chunks); });
    ir = KgInv(ssr, true);
  }
  void Clear(Lanes<V>* g) const {
    for (int32_t l = 0; l < lanes; ++l) g->lane[l].Clear(log_l);
  }
  void Project(int64_t id, Lanes<V>* e) const {
    e->ok = KgInRange(id, a.ent_rows);
    e->x = e->ok ? a.ent + id * a.de : nullptr;
    Clear(e);
    for (int32_t l = 0; l < lanes; ++l) {
      int32_t col[kKgmCols / V];
      KgmSlots<V>(l, lanes, chunks, col);
      for (int64_t c = 0; c < a.de; ++c)
        KgmStep<V>(e->lane[l], e->ok ? e->x[c] : 0.f, m ? m + c * a.dr : zero.data(), col, c == 0);
    }
    e->ss = Sum([&](int32_t l) { return KgLaneSumSq<V>(e->lane[l], l, lanes, chunks); });
    e->inv = KgInv(e->ss, true);
  }
  float Terms(const Lanes<V>& x, const Lanes<V>& c) const {
    return Sum([&](int32_t l) { return KgLaneScore<V>(a.kind, x.lane[l], x.inv, r, ir, c.lane[l], c.inv, l, lanes, chunks); });
  }
  void ScoreGrad(float g, const Lanes<V>& x, const Lanes<V>& c, Lanes<V>* gx, Lanes<V>* gr, Lanes<V>* gc) const {
    const float s = a.kind == kKgTransL2 ? Terms(x, c) : 0.f;
    const float gs = KgScale(a.kind, g, s);
    for (int32_t l = 0; l < lanes; ++l)
      KgLaneScoreGrad<V>(a.kind, gs, x.lane[l], x.inv, r, ir, c.lane[l], c.inv, gx->lane[l], gr->lane[l], gc->lane[l],
                         l, lanes, chunks);
  }
  // a projected row with gy complete: gz -> its row, then gx = gz . M^T (+0 for no entity row)
  void Through(const Lanes<V>& e, const Lanes<V>& gy, float* gz, float* gx) const {
    const float dot = Sum([&](int32_t l) { return KgLaneDot<V>(e.lane[l], e.inv, gy.lane[l], l, lanes, chunks); });
    HostOut<V> out{gz};
    for (int32_t l = 0; l < lanes; ++l)
      KgLaneRowGrad<V>(true, true, e.lane[l], e.ss, e.inv, dot, gy.lane[l], out, l, lanes, chunks);
    for (int64_t c = 0; c < a.de; ++c)
      gx[c] = e.ok ? KgmRowDot(gz, m ? m + c * a.dr : zero.data(), (int32_t)a.dr) : 0.f;
  }
};

template <int V>
void Forward(const Args& a, float* pos, float* neg_out) {
  const int64_t kp = a.corrupt == kKgBoth ? 2 * a.k : a.k;
  std::vector<Lanes<V>> rows(3);
  Lanes<V>&h = rows[0], &tl = rows[1], &n = rows[2];
  for (int64_t t = 0; t < a.b; ++t) {
    const Task<V> T(a, t);
    T.Project(a.src[t], &h);
    T.Project(a.dst[t], &tl);
    pos[t] = KgFinish(a.kind, T.Terms(h, tl));
    for (int64_t k = 0; k < a.k; ++k) {
      T.Project(a.neg[t * a.k + k], &n);
      if (a.corrupt != kKgTail) neg_out[t * kp + k] = KgFinish(a.kind, T.Terms(n, tl));
      if (a.corrupt != kKgFront)
        neg_out[t * kp + (a.corrupt == kKgBoth ? a.k : 0) + k] = KgFinish(a.kind, T.Terms(h, n));
    }
  }
}

struct Grads {
  const float* g_pos; const float* g_neg;
  float* g_src; float* g_rel; float* g_dst; float* g_neg_rows;
  float* gz_src; float* gz_dst; float* gz_neg_rows;
  float* g_matrix;         // [rel_rows, de * dr]
};

template <int V>
void Backward(const Args& a, const Grads& g) {
  const int64_t kp = a.corrupt == kKgBoth ? 2 * a.k : a.k;
  std::vector<Lanes<V>> rows(7);
  Lanes<V>&h = rows[0], &tl = rows[1], &n = rows[2], &gh = rows[3], &gt = rows[4], &gn = rows[5], &gr = rows[6];
  for (int64_t t = 0; t < a.b; ++t) {
    const Task<V> T(a, t);
    T.Project(a.src[t], &h);
    T.Project(a.dst[t], &tl);
    T.Clear(&gh);
    T.Clear(&gt);
    T.Clear(&gr);
    T.ScoreGrad(g.g_pos[t], h, tl, &gh, &gr, &gt);
    for (int64_t k = 0; k < a.k; ++k) {
      T.Project(a.neg[t * a.k + k], &n);
      T.Clear(&gn);
      if (a.corrupt != kKgTail) T.ScoreGrad(g.g_neg[t * kp + k], n, tl, &gn, &gr, &gt);
      if (a.corrupt != kKgFront) T.ScoreGrad(g.g_neg[t * kp + (a.corrupt == kKgBoth ? a.k : 0) + k], h, n, &gh, &gr, &gn);
      T.Through(n, gn, g.gz_neg_rows + (t * a.k + k) * a.dr, g.g_neg_rows + (t * a.k + k) * a.de);
    }
    T.Through(h, gh, g.gz_src + t * a.dr, g.g_src + t * a.de);
    T.Through(tl, gt, g.gz_dst + t * a.dr, g.g_dst + t * a.de);
    const float dot = T.Sum([&](int32_t l) { return KgLaneDot<V>(T.r, T.ir, gr.lane[l], l, T.lanes, T.chunks); });
    HostOut<V> out{g.g_rel + t * a.dr};
    for (int32_t l = 0; l < T.lanes; ++l)
      KgLaneRowGrad<V>(T.r.ok, true, T.r, T.ssr, T.ir, dot, gr.lane[l], out, l, T.lanes, T.chunks);
  }
  // G_M: per relation the occurrences by increasing t, within a triple n_0 .. n_{K-1}, h, t
  std::vector<char> started(a.rel_rows, 0);
  for (int64_t i = 0; i < a.rel_rows * a.de * a.dr; ++i) g.g_matrix[i] = 0.f;
  for (int64_t t = 0; t < a.b; ++t) {
    const int64_t rho = a.rel_id[t];
    if (!KgInRange(rho, a.rel_rows)) continue;
    float* gm = g.g_matrix + rho * a.de * a.dr;
    for (int64_t role = 0; role < a.k + 2; ++role) {
      const int64_t id = role < a.k ? a.neg[t * a.k + role] : role == a.k ? a.src[t] : a.dst[t];
      const float* gz = role < a.k ? g.gz_neg_rows + (t * a.k + role) * a.dr
                                   : (role == a.k ? g.gz_src : g.gz_dst) + t * a.dr;
      if (!KgInRange(id, a.ent_rows)) continue;
      const float* x = a.ent + id * a.de;
      bool first = !started[rho];
      for (int64_t c = 0; c < a.de; ++c)
        for (int64_t j = 0; j < a.dr; ++j) {
          bool f = first;
          KgAcc(MpwMul(x[c], gz[j]), &gm[c * a.dr + j], &f);
        }
      started[rho] = 1;
    }
  }
}

}  // namespace

// V of the dr-sums for an fp32 rel table at this address (the rule the launcher applies)
extern "C" int kg_matrix_chunk_width(int64_t dr, const float* rel) {
  return KgMatrixChunkWidth(dr, (uintptr_t)rel, true);
}

// The forward (g_pos == nullptr) or the gradient of b triples over fp32 host tables.  v: the
// chunk width to use (1, 4, 8 with dr % v == 0), or 0 for kg_matrix_chunk_width of rel.
extern "C" int kg_matrix_triple(int32_t kind, int32_t corrupt, int32_t v, const float* ent, int64_t ent_rows,
                                int64_t de, const float* rel, int64_t rel_rows, int64_t dr, const float* matrix,
                                const int64_t* src, const int64_t* rel_id, const int64_t* dst, const int64_t* neg,
                                int64_t b, int64_t k, float* pos, float* neg_out, const float* g_pos,
                                const float* g_neg, float* g_src, float* g_rel, float* g_dst, float* g_neg_rows,
                                float* gz_src, float* gz_dst, float* gz_neg_rows, float* g_matrix) {
  if (kind < 0 || kind > 1 || corrupt < 0 || corrupt > 2 || de < 1 || dr < 1) return -1;
  if (de > kKgMatrixMaxDim || dr > kKgMatrixMaxDim) return -1;
  if (v == 0) v = kg_matrix_chunk_width(dr, rel);
  if ((v != 1 && v != 4 && v != 8) || dr % v != 0) return -1;
  const Args a{kind, corrupt, ent, ent_rows, de, rel, rel_rows, dr, matrix, src, rel_id, dst, neg, b, k};
  if (!g_pos) {
    if (v == 8) Forward<8>(a, pos, neg_out);
    else if (v == 4) Forward<4>(a, pos, neg_out);
    else Forward<1>(a, pos, neg_out);
  } else {
    const Grads g{g_pos, g_neg, g_src, g_rel, g_dst, g_neg_rows, gz_src, gz_dst, gz_neg_rows, g_matrix};
    if (v == 8) Backward<8>(a, g);
    else if (v == 4) Backward<4>(a, g);
    else Backward<1>(a, g);
  }
  return 0;
}
