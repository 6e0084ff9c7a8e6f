// Knowledge-graph triple scoring (TransE with the l1 or l2 norm, DistMult: calculate_energy of
// examples/TransX/transX.py:72-79,105-133 and examples/distmult/distmult.py:74-79,99-126): the
// arithmetic of ONE LANE of one triple, shared by the kernels of kg_score_kernels.hip and by
// tests/csrc/kg_score_check.cc, which compiles this file with the host compiler.  Every operation
// is a correctly rounded fp32 multiply, add, divide or square root (on the device the __f*_rn
// forms / the IEEE sqrt the compiler expands, on the host plain operators and sqrtf in a
// translation unit built with -ffp-contract=off), a comparison or an integer operation: host and
// device return the same bits by construction.
//
// RANGE RULE: every id is a signed int64; an id outside [0, rows) of its table names no row.  It
// is never dereferenced, reads as a row of +0 and its gradient row is written as +0.
// ROWS, widened exactly to fp32: h = N(ent[src]), r = N(rel[rel_id]), t = N(ent[dst]),
// n_k = N(ent[neg[k]]).  N with `normalize` is tf.nn.l2_normalize: ss = sum x_c^2,
// inv = 1 / sqrt(ss > 1e-12f ? ss : 1e-12f), y_c = x_c * inv; without it inv = 1 (x * 1 == x).
// SCORES s(a, r, c), e_c = (a_c + r_c) - c_c:
//   kind 0 trans_l1  -(sum |e_c|)      kind 1 trans_l2  -sqrt(sum e_c * e_c)
//   kind 2 distmult  sum (a_c * r_c) * c_c
// pos = s(h, r, t); front_k = s(n_k, r, t); tail_k = s(h, r, n_k) - the same n_k in both.
//
// SUMMATION ORDER - every sum over columns (ss, the scores, the dot product of the gradient) - is
// the one edge_dot_kernels.hip states, with dh = d and the tables `ent` and `rel`: chunks of V
// adjacent columns, V = 8 when d % 8 == 0 and both tables start on a 16-byte boundary, else V = 4
// when d % 4 == 0 and the tables start on a 16-byte (fp32) / 8-byte (16-bit) boundary, else V = 1;
// L = min(64, the power of two >= d / V) lanes; lane l takes the chunks l, l + L, ... and adds
// their terms one by one in increasing column order, starting FROM its first term; a lane without
// a chunk holds +0; then for off = L / 2, ..., 1: s = s + s[lane ^ off].  Every lane ends with
// the same bits (fp32 addition commutes).
//
// GRADIENT.  Given g (of one score) the normalised-row gradients gy take, per column:
//   trans_l1  k = g * -sign(e_c), sign(0) = 0, which is exact:  gy_a += k, gy_r += k, gy_c += -k
//   trans_l2  q = sqrt(sum e_c * e_c) as in the forward, gq = q == 0 ? 0 : g / q,
//             k = -(gq * e_c): as trans_l1.  q == 0 gives a zero gradient - torch's sub-gradient
//             of the norm; TensorFlow's gradient of sqrt returns NaN there.
//   distmult  gy_a += g * (r_c * c_c), gy_r += g * (a_c * c_c), gy_c += g * (a_c * r_c)
// Every gy starts at +0 and every contribution is one add, in this order: the true triple, then
// k = 0 .. K - 1, front before tail.  Through the normalisation, with gy complete:
//   ss > 1e-12f:  gx_c = inv * (gy_c - y_c * dot), dot = sum y_c * gy_c (the stated order)
//   otherwise:    gx_c = inv * gy_c             without normalize:  gx_c = gy_c
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "mp_weighted.h"
#include "sparse_embed.h"

namespace euler_gpu {

constexpr int kKgTransL1 = 0, kKgTransL2 = 1, kKgDistMult = 2;
constexpr int kKgFront = 0, kKgTail = 1, kKgBoth = 2;
constexpr float kKgEps = 1e-12f;

// V, given d and the addresses of the two tables (the rule of edge_dot_kernels.hip)
inline int32_t KgChunkWidth(int64_t d, uintptr_t ent, bool ent_f32, uintptr_t rel, bool rel_f32) {
  const bool a16 = ent % 16 == 0 && rel % 16 == 0;
  const bool a4 = ent % (ent_f32 ? 16 : 8) == 0 && rel % (rel_f32 ? 16 : 8) == 0;
  return (d % 8 == 0 && a16) ? 8 : (d % 4 == 0 && a4) ? 4 : 1;
}

// log2 L, given the number of chunks
inline int32_t KgLogLanes(int64_t chunks) {
  int32_t log_l = 0;
  while (log_l < 6 && ((int64_t)1 << log_l) < chunks) ++log_l;
  return log_l;
}

EG_MPW_HD bool KgInRange(int64_t id, int64_t rows) { return id >= 0 && id < rows; }

// one term into a lane's running sum: the first is taken as it is
EG_MPW_HD void KgAcc(float m, float* s, bool* first) {
  *s = *first ? m : MpwAdd(*s, m);
  *first = false;
}

EG_MPW_HD float KgAbs(float x) { return x < 0.f ? -x : (x == 0.f ? 0.f : x); }

// inv of a row whose sum of squares is ss
EG_MPW_HD float KgInv(float ss, bool normalize) {
  if (!normalize) return 1.f;
  return MpwDiv(1.f, SeSqrt(ss > kKgEps ? ss : kKgEps));
}

// the score from the combined sum of its terms
EG_MPW_HD float KgFinish(int32_t kind, float s) {
  if (kind == kKgTransL1) return -s;
  if (kind == kKgTransL2) return -SeSqrt(s);
  return s;
}

// gq of trans_l2 from g and the combined sum of e * e; g itself for the other kinds
EG_MPW_HD float KgScale(int32_t kind, float g, float s) {
  if (kind != kKgTransL2) return g;
  const float q = SeSqrt(s);
  return q == 0.f ? 0.f : MpwDiv(g, q);
}

// A Row is what a lane sees of one table row: Chunk(j, f) gives the V raw columns of chunk j,
// widened (+0 for a row the range rule removed).  An Acc is a lane's gy of one row:
// Get(j, f) / Put(j, f) over the same chunks.

// a lane's part of sum x_c^2
template <int V, typename Row>
EG_MPW_HD float KgLaneSumSq(const Row& x, int32_t l, int32_t lanes, int32_t chunks) {
  float s = 0.f;
  bool first = true;
  for (int32_t j = l; j < chunks; j += lanes) {
    float f[V];
    x.Chunk(j, f);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) KgAcc(MpwMul(f[k], f[k]), &s, &first);
  }
  return s;
}

// a lane's part of the terms of s(a, r, c); ia / ir / ic are the rows' inv
template <int V, typename RowA, typename RowR, typename RowC>
EG_MPW_HD float KgLaneScore(int32_t kind, const RowA& a, float ia, const RowR& r, float ir, const RowC& c,
                            float ic, int32_t l, int32_t lanes, int32_t chunks) {
  float s = 0.f;
  bool first = true;
  for (int32_t j = l; j < chunks; j += lanes) {
    float fa[V], fr[V], fc[V];
    a.Chunk(j, fa);
    r.Chunk(j, fr);
    c.Chunk(j, fc);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) {
      const float ya = MpwMul(fa[k], ia), yr = MpwMul(fr[k], ir), yc = MpwMul(fc[k], ic);
      float m;
      if (kind == kKgDistMult) {
        m = MpwMul(MpwMul(ya, yr), yc);
      } else {
        const float e = MpwAdd(MpwAdd(ya, yr), -yc);
        m = kind == kKgTransL1 ? KgAbs(e) : MpwMul(e, e);
      }
      KgAcc(m, &s, &first);
    }
  }
  return s;
}

// the contributions of one scored triple (a, r, c) to a lane's gy_a, gy_r, gy_c; gs = KgScale(...)
template <int V, typename RowA, typename RowR, typename RowC, typename AccA, typename AccR, typename AccC>
EG_MPW_HD void KgLaneScoreGrad(int32_t kind, float gs, const RowA& a, float ia, const RowR& r, float ir,
                               const RowC& c, float ic, AccA& ga, AccR& gr, AccC& gc, int32_t l,
                               int32_t lanes, int32_t chunks) {
  for (int32_t j = l; j < chunks; j += lanes) {
    float fa[V], fr[V], fc[V], pa[V], pr[V], pc[V];
    a.Chunk(j, fa);
    r.Chunk(j, fr);
    c.Chunk(j, fc);
    ga.Get(j, pa);
    gr.Get(j, pr);
    gc.Get(j, pc);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) {
      const float ya = MpwMul(fa[k], ia), yr = MpwMul(fr[k], ir), yc = MpwMul(fc[k], ic);
      if (kind == kKgDistMult) {
        pa[k] = MpwAdd(pa[k], MpwMul(gs, MpwMul(yr, yc)));
        pr[k] = MpwAdd(pr[k], MpwMul(gs, MpwMul(ya, yc)));
        pc[k] = MpwAdd(pc[k], MpwMul(gs, MpwMul(ya, yr)));
      } else {
        const float e = MpwAdd(MpwAdd(ya, yr), -yc);
        float kk;
        if (kind == kKgTransL1) kk = e > 0.f ? -gs : (e < 0.f ? gs : 0.f);
        else kk = -MpwMul(gs, e);
        pa[k] = MpwAdd(pa[k], kk);
        pr[k] = MpwAdd(pr[k], kk);
        pc[k] = MpwAdd(pc[k], -kk);
      }
    }
    ga.Put(j, pa);
    gr.Put(j, pr);
    gc.Put(j, pc);
  }
}

// a lane's part of dot = sum y_c * gy_c
template <int V, typename Row, typename Acc>
EG_MPW_HD float KgLaneDot(const Row& x, float inv, const Acc& gy, int32_t l, int32_t lanes, int32_t chunks) {
  float s = 0.f;
  bool first = true;
  for (int32_t j = l; j < chunks; j += lanes) {
    float f[V], p[V];
    x.Chunk(j, f);
    gy.Get(j, p);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) KgAcc(MpwMul(MpwMul(f[k], inv), p[k]), &s, &first);
  }
  return s;
}

// gy -> gx of a lane's columns, stored through `out` (which may be gy's own storage).
// ok: the row exists; ss, inv: of the row; dot: the combined KgLaneDot (unused unless ss > eps).
template <int V, typename Row, typename Acc, typename Out>
EG_MPW_HD void KgLaneRowGrad(bool ok, bool normalize, const Row& x, float ss, float inv, float dot,
                             const Acc& gy, Out& out, int32_t l, int32_t lanes, int32_t chunks) {
  for (int32_t j = l; j < chunks; j += lanes) {
    float f[V], p[V];
    x.Chunk(j, f);
    gy.Get(j, p);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) {
      if (!ok) p[k] = 0.f;
      else if (normalize && ss > kKgEps) p[k] = MpwMul(inv, MpwAdd(p[k], -MpwMul(MpwMul(f[k], inv), dot)));
      else if (normalize) p[k] = MpwMul(inv, p[k]);
    }
    out.Put(j, p);
  }
}

}  // namespace euler_gpu
