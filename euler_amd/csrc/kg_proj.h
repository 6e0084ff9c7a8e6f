// The TransH and TransD projections fused into triple scoring (projection / generate_embedding of
// examples/TransX/transH.py:43-66 and transD.py:46-73): the arithmetic of ONE LANE of one triple,
// built on kg_score.h, shared by the kernels of kg_proj_kernels.hip and by
// tests/csrc/kg_proj_check.cc, which compiles this file with the host compiler.  As in kg_score.h
// every operation is one correctly rounded fp32 operation without contraction, every sum over
// columns is taken in the order stated there, and the RANGE RULE holds for every table an id
// indexes: an id outside [0, rows) names no row in any of them, is never dereferenced, reads as
// +0 and gets +0 gradient rows.  N(x) is kg_score.h's normalisation with `normalize`.
//
// proj 1 "hyperplane" (TransH).  Tables ent [N, d], rel [R, d], hyper [R, d].
//   w = N(hyper[rel_id]), r = N(rel[rel_id]); for an entity row x (not normalised)
//   p = sum x_c * w_c,  xp_c = x_c + (-(p * w_c));  the scores take hp, r, tp, np_k.
// proj 2 "transfer" (TransD).  Tables ent, ent_transfer [N, d], rel, rel_transfer [R, d].
//   rho = rel_transfer[rel_id] (raw); for entity id i: x = ent[i], a = ent_transfer[i],
//   p = sum x_c * a_c,  z_c = x_c + p * rho_c,  ss = sum z_c * z_c,  inv = KgInv(ss, true),
//   y_c = z_c * inv;  r = N(rel[rel_id]);  the scores take the ys.
// SCORES: kind trans_l1 or trans_l2 of kg_score.h, e_c = (a_c + r_c) - c_c, KgFinish; corrupt and
// the layout of the outputs as there.  The projection of n_k is computed once per k and serves
// the front and the tail score.
//
// GRADIENT.  The score-level gradients gy are KgLaneScoreGrad's (sign(0) = 0, gq = 0 where q == 0,
// every gy from +0, the true triple, then k = 0 .. K - 1, front before tail).  An entity row goes
// through its projection once its gy is complete - n_k at the end of iteration k, then h, then t:
//   proj 1  q = sum gy_c * w_c,  gx_c = gy_c + (-(q * w_c)),
//           gw_c = gw_c + (-((q * x_c) + (p * gy_c)));  gw starts at +0, takes the rows in the
//           order n_0 .. n_{K-1}, h, t and then goes through hyper's normalisation (KgLaneRowGrad).
//   proj 2  dot = sum y_c * gy_c,  gz_c = inv * (gy_c - y_c * dot) where ss > 1e-12f, else
//           inv * gy_c;  q = sum gz_c * rho_c,  gx_c = gz_c + q * a_c,  ga_c = q * x_c,
//           grho_c = grho_c + p * gz_c in the same row order; grho is the raw row's gradient.
//   g_rel goes through rel's normalisation as in kg_score.h.
//
// CHUNK WIDTH: KgChunkWidth over every table passed (KgProjChunkWidth below); L and the butterfly
// as in kg_score.h.  The order depends on d, the dtypes and the alignments only.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "kg_score.h"

namespace euler_gpu {

constexpr int kKgProjHyper = 1, kKgProjTransfer = 2;

// V, given d and the addresses of all tables (an absent aux table: 0): 8 when d % 8 == 0 and all
// start on 16 bytes, else 4 when d % 4 == 0 with fp32 tables on 16 bytes and 16-bit ones on 8
inline int32_t KgProjChunkWidth(int64_t d, uintptr_t ent, uintptr_t ent_aux, bool ent_f32, uintptr_t rel,
                                uintptr_t rel_aux, bool rel_f32) {
  const int32_t v0 = KgChunkWidth(d, ent, ent_f32, rel, rel_f32);
  const int32_t v1 = KgChunkWidth(d, ent_aux, ent_f32, rel_aux, rel_f32);
  return v0 < v1 ? v0 : v1;
}

// an Acc read as a Row
template <int V, typename Acc>
struct KgAccRow {
  const Acc& a;
  EG_MPW_HD void Chunk(int32_t j, float f[V]) const { a.Get(j, f); }
};

// a lane's part of sum x_c * (w_c * iw); iw = 1 for a raw w (w * 1 == w)
template <int V, typename RowX, typename RowW>
EG_MPW_HD float KgLaneProjDot(const RowX& x, const RowW& w, float iw, int32_t l, int32_t lanes, int32_t chunks) {
  float s = 0.f;
  bool first = true;
  for (int32_t j = l; j < chunks; j += lanes) {
    float fx[V], fw[V];
    x.Chunk(j, fx);
    w.Chunk(j, fw);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) KgAcc(MpwMul(fx[k], MpwMul(fw[k], iw)), &s, &first);
  }
  return s;
}

// The projected row as a Row: x_c + m, m = p * (w_c * iw), taken as -m when neg.
// proj 1: w = hyper with its inv, neg - the row xp;  proj 2: w = rho, iw = 1 - the row z.
template <int V, typename RowX, typename RowW>
struct KgProjRow {
  const RowX& x;
  const RowW& w;
  float iw, p;
  bool neg;
  EG_MPW_HD void Chunk(int32_t j, float f[V]) const {
    float fw[V];
    x.Chunk(j, f);
    w.Chunk(j, fw);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) {
      const float m = MpwMul(p, MpwMul(fw[k], iw));
      f[k] = MpwAdd(f[k], neg ? -m : m);
    }
  }
};

// proj 1, one entity row with gy complete and q combined: gx -> out (which may be gy's own
// storage; +0 for a row that does not exist), and the row's term into gw
template <int V, typename RowX, typename RowW, typename Acc, typename Out, typename AccW>
EG_MPW_HD void KgLaneHyperGrad(bool ok, const RowX& x, const RowW& w, float iw, float p, float q, const Acc& gy,
                               Out& out, AccW& gw, int32_t l, int32_t lanes, int32_t chunks) {
  for (int32_t j = l; j < chunks; j += lanes) {
    float fx[V], fw[V], g[V], pw[V];
    x.Chunk(j, fx);
    w.Chunk(j, fw);
    gy.Get(j, g);
    gw.Get(j, pw);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) {
      pw[k] = MpwAdd(pw[k], -MpwAdd(MpwMul(q, fx[k]), MpwMul(p, g[k])));
      g[k] = ok ? MpwAdd(g[k], -MpwMul(q, MpwMul(fw[k], iw))) : 0.f;
    }
    gw.Put(j, pw);
    out.Put(j, g);
  }
}

// proj 2, one entity row with gz in place of gy and q combined: gx -> out (which may be gz's own
// storage), ga -> out_aux (both +0 for a row that does not exist), and the row's term into grho
template <int V, typename RowX, typename RowA, typename Acc, typename Out, typename OutA, typename AccR>
EG_MPW_HD void KgLaneTransferGrad(bool ok, const RowX& x, const RowA& a, float p, float q, const Acc& gz, Out& out,
                                  OutA& out_aux, AccR& grho, int32_t l, int32_t lanes, int32_t chunks) {
  for (int32_t j = l; j < chunks; j += lanes) {
    float fx[V], fa[V], g[V], pr[V], ga[V];
    x.Chunk(j, fx);
    a.Chunk(j, fa);
    gz.Get(j, g);
    grho.Get(j, pr);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) {
      pr[k] = MpwAdd(pr[k], MpwMul(p, g[k]));
      ga[k] = ok ? MpwMul(q, fx[k]) : 0.f;
      g[k] = ok ? MpwAdd(g[k], MpwMul(q, fa[k])) : 0.f;
    }
    grho.Put(j, pr);
    out_aux.Put(j, ga);
    out.Put(j, g);
  }
}

}  // namespace euler_gpu
