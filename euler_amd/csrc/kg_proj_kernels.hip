// Fused triple scoring with the TransH ("hyperplane") and TransD ("transfer") projections on
// gfx950 and its gradient, with their C-ABI entry points: the lookups of the one or two extra
// tables, the projection of every entity row (one dot product and one axpy a row), TransD's
// second normalisation and the 1 + K' scores of a triple in one pass, where the composition
// tiles the hyperplane / transfer rows over the k negatives and builds [b, k, d] blocks again.
// The arithmetic, the range rule and the order are stated in kg_proj.h and kg_score.h, which the
// host check compiles too.  The argument ladder, the dtype fan-out and the launch shape are
// kg_entry.h's; this file adds the aux tables to them and the aux gradient rules in its entries.
//
// The design is that of kg_score_kernels.hip: a triple is a task of L lanes of a wave, partial
// sums are combined inside the wave (__shfl_xor) - no LDS, no atomics.  While a lane owns one
// chunk (d / V <= 64) the forward kernels, and the gradient kernels with V < 8, keep the rows of
// the true triple - and the gradient their gy - in registers over the k negatives (REG); wider
// rows, and every row of the gradient with V = 8 (LaunchForm), are read again from the tables,
// which L2 serves, and gy accumulates in the lane's own columns of the output rows.  The order
// depends on neither.  Every loop that holds a shuffle has a trip count that is the same
// for all lanes of a wave: a task past the end runs on rows the range rule removed.
#include <hip/hip_runtime.h>

#include "device_fns.h"
#include "device_mem.h"
#include "half_cvt.h"
#include "kg_entry.h"
#include "kg_lanes.h"
#include "kg_proj.h"

namespace euler_gpu {
namespace {

struct KgProjArgs : KgTripleArgs {
  int64_t d;
  const void* ent_aux; const void* rel_aux;
  float* g_rel_aux; float* g_src_aux; float* g_dst_aux; float* g_neg_aux_rows;   // gradient
};

// An entity row of a task with what its projection gives: x (and for proj 2 its transfer row a),
// p, and the ss / inv of proj 2's second normalisation (inv = 1 for proj 1: xp * 1 == xp).
template <int PROJ, int DE, int V, bool REG>
struct ProjEnt {
  LaneRow<DE, V, REG> x;
  LaneRow<DE, V, REG && PROJ == kKgProjTransfer> a;
  float p, ss, inv;
  // w: hyper with its inv iw (proj 1) or rel_transfer with iw = 1 (proj 2)
  template <typename RowW>
  __device__ __forceinline__ void Open(const KgProjArgs& g, int64_t id, const RowW& w, float iw, int32_t l,
                                       int32_t lanes, int32_t chunks) {
    x.Open(g.ent, id, g.ent_rows, g.d, l, chunks);
    if constexpr (PROJ == kKgProjHyper) {
      p = KgCombine(KgLaneProjDot<V>(x, w, iw, l, lanes, chunks), lanes);
      ss = 0.f;
      inv = 1.f;
    } else {
      a.Open(g.ent_aux, id, g.ent_rows, g.d, l, chunks);
      p = KgCombine(KgLaneProjDot<V>(x, a, 1.f, l, lanes, chunks), lanes);
      const KgProjRow<V, LaneRow<DE, V, REG>, RowW> z{x, w, 1.f, p, false};
      KgLaneNorm<V>(z, true, l, lanes, chunks, &ss, &inv);
    }
  }
  template <typename RowW>
  __device__ __forceinline__ KgProjRow<V, LaneRow<DE, V, REG>, RowW> View(const RowW& w, float iw) const {
    return KgProjRow<V, LaneRow<DE, V, REG>, RowW>{x, w, iw, p, PROJ == kKgProjHyper};
  }
};

template <int PROJ, int DE, int DR, int V, bool REG>
__global__ __launch_bounds__(256) void TripleScoreProjKernel(const KgProjArgs a) {
  const int32_t lanes = 1 << a.log_l;
  const int32_t lane = threadIdx.x & 63;
  const int32_t sub = lane >> a.log_l, l = lane & (lanes - 1);
  const int64_t tasks_per_wave = 64 >> a.log_l;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int32_t chunks = (int32_t)(a.d / V);
  for (int64_t t0 = wave * tasks_per_wave; t0 < a.b; t0 += waves * tasks_per_wave) {
    const int64_t t = t0 + sub;
    const bool live = t < a.b;
    const int64_t rid = live ? a.rel_id[t] : -1;
    LaneRow<DR, V, REG> R, W;
    R.Open(a.rel, rid, a.rel_rows, a.d, l, chunks);
    W.Open(a.rel_aux, rid, a.rel_rows, a.d, l, chunks);
    float ss, ir, iw = 1.f;
    KgLaneNorm<V>(R, true, l, lanes, chunks, &ss, &ir);
    if constexpr (PROJ == kKgProjHyper) KgLaneNorm<V>(W, true, l, lanes, chunks, &ss, &iw);
    ProjEnt<PROJ, DE, V, REG> H, T, N;
    H.Open(a, live ? a.src[t] : -1, W, iw, l, lanes, chunks);
    T.Open(a, live ? a.dst[t] : -1, W, iw, l, lanes, chunks);
    const auto hv = H.View(W, iw), tv = T.View(W, iw);
    const float pos = KgFinish(a.kind, KgCombine(KgLaneScore<V>(a.kind, hv, H.inv, R, ir, tv, T.inv, l, lanes, chunks), lanes));
    if (live && l == 0) a.pos_out[t] = pos;
    for (int64_t k = 0; k < a.k; ++k) {
      N.Open(a, live ? a.neg[t * a.k + k] : -1, W, iw, l, lanes, chunks);
      const auto nv = N.View(W, iw);
      KgLaneCorrupt<V>(a.kind, a.corrupt, hv, H.inv, R, ir, tv, T.inv, nv, N.inv, l, lanes, chunks,
                       [&](bool tail, float s) {
                         if (live && l == 0) a.neg_out[KgNegSlot(a.corrupt, a.k, t, k, tail)] = s;
                       });
    }
  }
}

// gy -> gx of a normalised row (rel, hyper), written to its output row
template <int V, typename Row, typename Acc>
__device__ __forceinline__ void KgProjRowGrad(const Row& x, float ss, float inv, const Acc& gy, LaneOut<V> out,
                                              int32_t l, int32_t lanes, int32_t chunks) {
  const float dot = KgCombine(KgLaneDot<V>(x, inv, gy, l, lanes, chunks), lanes);
  KgLaneRowGrad<V>(x.ok, true, x, ss, inv, dot, gy, out, l, lanes, chunks);
}

// An entity row whose gy is complete goes through its projection: gx -> out, for proj 2 ga ->
// out_aux, and the row's term into gaux (gw of proj 1, grho of proj 2).
template <int PROJ, int DE, int V, bool REG, typename RowW, typename Acc>
__device__ __forceinline__ void KgThrough(const ProjEnt<PROJ, DE, V, REG>& e, const RowW& w, float iw, Acc& gy,
                                          LaneOut<V> out, LaneOut<V> out_aux, Acc& gaux, int32_t l, int32_t lanes,
                                          int32_t chunks) {
  if constexpr (PROJ == kKgProjHyper) {
    const KgAccRow<V, Acc> gr{gy};
    const float q = KgCombine(KgLaneProjDot<V>(gr, w, iw, l, lanes, chunks), lanes);
    KgLaneHyperGrad<V>(e.x.ok, e.x, w, iw, e.p, q, gy, out, gaux, l, lanes, chunks);
  } else {
    const auto z = e.View(w, 1.f);
    const float dot = KgCombine(KgLaneDot<V>(z, e.inv, gy, l, lanes, chunks), lanes);
    KgLaneRowGrad<V>(true, true, z, e.ss, e.inv, dot, gy, gy, l, lanes, chunks);       // gz in place of gy
    const KgAccRow<V, Acc> gr{gy};
    const float q = KgCombine(KgLaneProjDot<V>(gr, w, 1.f, l, lanes, chunks), lanes);
    KgLaneTransferGrad<V>(e.x.ok, e.x, e.a, e.p, q, gy, out, out_aux, gaux, l, lanes, chunks);
  }
}

template <int PROJ, int DE, int DR, int V, bool REG>
__global__ __launch_bounds__(256) void TripleScoreProjGradKernel(const KgProjArgs a) {
  const int32_t lanes = 1 << a.log_l;
  const int32_t lane = threadIdx.x & 63;
  const int32_t sub = lane >> a.log_l, l = lane & (lanes - 1);
  const int64_t tasks_per_wave = 64 >> a.log_l;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int32_t chunks = (int32_t)(a.d / V);
  const bool vec = a.out_vec != 0;
  constexpr bool kAux = PROJ == kKgProjTransfer;  // the entity tables' aux gradient rows exist
  for (int64_t t0 = wave * tasks_per_wave; t0 < a.b; t0 += waves * tasks_per_wave) {
    const int64_t t = t0 + sub;
    const bool live = t < a.b;
    const int64_t tt = live ? t : 0;
    const int64_t rid = live ? a.rel_id[t] : -1;
    LaneRow<DR, V, REG> R, W;
    R.Open(a.rel, rid, a.rel_rows, a.d, l, chunks);
    W.Open(a.rel_aux, rid, a.rel_rows, a.d, l, chunks);
    float ssr, ssw = 0.f, ir, iw = 1.f;
    KgLaneNorm<V>(R, true, l, lanes, chunks, &ssr, &ir);
    if constexpr (PROJ == kKgProjHyper) KgLaneNorm<V>(W, true, l, lanes, chunks, &ssw, &iw);
    ProjEnt<PROJ, DE, V, REG> H, T, N;
    H.Open(a, live ? a.src[t] : -1, W, iw, l, lanes, chunks);
    T.Open(a, live ? a.dst[t] : -1, W, iw, l, lanes, chunks);
    const auto hv = H.View(W, iw), tv = T.View(W, iw);
    const LaneOut<V> oh{a.g_src + tt * a.d, live, vec}, orl{a.g_rel + tt * a.d, live, vec},
        ot{a.g_dst + tt * a.d, live, vec}, ow{a.g_rel_aux + tt * a.d, live, vec},
        oha{kAux ? a.g_src_aux + tt * a.d : nullptr, live && kAux, vec},
        ota{kAux ? a.g_dst_aux + tt * a.d : nullptr, live && kAux, vec};
    LaneAcc<V, REG> gh, gr, gt, gn, gw;
    gh.Open(oh, l, lanes, chunks);
    gr.Open(orl, l, lanes, chunks);
    gt.Open(ot, l, lanes, chunks);
    gw.Open(ow, l, lanes, chunks);
    {
      const float s = a.kind == kKgTransL2
                          ? KgCombine(KgLaneScore<V>(a.kind, hv, H.inv, R, ir, tv, T.inv, l, lanes, chunks), lanes)
                          : 0.f;
      const float gs = KgScale(a.kind, live ? a.g_pos[t] : 0.f, s);
      KgLaneScoreGrad<V>(a.kind, gs, hv, H.inv, R, ir, tv, T.inv, gh, gr, gt, l, lanes, chunks);
    }
    for (int64_t k = 0; k < a.k; ++k) {
      N.Open(a, live ? a.neg[t * a.k + k] : -1, W, iw, l, lanes, chunks);
      const auto nv = N.View(W, iw);
      const LaneOut<V> on{a.g_neg_rows + (tt * a.k + k) * a.d, live, vec},
          ona{kAux ? a.g_neg_aux_rows + (tt * a.k + k) * a.d : nullptr, live && kAux, vec};
      gn.Open(on, l, lanes, chunks);
      const auto g = [&](bool tail) { return live ? a.g_neg[KgNegSlot(a.corrupt, a.k, t, k, tail)] : 0.f; };
      KgLaneCorruptGrad<V>(a.kind, a.corrupt, g, hv, H.inv, R, ir, tv, T.inv, nv, N.inv, gh, gr, gt, gn, l, lanes,
                           chunks);
      KgThrough(N, W, iw, gn, on, ona, gw, l, lanes, chunks);
    }
    KgThrough(H, W, iw, gh, oh, oha, gw, l, lanes, chunks);
    KgThrough(T, W, iw, gt, ot, ota, gw, l, lanes, chunks);
    KgProjRowGrad<V>(R, ssr, ir, gr, orl, l, lanes, chunks);
    if constexpr (PROJ == kKgProjHyper) {
      KgProjRowGrad<V>(W, ssw, iw, gw, ow, l, lanes, chunks);
    } else {
      LaneOut<V> out = ow;                        // grho is the raw row's gradient: +0 for no row
      KgLaneRowGrad<V>(W.ok, false, W, 0.f, 1.f, 0.f, gw, out, l, lanes, chunks);
    }
  }
}

template <int PROJ, int DE, int DR, int V, bool REG, bool GRAD>
void LaunchOne(hipStream_t st, const KgProjArgs& a, dim3 grid) {
  if constexpr (GRAD) hipLaunchKernelGGL((TripleScoreProjGradKernel<PROJ, DE, DR, V, REG>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((TripleScoreProjKernel<PROJ, DE, DR, V, REG>), grid, dim3(256), 0, st, a);
}

// The register form needs a lane to own at most one chunk (reg).  The gradient with V = 8 would
// hold five rows and five gy of eight columns (the transfer one three rows more): 256 VGPRs and
// AGPRs on top, one wave a SIMD.  It takes the memory form at every d (two waves a SIMD).
template <int PROJ, int DE, int DR, int V>
void LaunchForm(hipStream_t st, const KgProjArgs& a, bool grad, dim3 grid, bool reg) {
  if (!grad) {
    reg ? LaunchOne<PROJ, DE, DR, V, true, false>(st, a, grid) : LaunchOne<PROJ, DE, DR, V, false, false>(st, a, grid);
  } else if constexpr (V == 8) {
    LaunchOne<PROJ, DE, DR, V, false, true>(st, a, grid);
  } else {
    reg ? LaunchOne<PROJ, DE, DR, V, true, true>(st, a, grid) : LaunchOne<PROJ, DE, DR, V, false, true>(st, a, grid);
  }
}

template <int PROJ, int DE, int DR>
int LaunchProj(hipStream_t st, KgProjArgs a, bool grad) {
  const int32_t v = KgProjChunkWidth(a.d, (uintptr_t)a.ent, (uintptr_t)a.ent_aux, DE == kF32, (uintptr_t)a.rel,
                                     (uintptr_t)a.rel_aux, DR == kF32);
  const KgLaunchShape shape = KgTaskLaunch(a.b, a.d / v);
  a.log_l = shape.log_l;
  const dim3 grid(shape.grid);
  if (v == 8) LaunchForm<PROJ, DE, DR, 8>(st, a, grad, grid, shape.reg);
  else if (v == 4) LaunchForm<PROJ, DE, DR, 4>(st, a, grad, grid, shape.reg);
  else LaunchForm<PROJ, DE, DR, 1>(st, a, grad, grid, shape.reg);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int Dispatch(hipStream_t st, int32_t proj, const KgProjArgs& a, int32_t ent_dtype, int32_t rel_dtype, bool grad) {
  return KgDispatchTables(ent_dtype, rel_dtype, [&](auto de, auto dr) {
    if (proj == kKgProjHyper) return LaunchProj<kKgProjHyper, de, dr>(st, a, grad);
    return LaunchProj<kKgProjTransfer, de, dr>(st, a, grad);
  });
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_triple_score_proj(void* stream, int32_t proj, int32_t kind, int32_t corrupt,
                                const void* ent_dev, const void* ent_aux_dev, int32_t ent_dtype, int64_t ent_rows,
                                const void* rel_dev, const void* rel_aux_dev, int32_t rel_dtype, int64_t rel_rows,
                                const int64_t* src_dev, const int64_t* rel_id_dev, const int64_t* dst_dev,
                                const int64_t* neg_dev, int64_t b, int64_t k, int64_t d,
                                float* pos_out_dev, float* neg_out_dev) {
  const KgProjArgs a{KgShared(kind, corrupt, ent_dev, ent_rows, rel_dev, rel_rows, src_dev, rel_id_dev, dst_dev,
                              neg_dev, b, k, pos_out_dev, neg_out_dev),
                     d, ent_aux_dev, rel_aux_dev};
  bool run;
  const int rc = CheckKgCall({"triple_score_proj", kKgProjFamily, ent_dtype, rel_dtype, d, proj, ent_aux_dev, rel_aux_dev},
                             a, &run);
  if (rc != EULER_GPU_OK || !run) return rc;
  if (!pos_out_dev || (k > 0 && !neg_out_dev)) return Fail(EULER_GPU_EINVAL, "triple_score_proj: null output buffer");
  return Dispatch((hipStream_t)stream, proj, a, ent_dtype, rel_dtype, false);
}

int euler_gpu_triple_score_proj_grad(void* stream, int32_t proj, int32_t kind, int32_t corrupt,
                                     const void* ent_dev, const void* ent_aux_dev, int32_t ent_dtype,
                                     int64_t ent_rows, const void* rel_dev, const void* rel_aux_dev,
                                     int32_t rel_dtype, int64_t rel_rows, const int64_t* src_dev,
                                     const int64_t* rel_id_dev, const int64_t* dst_dev, const int64_t* neg_dev,
                                     int64_t b, int64_t k, int64_t d, const float* g_pos_dev, const float* g_neg_dev,
                                     float* g_src_dev, float* g_rel_dev, float* g_dst_dev, float* g_neg_rows_dev,
                                     float* g_rel_aux_dev, float* g_src_aux_dev, float* g_dst_aux_dev,
                                     float* g_neg_aux_rows_dev) {
  KgProjArgs a{KgShared(kind, corrupt, ent_dev, ent_rows, rel_dev, rel_rows, src_dev, rel_id_dev, dst_dev, neg_dev, b,
                        k, nullptr, nullptr, g_pos_dev, g_neg_dev, g_src_dev, g_rel_dev, g_dst_dev, g_neg_rows_dev),
               d, ent_aux_dev, rel_aux_dev, g_rel_aux_dev, g_src_aux_dev, g_dst_aux_dev, g_neg_aux_rows_dev};
  bool run;
  const int rc = CheckKgCall(
      {"triple_score_proj_grad", kKgProjFamily, ent_dtype, rel_dtype, d, proj, ent_aux_dev, rel_aux_dev}, a, &run);
  if (proj == kKgProjHyper && (g_src_aux_dev || g_dst_aux_dev || g_neg_aux_rows_dev) && rc == EULER_GPU_OK)
    return Fail(EULER_GPU_EINVAL, "triple_score_proj_grad: proj 1 takes no entity aux gradient buffers");
  if (rc != EULER_GPU_OK || !run) return rc;
  if (!g_pos_dev || !g_src_dev || !g_rel_dev || !g_dst_dev || !g_rel_aux_dev ||
      (k > 0 && (!g_neg_dev || !g_neg_rows_dev)))
    return Fail(EULER_GPU_EINVAL, "triple_score_proj_grad: null gradient buffer");
  if (proj == kKgProjTransfer && (!g_src_aux_dev || !g_dst_aux_dev || (k > 0 && !g_neg_aux_rows_dev)))
    return Fail(EULER_GPU_EINVAL, "triple_score_proj_grad: proj 2 without its entity aux gradient buffers");
  const uintptr_t all = (uintptr_t)g_src_dev | (uintptr_t)g_rel_dev | (uintptr_t)g_dst_dev | (uintptr_t)g_neg_rows_dev |
                        (uintptr_t)g_rel_aux_dev | (uintptr_t)g_src_aux_dev | (uintptr_t)g_dst_aux_dev |
                        (uintptr_t)g_neg_aux_rows_dev;
  if (all % 4 != 0) return Fail(EULER_GPU_EINVAL, "triple_score_proj_grad: a gradient buffer is not aligned to its type");
  a.out_vec = all % 16 == 0;
  return Dispatch((hipStream_t)stream, proj, a, ent_dtype, rel_dtype, true);
}

}  // extern "C"
