// Fused triple scoring with the TransH ("hyperplane") and TransD ("transfer") projections on
// gfx950 and its gradient, with their C-ABI entry points: the lookups of the one or two extra
// tables, the projection of every entity row (one dot product and one axpy a row), TransD's
// second normalisation and the 1 + K' scores of a triple in one pass, where the composition
// tiles the hyperplane / transfer rows over the k negatives and builds [b, k, d] blocks again.
// The arithmetic, the range rule and the order are stated in kg_proj.h and kg_score.h, which the
// host check compiles too.
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
#include "kg_lanes.h"
#include "kg_proj.h"

namespace euler_gpu {
namespace {

struct KgProjArgs {
  int32_t kind, corrupt, log_l;
  const void* ent; const void* ent_aux; int64_t ent_rows;
  const void* rel; const void* rel_aux; int64_t rel_rows;
  const int64_t* src; const int64_t* rel_id; const int64_t* dst; const int64_t* neg;
  int64_t b, k, d;
  float* pos_out; float* neg_out;                 // forward
  const float* g_pos; const float* g_neg;         // gradient
  float* g_src; float* g_rel; float* g_dst; float* g_neg_rows;
  float* g_rel_aux; float* g_src_aux; float* g_dst_aux; float* g_neg_aux_rows;
  int32_t out_vec;                                // every gradient buffer starts on 16 bytes
};

// ss and inv of a normalised row
template <int V, typename Row>
__device__ __forceinline__ void KgProjNorm(const Row& x, int32_t l, int32_t lanes, int32_t chunks, float* ss,
                                           float* inv) {
  *ss = KgCombine(KgLaneSumSq<V>(x, l, lanes, chunks), lanes);
  *inv = KgInv(*ss, true);
}

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
      KgProjNorm<V>(z, l, lanes, chunks, &ss, &inv);
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
  const int64_t kp = a.corrupt == kKgBoth ? 2 * a.k : a.k;
  for (int64_t t0 = wave * tasks_per_wave; t0 < a.b; t0 += waves * tasks_per_wave) {
    const int64_t t = t0 + sub;
    const bool live = t < a.b;
    const int64_t rid = live ? a.rel_id[t] : -1;
    LaneRow<DR, V, REG> R, W;
    R.Open(a.rel, rid, a.rel_rows, a.d, l, chunks);
    W.Open(a.rel_aux, rid, a.rel_rows, a.d, l, chunks);
    float ss, ir, iw = 1.f;
    KgProjNorm<V>(R, l, lanes, chunks, &ss, &ir);
    if constexpr (PROJ == kKgProjHyper) KgProjNorm<V>(W, l, lanes, chunks, &ss, &iw);
    ProjEnt<PROJ, DE, V, REG> H, T, N;
    H.Open(a, live ? a.src[t] : -1, W, iw, l, lanes, chunks);
    T.Open(a, live ? a.dst[t] : -1, W, iw, l, lanes, chunks);
    const auto hv = H.View(W, iw), tv = T.View(W, iw);
    const float pos = KgFinish(a.kind, KgCombine(KgLaneScore<V>(a.kind, hv, H.inv, R, ir, tv, T.inv, l, lanes, chunks), lanes));
    if (live && l == 0) a.pos_out[t] = pos;
    for (int64_t k = 0; k < a.k; ++k) {
      N.Open(a, live ? a.neg[t * a.k + k] : -1, W, iw, l, lanes, chunks);
      const auto nv = N.View(W, iw);
      if (a.corrupt != kKgTail) {
        const float s = KgFinish(a.kind, KgCombine(KgLaneScore<V>(a.kind, nv, N.inv, R, ir, tv, T.inv, l, lanes, chunks), lanes));
        if (live && l == 0) a.neg_out[t * kp + k] = s;
      }
      if (a.corrupt != kKgFront) {
        const float s = KgFinish(a.kind, KgCombine(KgLaneScore<V>(a.kind, hv, H.inv, R, ir, nv, N.inv, l, lanes, chunks), lanes));
        if (live && l == 0) a.neg_out[t * kp + (a.corrupt == kKgBoth ? a.k : 0) + k] = s;
      }
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
  const bool l2 = a.kind == kKgTransL2;
  constexpr bool kAux = PROJ == kKgProjTransfer;  // the entity tables' aux gradient rows exist
  const int64_t kp = a.corrupt == kKgBoth ? 2 * a.k : a.k;
  for (int64_t t0 = wave * tasks_per_wave; t0 < a.b; t0 += waves * tasks_per_wave) {
    const int64_t t = t0 + sub;
    const bool live = t < a.b;
    const int64_t tt = live ? t : 0;
    const int64_t rid = live ? a.rel_id[t] : -1;
    LaneRow<DR, V, REG> R, W;
    R.Open(a.rel, rid, a.rel_rows, a.d, l, chunks);
    W.Open(a.rel_aux, rid, a.rel_rows, a.d, l, chunks);
    float ssr, ssw = 0.f, ir, iw = 1.f;
    KgProjNorm<V>(R, l, lanes, chunks, &ssr, &ir);
    if constexpr (PROJ == kKgProjHyper) KgProjNorm<V>(W, l, lanes, chunks, &ssw, &iw);
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
      const float s = l2 ? KgCombine(KgLaneScore<V>(a.kind, hv, H.inv, R, ir, tv, T.inv, l, lanes, chunks), lanes) : 0.f;
      const float gs = KgScale(a.kind, live ? a.g_pos[t] : 0.f, s);
      KgLaneScoreGrad<V>(a.kind, gs, hv, H.inv, R, ir, tv, T.inv, gh, gr, gt, l, lanes, chunks);
    }
    for (int64_t k = 0; k < a.k; ++k) {
      N.Open(a, live ? a.neg[t * a.k + k] : -1, W, iw, l, lanes, chunks);
      const auto nv = N.View(W, iw);
      const LaneOut<V> on{a.g_neg_rows + (tt * a.k + k) * a.d, live, vec},
          ona{kAux ? a.g_neg_aux_rows + (tt * a.k + k) * a.d : nullptr, live && kAux, vec};
      gn.Open(on, l, lanes, chunks);
      if (a.corrupt != kKgTail) {
        const float s = l2 ? KgCombine(KgLaneScore<V>(a.kind, nv, N.inv, R, ir, tv, T.inv, l, lanes, chunks), lanes) : 0.f;
        const float gs = KgScale(a.kind, live ? a.g_neg[t * kp + k] : 0.f, s);
        KgLaneScoreGrad<V>(a.kind, gs, nv, N.inv, R, ir, tv, T.inv, gn, gr, gt, l, lanes, chunks);
      }
      if (a.corrupt != kKgFront) {
        const float s = l2 ? KgCombine(KgLaneScore<V>(a.kind, hv, H.inv, R, ir, nv, N.inv, l, lanes, chunks), lanes) : 0.f;
        const float gs = KgScale(a.kind, live ? a.g_neg[t * kp + (a.corrupt == kKgBoth ? a.k : 0) + k] : 0.f, s);
        KgLaneScoreGrad<V>(a.kind, gs, hv, H.inv, R, ir, nv, N.inv, gh, gr, gn, l, lanes, chunks);
      }
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
  const int64_t chunks = a.d / v;
  a.log_l = KgLogLanes(chunks);
  const bool reg = chunks <= 64;                  // a lane owns at most one chunk
  const int64_t tasks_per_wave = 64 >> a.log_l;
  const int64_t waves = (a.b + tasks_per_wave - 1) / tasks_per_wave;
  int64_t blocks = (waves + 3) / 4;
  if (blocks > 256 * 32) blocks = 256 * 32;
  const dim3 grid((unsigned)blocks);
  if (v == 8) LaunchForm<PROJ, DE, DR, 8>(st, a, grad, grid, reg);
  else if (v == 4) LaunchForm<PROJ, DE, DR, 4>(st, a, grad, grid, reg);
  else LaunchForm<PROJ, DE, DR, 1>(st, a, grad, grid, reg);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int PROJ, int DE>
int DispatchRel(hipStream_t st, const KgProjArgs& a, int32_t rel_dtype, bool grad) {
  if (rel_dtype == EULER_GPU_F32) return LaunchProj<PROJ, DE, kF32>(st, a, grad);
  if (rel_dtype == EULER_GPU_BF16) return LaunchProj<PROJ, DE, kBF16>(st, a, grad);
  return LaunchProj<PROJ, DE, kF16>(st, a, grad);
}

template <int PROJ>
int DispatchEnt(hipStream_t st, const KgProjArgs& a, int32_t ent_dtype, int32_t rel_dtype, bool grad) {
  if (ent_dtype == EULER_GPU_F32) return DispatchRel<PROJ, kF32>(st, a, rel_dtype, grad);
  if (ent_dtype == EULER_GPU_BF16) return DispatchRel<PROJ, kBF16>(st, a, rel_dtype, grad);
  return DispatchRel<PROJ, kF16>(st, a, rel_dtype, grad);
}

int Dispatch(hipStream_t st, int32_t proj, const KgProjArgs& a, int32_t ent_dtype, int32_t rel_dtype, bool grad) {
  if (proj == kKgProjHyper) return DispatchEnt<kKgProjHyper>(st, a, ent_dtype, rel_dtype, grad);
  return DispatchEnt<kKgProjTransfer>(st, a, ent_dtype, rel_dtype, grad);
}

bool KnownDtype(int32_t t) { return t == EULER_GPU_F32 || t == EULER_GPU_BF16 || t == EULER_GPU_F16; }

// The checks both entries share.  -> EULER_GPU_OK with *run = false when there is nothing to do.
int CheckProjArgs(const char* what, int32_t proj, const KgProjArgs& a, int32_t ent_dtype, int32_t rel_dtype, bool* run) {
  *run = false;
  const std::string w(what);
  if (proj < 1 || proj > 2) return Fail(EULER_GPU_EINVAL, w + ": proj outside 1..2 (1 hyperplane, 2 transfer)");
  if (a.kind < 0 || a.kind > 1) return Fail(EULER_GPU_EINVAL, w + ": kind outside 0..1 (distmult takes no projection)");
  if (a.corrupt < 0 || a.corrupt > 2) return Fail(EULER_GPU_EINVAL, w + ": corrupt outside 0..2");
  if (!KnownDtype(ent_dtype) || !KnownDtype(rel_dtype))
    return Fail(EULER_GPU_EINVAL, w + ": unknown dtype (0 fp32, 1 bf16, 2 fp16)");
  if (a.k < 0 || a.b < 0 || a.d < 0) return Fail(EULER_GPU_EINVAL, w + ": b, k or d < 0");
  if (a.ent_rows < 1 || a.rel_rows < 1) return Fail(EULER_GPU_EINVAL, w + ": a table with fewer than 1 row");
  if (a.d >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, w + ": d >= 2^31");
  if (a.b >= (1LL << 31) || a.k >= (1LL << 31) || a.b * (a.k > 1 ? a.k : 1) * 2 >= (1LL << 31))
    return Fail(EULER_GPU_EINVAL, w + ": b * max(k, 1) * 2 >= 2^31");
  if (proj == kKgProjHyper && a.ent_aux) return Fail(EULER_GPU_EINVAL, w + ": proj 1 takes no ent_aux table");
  if (a.b == 0 || a.d == 0) return EULER_GPU_OK;
  if (!a.ent || !a.rel || !a.src || !a.rel_id || !a.dst) return Fail(EULER_GPU_EINVAL, w + ": null buffer");
  if (!a.rel_aux || (proj == kKgProjTransfer && !a.ent_aux))
    return Fail(EULER_GPU_EINVAL, w + ": a missing aux table (proj 1: hyper; proj 2: ent_transfer and rel_transfer)");
  if (a.k > 0 && !a.neg) return Fail(EULER_GPU_EINVAL, w + ": k > 0 without negatives");
  const uintptr_t ea = ent_dtype == EULER_GPU_F32 ? 4 : 2, ra = rel_dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)a.ent % ea != 0 || (uintptr_t)a.ent_aux % ea != 0 || (uintptr_t)a.rel % ra != 0 ||
      (uintptr_t)a.rel_aux % ra != 0)
    return Fail(EULER_GPU_EINVAL, w + ": a table is not aligned to its type");
  *run = true;
  return EULER_GPU_OK;
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
  KgProjArgs a{};
  a.kind = kind; a.corrupt = corrupt;
  a.ent = ent_dev; a.ent_aux = ent_aux_dev; a.ent_rows = ent_rows;
  a.rel = rel_dev; a.rel_aux = rel_aux_dev; a.rel_rows = rel_rows;
  a.src = src_dev; a.rel_id = rel_id_dev; a.dst = dst_dev; a.neg = neg_dev;
  a.b = b; a.k = k; a.d = d;
  a.pos_out = pos_out_dev; a.neg_out = neg_out_dev;
  bool run;
  const int rc = CheckProjArgs("triple_score_proj", proj, a, ent_dtype, rel_dtype, &run);
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
  KgProjArgs a{};
  a.kind = kind; a.corrupt = corrupt;
  a.ent = ent_dev; a.ent_aux = ent_aux_dev; a.ent_rows = ent_rows;
  a.rel = rel_dev; a.rel_aux = rel_aux_dev; a.rel_rows = rel_rows;
  a.src = src_dev; a.rel_id = rel_id_dev; a.dst = dst_dev; a.neg = neg_dev;
  a.b = b; a.k = k; a.d = d;
  a.g_pos = g_pos_dev; a.g_neg = g_neg_dev;
  a.g_src = g_src_dev; a.g_rel = g_rel_dev; a.g_dst = g_dst_dev; a.g_neg_rows = g_neg_rows_dev;
  a.g_rel_aux = g_rel_aux_dev; a.g_src_aux = g_src_aux_dev; a.g_dst_aux = g_dst_aux_dev;
  a.g_neg_aux_rows = g_neg_aux_rows_dev;
  bool run;
  const int rc = CheckProjArgs("triple_score_proj_grad", proj, a, ent_dtype, rel_dtype, &run);
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
