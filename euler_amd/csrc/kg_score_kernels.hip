// Fused triple scoring for knowledge-graph embedding (TransE l1 / l2, DistMult) on gfx950 and
// its gradient, with their C-ABI entry points: the lookup of the rows of src, rel, dst and the
// [b, k] negatives, their l2 normalisation and the 1 + K' scores of a triple in one pass - 3 + k
// table rows read and 1 + K' floats written per triple, where the composition from gather and
// element-wise ops builds about a dozen [b, k, d] blocks.  The arithmetic, the range rule and
// the summation order are stated in kg_score.h, which the host check compiles too.  The argument
// ladder, the dtype fan-out and the launch shape are kg_entry.h's, shared with the two projected
// families; the corruption step of a negative is kg_lanes.h's.
//
// A triple is a task of L lanes of a wave (64 / L triples a wave), as in edge_dot_kernels.hip;
// partial sums stay in registers and are combined inside the wave (__shfl_xor) - no LDS, no
// atomics.  While a lane owns one chunk (d / V <= 64) the rows h, r, t - and in the gradient
// their gy - stay in registers over the k negatives (REG); wider rows are read again from the
// tables, which L2 serves, and gy accumulates in the lane's own columns of the output rows.  The
// order of kg_score.h depends on neither.  Every loop that holds a shuffle has a trip count that
// is the same for all lanes of a wave: a task past the end runs on rows the range rule removed.
#include <hip/hip_runtime.h>

#include "device_fns.h"
#include "device_mem.h"
#include "half_cvt.h"
#include "kg_entry.h"
#include "kg_lanes.h"
#include "kg_score.h"

namespace euler_gpu {
namespace {

struct KgArgs : KgTripleArgs {
  int32_t normalize;
  int64_t d;
};

template <int DE, int DR, int V, bool REG>
__global__ __launch_bounds__(256) void TripleScoreKernel(const KgArgs a) {
  const int32_t lanes = 1 << a.log_l;
  const int32_t lane = threadIdx.x & 63;
  const int32_t sub = lane >> a.log_l, l = lane & (lanes - 1);
  const int64_t tasks_per_wave = 64 >> a.log_l;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int32_t chunks = (int32_t)(a.d / V);
  const bool normalize = a.normalize != 0;
  for (int64_t t0 = wave * tasks_per_wave; t0 < a.b; t0 += waves * tasks_per_wave) {
    const int64_t t = t0 + sub;
    const bool live = t < a.b;
    LaneRow<DE, V, REG> H, T, N;
    LaneRow<DR, V, REG> R;
    H.Open(a.ent, live ? a.src[t] : -1, a.ent_rows, a.d, l, chunks);
    R.Open(a.rel, live ? a.rel_id[t] : -1, a.rel_rows, a.d, l, chunks);
    T.Open(a.ent, live ? a.dst[t] : -1, a.ent_rows, a.d, l, chunks);
    float ss, ih, ir, it, in;
    KgLaneNorm<V>(H, normalize, l, lanes, chunks, &ss, &ih);
    KgLaneNorm<V>(R, normalize, l, lanes, chunks, &ss, &ir);
    KgLaneNorm<V>(T, normalize, l, lanes, chunks, &ss, &it);
    const float pos = KgFinish(a.kind, KgCombine(KgLaneScore<V>(a.kind, H, ih, R, ir, T, it, l, lanes, chunks), lanes));
    if (live && l == 0) a.pos_out[t] = pos;
    for (int64_t k = 0; k < a.k; ++k) {
      N.Open(a.ent, live ? a.neg[t * a.k + k] : -1, a.ent_rows, a.d, l, chunks);
      KgLaneNorm<V>(N, normalize, l, lanes, chunks, &ss, &in);
      KgLaneCorrupt<V>(a.kind, a.corrupt, H, ih, R, ir, T, it, N, in, l, lanes, chunks, [&](bool tail, float s) {
        if (live && l == 0) a.neg_out[KgNegSlot(a.corrupt, a.k, t, k, tail)] = s;
      });
    }
  }
}

// gy -> gx of one row, written to its output row
template <int V, typename Row, typename Acc>
__device__ __forceinline__ void KgRowGrad(const Row& x, bool normalize, float ss, float inv, const Acc& gy,
                                          LaneOut<V> out, int32_t l, int32_t lanes, int32_t chunks) {
  const float dot = normalize ? KgCombine(KgLaneDot<V>(x, inv, gy, l, lanes, chunks), lanes) : 0.f;
  KgLaneRowGrad<V>(x.ok, normalize, x, ss, inv, dot, gy, out, l, lanes, chunks);
}

template <int DE, int DR, int V, bool REG>
__global__ __launch_bounds__(256) void TripleScoreGradKernel(const KgArgs a) {
  const int32_t lanes = 1 << a.log_l;
  const int32_t lane = threadIdx.x & 63;
  const int32_t sub = lane >> a.log_l, l = lane & (lanes - 1);
  const int64_t tasks_per_wave = 64 >> a.log_l;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int32_t chunks = (int32_t)(a.d / V);
  const bool normalize = a.normalize != 0, vec = a.out_vec != 0;
  for (int64_t t0 = wave * tasks_per_wave; t0 < a.b; t0 += waves * tasks_per_wave) {
    const int64_t t = t0 + sub;
    const bool live = t < a.b;
    const int64_t tt = live ? t : 0;
    LaneRow<DE, V, REG> H, T, N;
    LaneRow<DR, V, REG> R;
    H.Open(a.ent, live ? a.src[t] : -1, a.ent_rows, a.d, l, chunks);
    R.Open(a.rel, live ? a.rel_id[t] : -1, a.rel_rows, a.d, l, chunks);
    T.Open(a.ent, live ? a.dst[t] : -1, a.ent_rows, a.d, l, chunks);
    float ssh, ssr, sst, ssn, ih, ir, it, in;
    KgLaneNorm<V>(H, normalize, l, lanes, chunks, &ssh, &ih);
    KgLaneNorm<V>(R, normalize, l, lanes, chunks, &ssr, &ir);
    KgLaneNorm<V>(T, normalize, l, lanes, chunks, &sst, &it);
    const LaneOut<V> oh{a.g_src + tt * a.d, live, vec}, orl{a.g_rel + tt * a.d, live, vec},
        ot{a.g_dst + tt * a.d, live, vec};
    LaneAcc<V, REG> gh, gr, gt, gn;
    gh.Open(oh, l, lanes, chunks);
    gr.Open(orl, l, lanes, chunks);
    gt.Open(ot, l, lanes, chunks);
    {
      const float s =
          a.kind == kKgTransL2 ? KgCombine(KgLaneScore<V>(a.kind, H, ih, R, ir, T, it, l, lanes, chunks), lanes) : 0.f;
      const float gs = KgScale(a.kind, live ? a.g_pos[t] : 0.f, s);
      KgLaneScoreGrad<V>(a.kind, gs, H, ih, R, ir, T, it, gh, gr, gt, l, lanes, chunks);
    }
    for (int64_t k = 0; k < a.k; ++k) {
      N.Open(a.ent, live ? a.neg[t * a.k + k] : -1, a.ent_rows, a.d, l, chunks);
      KgLaneNorm<V>(N, normalize, l, lanes, chunks, &ssn, &in);
      const LaneOut<V> on{a.g_neg_rows + (tt * a.k + k) * a.d, live, vec};
      gn.Open(on, l, lanes, chunks);
      const auto g = [&](bool tail) { return live ? a.g_neg[KgNegSlot(a.corrupt, a.k, t, k, tail)] : 0.f; };
      KgLaneCorruptGrad<V>(a.kind, a.corrupt, g, H, ih, R, ir, T, it, N, in, gh, gr, gt, gn, l, lanes, chunks);
      KgRowGrad<V>(N, normalize, ssn, in, gn, on, l, lanes, chunks);
    }
    KgRowGrad<V>(H, normalize, ssh, ih, gh, oh, l, lanes, chunks);
    KgRowGrad<V>(R, normalize, ssr, ir, gr, orl, l, lanes, chunks);
    KgRowGrad<V>(T, normalize, sst, it, gt, ot, l, lanes, chunks);
  }
}

template <int DE, int DR, int V, bool REG>
void LaunchOne(hipStream_t st, const KgArgs& a, bool grad, dim3 grid) {
  if (grad) hipLaunchKernelGGL((TripleScoreGradKernel<DE, DR, V, REG>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((TripleScoreKernel<DE, DR, V, REG>), grid, dim3(256), 0, st, a);
}

template <int DE, int DR>
int LaunchTripleScore(hipStream_t st, KgArgs a, bool grad) {
  const int32_t v = KgChunkWidth(a.d, (uintptr_t)a.ent, DE == kF32, (uintptr_t)a.rel, DR == kF32);
  const KgLaunchShape shape = KgTaskLaunch(a.b, a.d / v);
  a.log_l = shape.log_l;
  const bool reg = shape.reg;
  const dim3 grid(shape.grid);
  if (v == 8) reg ? LaunchOne<DE, DR, 8, true>(st, a, grad, grid) : LaunchOne<DE, DR, 8, false>(st, a, grad, grid);
  else if (v == 4) reg ? LaunchOne<DE, DR, 4, true>(st, a, grad, grid) : LaunchOne<DE, DR, 4, false>(st, a, grad, grid);
  else reg ? LaunchOne<DE, DR, 1, true>(st, a, grad, grid) : LaunchOne<DE, DR, 1, false>(st, a, grad, grid);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int Dispatch(hipStream_t st, const KgArgs& a, int32_t ent_dtype, int32_t rel_dtype, bool grad) {
  return KgDispatchTables(ent_dtype, rel_dtype,
                          [&](auto de, auto dr) { return LaunchTripleScore<de, dr>(st, a, grad); });
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_triple_score(void* stream, int32_t kind, int32_t normalize, int32_t corrupt,
                           const void* ent_dev, int32_t ent_dtype, int64_t ent_rows,
                           const void* rel_dev, int32_t rel_dtype, int64_t rel_rows,
                           const int64_t* src_dev, const int64_t* rel_id_dev, const int64_t* dst_dev,
                           const int64_t* neg_dev, int64_t b, int64_t k, int64_t d,
                           float* pos_out_dev, float* neg_out_dev) {
  const KgArgs a{KgShared(kind, corrupt, ent_dev, ent_rows, rel_dev, rel_rows, src_dev, rel_id_dev, dst_dev, neg_dev,
                          b, k, pos_out_dev, neg_out_dev),
                 normalize, d};
  bool run;
  const int rc = CheckKgCall({"triple_score", kKgScoreFamily, ent_dtype, rel_dtype, d}, a, &run);
  if (rc != EULER_GPU_OK || !run) return rc;
  if (!pos_out_dev || (k > 0 && !neg_out_dev)) return Fail(EULER_GPU_EINVAL, "triple_score: null output buffer");
  return Dispatch((hipStream_t)stream, a, ent_dtype, rel_dtype, false);
}

int euler_gpu_triple_score_grad(void* stream, int32_t kind, int32_t normalize, int32_t corrupt,
                                const void* ent_dev, int32_t ent_dtype, int64_t ent_rows,
                                const void* rel_dev, int32_t rel_dtype, int64_t rel_rows,
                                const int64_t* src_dev, const int64_t* rel_id_dev, const int64_t* dst_dev,
                                const int64_t* neg_dev, int64_t b, int64_t k, int64_t d,
                                const float* g_pos_dev, const float* g_neg_dev,
                                float* g_src_dev, float* g_rel_dev, float* g_dst_dev, float* g_neg_rows_dev) {
  KgArgs a{KgShared(kind, corrupt, ent_dev, ent_rows, rel_dev, rel_rows, src_dev, rel_id_dev, dst_dev, neg_dev, b, k,
                    nullptr, nullptr, g_pos_dev, g_neg_dev, g_src_dev, g_rel_dev, g_dst_dev, g_neg_rows_dev),
           normalize, d};
  bool run;
  const int rc = CheckKgCall({"triple_score_grad", kKgScoreFamily, ent_dtype, rel_dtype, d}, a, &run);
  if (rc != EULER_GPU_OK || !run) return rc;
  if (!g_pos_dev || !g_src_dev || !g_rel_dev || !g_dst_dev || (k > 0 && (!g_neg_dev || !g_neg_rows_dev)))
    return Fail(EULER_GPU_EINVAL, "triple_score_grad: null gradient buffer");
  const uintptr_t all = (uintptr_t)g_src_dev | (uintptr_t)g_rel_dev | (uintptr_t)g_dst_dev | (uintptr_t)g_neg_rows_dev;
  if (all % 4 != 0) return Fail(EULER_GPU_EINVAL, "triple_score_grad: a gradient buffer is not aligned to its type");
  a.out_vec = all % 16 == 0;
  return Dispatch((hipStream_t)stream, a, ent_dtype, rel_dtype, true);
}

}  // extern "C"
