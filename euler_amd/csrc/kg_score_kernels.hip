// Fused triple scoring for knowledge-graph embedding (TransE l1 / l2, DistMult) on gfx950 and
// its gradient, with their C-ABI entry points: the lookup of the rows of src, rel, dst and the
// [b, k] negatives, their l2 normalisation and the 1 + K' scores of a triple in one pass - 3 + k
// table rows read and 1 + K' floats written per triple, where the composition from gather and
// element-wise ops builds about a dozen [b, k, d] blocks.  The arithmetic, the range rule and
// the summation order are stated in kg_score.h, which the host check compiles too.
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
#include "kg_lanes.h"
#include "kg_score.h"

namespace euler_gpu {
namespace {

struct KgArgs {
  int32_t kind, normalize, corrupt, log_l;
  const void* ent; int64_t ent_rows;
  const void* rel; int64_t rel_rows;
  const int64_t* src; const int64_t* rel_id; const int64_t* dst; const int64_t* neg;
  int64_t b, k, d;
  float* pos_out; float* neg_out;                 // forward
  const float* g_pos; const float* g_neg;         // gradient
  float* g_src; float* g_rel; float* g_dst; float* g_neg_rows;
  int32_t out_vec;                                // the four gradient buffers start on 16 bytes
};

// ss and inv of a row
template <int V, typename Row>
__device__ __forceinline__ void KgNorm(const Row& x, bool normalize, int32_t l, int32_t lanes, int32_t chunks,
                                       float* ss, float* inv) {
  *ss = normalize ? KgCombine(KgLaneSumSq<V>(x, l, lanes, chunks), lanes) : 0.f;
  *inv = KgInv(*ss, normalize);
}

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
  const int64_t kp = a.corrupt == kKgBoth ? 2 * a.k : a.k;
  for (int64_t t0 = wave * tasks_per_wave; t0 < a.b; t0 += waves * tasks_per_wave) {
    const int64_t t = t0 + sub;
    const bool live = t < a.b;
    LaneRow<DE, V, REG> H, T, N;
    LaneRow<DR, V, REG> R;
    H.Open(a.ent, live ? a.src[t] : -1, a.ent_rows, a.d, l, chunks);
    R.Open(a.rel, live ? a.rel_id[t] : -1, a.rel_rows, a.d, l, chunks);
    T.Open(a.ent, live ? a.dst[t] : -1, a.ent_rows, a.d, l, chunks);
    float ss, ih, ir, it, in;
    KgNorm<V>(H, normalize, l, lanes, chunks, &ss, &ih);
    KgNorm<V>(R, normalize, l, lanes, chunks, &ss, &ir);
    KgNorm<V>(T, normalize, l, lanes, chunks, &ss, &it);
    const float pos = KgFinish(a.kind, KgCombine(KgLaneScore<V>(a.kind, H, ih, R, ir, T, it, l, lanes, chunks), lanes));
    if (live && l == 0) a.pos_out[t] = pos;
    for (int64_t k = 0; k < a.k; ++k) {
      N.Open(a.ent, live ? a.neg[t * a.k + k] : -1, a.ent_rows, a.d, l, chunks);
      KgNorm<V>(N, normalize, l, lanes, chunks, &ss, &in);
      if (a.corrupt != kKgTail) {
        const float s = KgFinish(a.kind, KgCombine(KgLaneScore<V>(a.kind, N, in, R, ir, T, it, l, lanes, chunks), lanes));
        if (live && l == 0) a.neg_out[t * kp + k] = s;
      }
      if (a.corrupt != kKgFront) {
        const float s = KgFinish(a.kind, KgCombine(KgLaneScore<V>(a.kind, H, ih, R, ir, N, in, l, lanes, chunks), lanes));
        if (live && l == 0) a.neg_out[t * kp + (a.corrupt == kKgBoth ? a.k : 0) + k] = s;
      }
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
  const bool l2 = a.kind == kKgTransL2;
  const int64_t kp = a.corrupt == kKgBoth ? 2 * a.k : a.k;
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
    KgNorm<V>(H, normalize, l, lanes, chunks, &ssh, &ih);
    KgNorm<V>(R, normalize, l, lanes, chunks, &ssr, &ir);
    KgNorm<V>(T, normalize, l, lanes, chunks, &sst, &it);
    const LaneOut<V> oh{a.g_src + tt * a.d, live, vec}, orl{a.g_rel + tt * a.d, live, vec},
        ot{a.g_dst + tt * a.d, live, vec};
    LaneAcc<V, REG> gh, gr, gt, gn;
    gh.Open(oh, l, lanes, chunks);
    gr.Open(orl, l, lanes, chunks);
    gt.Open(ot, l, lanes, chunks);
    {
      const float s = l2 ? KgCombine(KgLaneScore<V>(a.kind, H, ih, R, ir, T, it, l, lanes, chunks), lanes) : 0.f;
      const float gs = KgScale(a.kind, live ? a.g_pos[t] : 0.f, s);
      KgLaneScoreGrad<V>(a.kind, gs, H, ih, R, ir, T, it, gh, gr, gt, l, lanes, chunks);
    }
    for (int64_t k = 0; k < a.k; ++k) {
      N.Open(a.ent, live ? a.neg[t * a.k + k] : -1, a.ent_rows, a.d, l, chunks);
      KgNorm<V>(N, normalize, l, lanes, chunks, &ssn, &in);
      const LaneOut<V> on{a.g_neg_rows + (tt * a.k + k) * a.d, live, vec};
      gn.Open(on, l, lanes, chunks);
      if (a.corrupt != kKgTail) {
        const float s = l2 ? KgCombine(KgLaneScore<V>(a.kind, N, in, R, ir, T, it, l, lanes, chunks), lanes) : 0.f;
        const float gs = KgScale(a.kind, live ? a.g_neg[t * kp + k] : 0.f, s);
        KgLaneScoreGrad<V>(a.kind, gs, N, in, R, ir, T, it, gn, gr, gt, l, lanes, chunks);
      }
      if (a.corrupt != kKgFront) {
        const float s = l2 ? KgCombine(KgLaneScore<V>(a.kind, H, ih, R, ir, N, in, l, lanes, chunks), lanes) : 0.f;
        const float gs = KgScale(a.kind, live ? a.g_neg[t * kp + (a.corrupt == kKgBoth ? a.k : 0) + k] : 0.f, s);
        KgLaneScoreGrad<V>(a.kind, gs, H, ih, R, ir, N, in, gh, gr, gn, l, lanes, chunks);
      }
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
  const int64_t chunks = a.d / v;
  a.log_l = KgLogLanes(chunks);
  const bool reg = chunks <= 64;                  // a lane owns at most one chunk
  const int64_t tasks_per_wave = 64 >> a.log_l;
  const int64_t waves = (a.b + tasks_per_wave - 1) / tasks_per_wave;
  int64_t blocks = (waves + 3) / 4;
  if (blocks > 256 * 32) blocks = 256 * 32;
  const dim3 grid((unsigned)blocks);
  if (v == 8) reg ? LaunchOne<DE, DR, 8, true>(st, a, grad, grid) : LaunchOne<DE, DR, 8, false>(st, a, grad, grid);
  else if (v == 4) reg ? LaunchOne<DE, DR, 4, true>(st, a, grad, grid) : LaunchOne<DE, DR, 4, false>(st, a, grad, grid);
  else reg ? LaunchOne<DE, DR, 1, true>(st, a, grad, grid) : LaunchOne<DE, DR, 1, false>(st, a, grad, grid);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DE>
int DispatchRel(hipStream_t st, const KgArgs& a, int32_t rel_dtype, bool grad) {
  if (rel_dtype == EULER_GPU_F32) return LaunchTripleScore<DE, kF32>(st, a, grad);
  if (rel_dtype == EULER_GPU_BF16) return LaunchTripleScore<DE, kBF16>(st, a, grad);
  return LaunchTripleScore<DE, kF16>(st, a, grad);
}

bool KgKnownDtype(int32_t t) { return t == EULER_GPU_F32 || t == EULER_GPU_BF16 || t == EULER_GPU_F16; }

// The checks both entries share.  -> EULER_GPU_OK with *run = false when there is nothing to do.
int CheckTripleArgs(const char* what, const KgArgs& a, int32_t ent_dtype, int32_t rel_dtype, bool* run) {
  *run = false;
  if (a.kind < 0 || a.kind > 2) return Fail(EULER_GPU_EINVAL, std::string(what) + ": kind outside 0..2");
  if (a.corrupt < 0 || a.corrupt > 2) return Fail(EULER_GPU_EINVAL, std::string(what) + ": corrupt outside 0..2");
  if (!KgKnownDtype(ent_dtype) || !KgKnownDtype(rel_dtype))
    return Fail(EULER_GPU_EINVAL, std::string(what) + ": unknown dtype (0 fp32, 1 bf16, 2 fp16)");
  if (a.k < 0 || a.b < 0 || a.d < 0) return Fail(EULER_GPU_EINVAL, std::string(what) + ": b, k or d < 0");
  if (a.ent_rows < 1 || a.rel_rows < 1) return Fail(EULER_GPU_EINVAL, std::string(what) + ": a table with fewer than 1 row");
  if (a.d >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, std::string(what) + ": d >= 2^31");
  if (a.b >= (1LL << 31) || a.k >= (1LL << 31) || a.b * (a.k > 1 ? a.k : 1) * 2 >= (1LL << 31))
    return Fail(EULER_GPU_EINVAL, std::string(what) + ": b * max(k, 1) * 2 >= 2^31");
  if (a.b == 0 || a.d == 0) return EULER_GPU_OK;
  if (!a.ent || !a.rel || !a.src || !a.rel_id || !a.dst) return Fail(EULER_GPU_EINVAL, std::string(what) + ": null buffer");
  if (a.k > 0 && !a.neg) return Fail(EULER_GPU_EINVAL, std::string(what) + ": k > 0 without negatives");
  if ((uintptr_t)a.ent % (ent_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)a.rel % (rel_dtype == EULER_GPU_F32 ? 4 : 2) != 0)
    return Fail(EULER_GPU_EINVAL, std::string(what) + ": a table is not aligned to its type");
  *run = true;
  return EULER_GPU_OK;
}

int DispatchEnt(hipStream_t st, const KgArgs& a, int32_t ent_dtype, int32_t rel_dtype, bool grad) {
  if (ent_dtype == EULER_GPU_F32) return DispatchRel<kF32>(st, a, rel_dtype, grad);
  if (ent_dtype == EULER_GPU_BF16) return DispatchRel<kBF16>(st, a, rel_dtype, grad);
  return DispatchRel<kF16>(st, a, rel_dtype, grad);
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
  KgArgs a{};
  a.kind = kind; a.normalize = normalize; a.corrupt = corrupt;
  a.ent = ent_dev; a.ent_rows = ent_rows; a.rel = rel_dev; a.rel_rows = rel_rows;
  a.src = src_dev; a.rel_id = rel_id_dev; a.dst = dst_dev; a.neg = neg_dev;
  a.b = b; a.k = k; a.d = d;
  a.pos_out = pos_out_dev; a.neg_out = neg_out_dev;
  bool run;
  const int rc = CheckTripleArgs("triple_score", a, ent_dtype, rel_dtype, &run);
  if (rc != EULER_GPU_OK || !run) return rc;
  if (!pos_out_dev || (k > 0 && !neg_out_dev)) return Fail(EULER_GPU_EINVAL, "triple_score: null output buffer");
  return DispatchEnt((hipStream_t)stream, a, ent_dtype, rel_dtype, false);
}

int euler_gpu_triple_score_grad(void* stream, int32_t kind, int32_t normalize, int32_t corrupt,
                                const void* ent_dev, int32_t ent_dtype, int64_t ent_rows,
                                const void* rel_dev, int32_t rel_dtype, int64_t rel_rows,
                                const int64_t* src_dev, const int64_t* rel_id_dev, const int64_t* dst_dev,
                                const int64_t* neg_dev, int64_t b, int64_t k, int64_t d,
                                const float* g_pos_dev, const float* g_neg_dev,
                                float* g_src_dev, float* g_rel_dev, float* g_dst_dev, float* g_neg_rows_dev) {
  KgArgs a{};
  a.kind = kind; a.normalize = normalize; a.corrupt = corrupt;
  a.ent = ent_dev; a.ent_rows = ent_rows; a.rel = rel_dev; a.rel_rows = rel_rows;
  a.src = src_dev; a.rel_id = rel_id_dev; a.dst = dst_dev; a.neg = neg_dev;
  a.b = b; a.k = k; a.d = d;
  a.g_pos = g_pos_dev; a.g_neg = g_neg_dev;
  a.g_src = g_src_dev; a.g_rel = g_rel_dev; a.g_dst = g_dst_dev; a.g_neg_rows = g_neg_rows_dev;
  bool run;
  const int rc = CheckTripleArgs("triple_score_grad", a, ent_dtype, rel_dtype, &run);
  if (rc != EULER_GPU_OK || !run) return rc;
  if (!g_pos_dev || !g_src_dev || !g_rel_dev || !g_dst_dev || (k > 0 && (!g_neg_dev || !g_neg_rows_dev)))
    return Fail(EULER_GPU_EINVAL, "triple_score_grad: null gradient buffer");
  if (((uintptr_t)g_src_dev | (uintptr_t)g_rel_dev | (uintptr_t)g_dst_dev | (uintptr_t)g_neg_rows_dev) % 4 != 0)
    return Fail(EULER_GPU_EINVAL, "triple_score_grad: a gradient buffer is not aligned to its type");
  a.out_vec = ((uintptr_t)g_src_dev | (uintptr_t)g_rel_dev | (uintptr_t)g_dst_dev | (uintptr_t)g_neg_rows_dev) % 16 == 0;
  return DispatchEnt((hipStream_t)stream, a, ent_dtype, rel_dtype, true);
}

}  // extern "C"
