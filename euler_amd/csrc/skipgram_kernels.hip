// The fused skip-gram loss head (DeepWalk / node2vec / LINE / unsupervised GraphSAGE:
// solution/base_unsupervise.py of the reference) on gfx950 and its gradient, with their C-ABI
// entry points: the lookup of target[src] and of the P + K context rows, the P + K logits, the
// sigmoid cross-entropy of the row and the rank of the last positive in one pass - 1 + P + K
// table rows read once each and P + K + 2 words written per pair row, where the composition
// builds [B, 1 + K, d] blocks, two batched matmuls and two top_k sorts.  The arithmetic, the
// range rule and every order are stated in skipgram.h, which the host check compiles too.
//
// A pair row is a task of L lanes of a wave (64 / L rows a wave), as a triple is in
// kg_score_kernels.hip; the partial dot products stay in registers and are combined inside the
// wave (__shfl_xor) - no atomics.  While a lane owns one chunk (d / V <= 64) the target row - and
// in the gradient G_src - stays in registers over the context rows (REG); a wider target row is
// read again, which L2 serves, and G_src accumulates in the lane's own columns of its output
// row.  The last positive's logit is taken first, because the rank compares with it; the row sum
// still adds the terms in the order j = 0 .. P + K - 1.  Every loop that holds a shuffle has a
// trip count that is the same for all lanes of a wave: a task past the end runs on rows the
// range rule removed.  The total is a second launch of one block: its order is a function of B.
#include <hip/hip_runtime.h>

#include "device_fns.h"
#include "device_mem.h"
#include "half_cvt.h"
#include "kg_lanes.h"
#include "skipgram.h"

namespace euler_gpu {
namespace {

struct SgArgs {
  int32_t log_l, out_vec;                         // out_vec: the gradient buffers start on 16 bytes
  const void* target; int64_t target_rows;
  const void* context; int64_t context_rows;
  const int64_t* src; const int64_t* pos; const int64_t* neg;
  int64_t b, p, k, d;
  float* logits; int32_t* rank; float* row_loss; float* loss;     // forward
  const float* saved; const float* g;                             // gradient
  float* g_src; float* g_pos; float* g_neg;
};

// the id of context row j of live pair row t
__device__ __forceinline__ int64_t SgContextId(const SgArgs& a, int64_t t, int64_t j) {
  return j < a.p ? a.pos[t * a.p + j] : a.neg[t * a.k + (j - a.p)];
}

template <int DT, int DC, int V, bool REG>
__global__ __launch_bounds__(256) void SkipgramLossKernel(const SgArgs a) {
  const int32_t lanes = 1 << a.log_l;
  const int32_t lane = threadIdx.x & 63;
  const int32_t sub = lane >> a.log_l, l = lane & (lanes - 1);
  const int64_t tasks_per_wave = 64 >> a.log_l;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int32_t chunks = (int32_t)(a.d / V);
  const int64_t n = a.p + a.k;
  for (int64_t t0 = wave * tasks_per_wave; t0 < a.b; t0 += waves * tasks_per_wave) {
    const int64_t t = t0 + sub;
    const bool live = t < a.b;
    LaneRow<DT, V, REG> T;
    LaneRow<DC, V, REG> C;
    T.Open(a.target, live ? a.src[t] : -1, a.target_rows, a.d, l, chunks);
    C.Open(a.context, live ? SgContextId(a, t, a.p - 1) : -1, a.context_rows, a.d, l, chunks);
    const float x_last = KgCombine(SgLaneDot<V>(T, C, l, lanes, chunks), lanes);
    SgRowState st;
    st.Start(a.p, x_last);
    for (int64_t j = 0; j < n; ++j) {
      float x = x_last;
      if (j != a.p - 1) {
        C.Open(a.context, live ? SgContextId(a, t, j) : -1, a.context_rows, a.d, l, chunks);
        x = KgCombine(SgLaneDot<V>(T, C, l, lanes, chunks), lanes);
      }
      st.Add(x);
      if (live && l == 0) a.logits[t * n + j] = x;
    }
    if (live && l == 0) {
      a.rank[t] = st.rank;
      a.row_loss[t] = st.sum;
    }
  }
}

// one block of kSgPartials threads: the partial sums, the butterfly inside each wave's run, the four runs
__global__ __launch_bounds__(kSgPartials) void SkipgramTotalKernel(const float* row_loss, int64_t b, int64_t p,
                                                                   int64_t k, float* loss) {
  __shared__ float run[kSgPartials / 64];
  const int32_t l = threadIdx.x;
  float s = SgLanePartial(row_loss, l, b);
  for (int32_t off = 32; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off));
  if ((l & 63) == 0) run[l >> 6] = s;
  __syncthreads();
  if (l == 0) *loss = SgFinish(SmxCombine4(run[0], run[1], run[2], run[3]), b, p, k);
}

template <int DT, int DC, int V, bool REG>
__global__ __launch_bounds__(256) void SkipgramLossGradKernel(const SgArgs a) {
  const int32_t lanes = 1 << a.log_l;
  const int32_t lane = threadIdx.x & 63;
  const int32_t sub = lane >> a.log_l, l = lane & (lanes - 1);
  const int64_t tasks_per_wave = 64 >> a.log_l;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int32_t chunks = (int32_t)(a.d / V);
  const int64_t n = a.p + a.k;
  const bool vec = a.out_vec != 0;
  const float gs = MpwDiv(a.g[0], SgCount(a.b, a.p, a.k));
  for (int64_t t0 = wave * tasks_per_wave; t0 < a.b; t0 += waves * tasks_per_wave) {
    const int64_t t = t0 + sub;
    if (t >= a.b) continue;                       // (no shuffle below)
    LaneRow<DT, V, REG> T;
    LaneRow<DC, V, REG> C;
    T.Open(a.target, a.src[t], a.target_rows, a.d, l, chunks);
    const LaneOut<V> os{a.g_src + t * a.d, true, vec};
    LaneAcc<V, REG> acc;
    acc.Open(os, l, lanes, chunks);
    for (int64_t j = 0; j < n; ++j) {
      C.Open(a.context, SgContextId(a, t, j), a.context_rows, a.d, l, chunks);
      const float c = SgCoef(gs, a.saved[t * n + j], j < a.p);
      float* row = j < a.p ? a.g_pos + (t * a.p + j) * a.d : a.g_neg + (t * a.k + (j - a.p)) * a.d;
      LaneOut<V> oc{row, true, vec};
      SgLaneGrad<V>(c, C.ok, T, C, acc, oc, l, lanes, chunks);
    }
    LaneOut<V> out = os;
    SgLaneSrcGrad<V>(T.ok, acc, out, l, lanes, chunks);
  }
}

template <int DT, int DC, int V, bool REG>
void LaunchOne(hipStream_t st, const SgArgs& a, bool grad, dim3 grid) {
  if (grad) hipLaunchKernelGGL((SkipgramLossGradKernel<DT, DC, V, REG>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((SkipgramLossKernel<DT, DC, V, REG>), grid, dim3(256), 0, st, a);
}

template <int DT, int DC>
int LaunchSkipgram(hipStream_t st, SgArgs a, bool grad) {
  const int32_t v = KgChunkWidth(a.d, (uintptr_t)a.target, DT == kF32, (uintptr_t)a.context, DC == kF32);
  const int64_t chunks = a.d / v;
  a.log_l = KgLogLanes(chunks);
  const bool reg = chunks <= 64;                  // a lane owns at most one chunk
  const int64_t tasks_per_wave = 64 >> a.log_l;
  const int64_t waves = (a.b + tasks_per_wave - 1) / tasks_per_wave;
  int64_t blocks = (waves + 3) / 4;
  if (blocks > 256 * 32) blocks = 256 * 32;
  const dim3 grid((unsigned)blocks);
  if (v == 8) reg ? LaunchOne<DT, DC, 8, true>(st, a, grad, grid) : LaunchOne<DT, DC, 8, false>(st, a, grad, grid);
  else if (v == 4) reg ? LaunchOne<DT, DC, 4, true>(st, a, grad, grid) : LaunchOne<DT, DC, 4, false>(st, a, grad, grid);
  else reg ? LaunchOne<DT, DC, 1, true>(st, a, grad, grid) : LaunchOne<DT, DC, 1, false>(st, a, grad, grid);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DT>
int DispatchContext(hipStream_t st, const SgArgs& a, int32_t context_dtype, bool grad) {
  if (context_dtype == EULER_GPU_F32) return LaunchSkipgram<DT, kF32>(st, a, grad);
  if (context_dtype == EULER_GPU_BF16) return LaunchSkipgram<DT, kBF16>(st, a, grad);
  return LaunchSkipgram<DT, kF16>(st, a, grad);
}

int DispatchTarget(hipStream_t st, const SgArgs& a, int32_t target_dtype, int32_t context_dtype, bool grad) {
  if (target_dtype == EULER_GPU_F32) return DispatchContext<kF32>(st, a, context_dtype, grad);
  if (target_dtype == EULER_GPU_BF16) return DispatchContext<kBF16>(st, a, context_dtype, grad);
  return DispatchContext<kF16>(st, a, context_dtype, grad);
}

// The checks both entries share.  -> EULER_GPU_OK with *run = false when b == 0.
int CheckSkipgramArgs(const char* what, const SgArgs& a, int32_t target_dtype, int32_t context_dtype, bool* run) {
  *run = false;
  const std::string w(what);
  if (!KnownDtype(target_dtype) || !KnownDtype(context_dtype))
    return Fail(EULER_GPU_EINVAL, w + ": unknown dtype" + kDtypeCodes);
  if (a.b < 0 || a.k < 0) return Fail(EULER_GPU_EINVAL, w + ": b or k < 0");
  if (a.p < 1 || a.d < 1) return Fail(EULER_GPU_EINVAL, w + ": p < 1 or d < 1");
  if (a.target_rows < 1 || a.context_rows < 1) return Fail(EULER_GPU_EINVAL, w + ": a table with fewer than 1 row");
  if (a.target_rows >= (1LL << 31) || a.context_rows >= (1LL << 31))
    return Fail(EULER_GPU_EINVAL, w + ": a table of 2^31 rows or more");
  if (a.d >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, w + ": d >= 2^31");
  if (a.b >= (1LL << 31) || a.p >= (1LL << 31) || a.k >= (1LL << 31) || a.b * (a.p + a.k) >= (1LL << 31))
    return Fail(EULER_GPU_EINVAL, w + ": b * (p + k) >= 2^31");
  if (a.b == 0) return EULER_GPU_OK;
  if (!a.target || !a.context || !a.src || !a.pos) return Fail(EULER_GPU_EINVAL, w + ": null buffer");
  if (a.k > 0 && !a.neg) return Fail(EULER_GPU_EINVAL, w + ": k > 0 without negatives");
  if ((uintptr_t)a.target % (target_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)a.context % (context_dtype == EULER_GPU_F32 ? 4 : 2) != 0)
    return Fail(EULER_GPU_EINVAL, w + ": a table is not aligned to its type");
  *run = true;
  return EULER_GPU_OK;
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_skipgram_loss(void* stream, const void* target_dev, int32_t target_dtype, int64_t target_rows,
                            const void* context_dev, int32_t context_dtype, int64_t context_rows,
                            const int64_t* src_dev, const int64_t* pos_dev, const int64_t* neg_dev,
                            int64_t b, int64_t p, int64_t k, int64_t d,
                            float* logits_dev, int32_t* rank_dev, float* row_loss_dev, float* loss_dev) {
  SgArgs a{};
  a.target = target_dev; a.target_rows = target_rows; a.context = context_dev; a.context_rows = context_rows;
  a.src = src_dev; a.pos = pos_dev; a.neg = neg_dev;
  a.b = b; a.p = p; a.k = k; a.d = d;
  a.logits = logits_dev; a.rank = rank_dev; a.row_loss = row_loss_dev; a.loss = loss_dev;
  bool run;
  const int rc = CheckSkipgramArgs("skipgram_loss", a, target_dtype, context_dtype, &run);
  if (rc != EULER_GPU_OK) return rc;
  if (!loss_dev || (run && (!logits_dev || !rank_dev || !row_loss_dev)))
    return Fail(EULER_GPU_EINVAL, "skipgram_loss: null output buffer");
  if (((uintptr_t)logits_dev | (uintptr_t)rank_dev | (uintptr_t)row_loss_dev | (uintptr_t)loss_dev) % 4 != 0)
    return Fail(EULER_GPU_EINVAL, "skipgram_loss: an output buffer is not aligned to its type");
  hipStream_t st = (hipStream_t)stream;
  if (run) {
    const int rl = DispatchTarget(st, a, target_dtype, context_dtype, false);
    if (rl != EULER_GPU_OK) return rl;
  }
  // b == 0: the loss alone, +0
  hipLaunchKernelGGL(SkipgramTotalKernel, dim3(1), dim3(kSgPartials), 0, st, row_loss_dev, b, p, k, loss_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_skipgram_loss_grad(void* stream, const void* target_dev, int32_t target_dtype, int64_t target_rows,
                                 const void* context_dev, int32_t context_dtype, int64_t context_rows,
                                 const int64_t* src_dev, const int64_t* pos_dev, const int64_t* neg_dev,
                                 int64_t b, int64_t p, int64_t k, int64_t d,
                                 const float* logits_dev, const float* g_dev,
                                 float* g_src_dev, float* g_pos_dev, float* g_neg_dev) {
  SgArgs a{};
  a.target = target_dev; a.target_rows = target_rows; a.context = context_dev; a.context_rows = context_rows;
  a.src = src_dev; a.pos = pos_dev; a.neg = neg_dev;
  a.b = b; a.p = p; a.k = k; a.d = d;
  a.saved = logits_dev; a.g = g_dev;
  a.g_src = g_src_dev; a.g_pos = g_pos_dev; a.g_neg = g_neg_dev;
  bool run;
  const int rc = CheckSkipgramArgs("skipgram_loss_grad", a, target_dtype, context_dtype, &run);
  if (rc != EULER_GPU_OK || !run) return rc;
  if (!logits_dev || !g_dev || !g_src_dev || !g_pos_dev || (k > 0 && !g_neg_dev))
    return Fail(EULER_GPU_EINVAL, "skipgram_loss_grad: null gradient buffer");
  const uintptr_t all = (uintptr_t)logits_dev | (uintptr_t)g_dev | (uintptr_t)g_src_dev | (uintptr_t)g_pos_dev |
                        (uintptr_t)g_neg_dev;
  if (all % 4 != 0) return Fail(EULER_GPU_EINVAL, "skipgram_loss_grad: a gradient buffer is not aligned to its type");
  a.out_vec = ((uintptr_t)g_src_dev | (uintptr_t)g_pos_dev | (uintptr_t)g_neg_dev) % 16 == 0;
  return DispatchTarget((hipStream_t)stream, a, target_dtype, context_dtype, true);
}

}  // extern "C"
