// The fused supervised loss head (SuperviseModel.__call__ after out_fc, mp_utils/base.py:24-47 of
// the reference, with f1_score / acc_score / auc_score of utils/metrics.py:29-48) on gfx950 and
// its gradient, with their C-ABI entry points: the label fetch, the sigmoid, the sigmoid
// cross-entropy, its mean, the rounded prediction, the tp / fp / fn / correct counts and the two
// AUC histograms in ONE read of the logits and the labels, where the composition runs a dozen
// framework kernels, a [B, C] label block and, for auc, a [T, B * C] comparison.  The arithmetic
// and every order are stated in supervise.h, which the host check compiles too.
//
// A block of 256 lanes owns a tile of R rows (R = 256 while C <= 15, else 64) and walks it in
// chunks of at most 64 columns.  The elements of a chunk are spread over the lanes in storage
// order, so the loads of the logits and labels and the stores of prob and diff are coalesced;
// each lane leaves its term in LDS, and after a barrier lane r adds the terms of row r in the
// order c = 0 .. C - 1, carrying its sum from chunk to chunk: the row sum does not depend on the
// tile or on the grid.  In the graph form lane r first finds the label slot of node r (the
// lookup of DenseFeatureTypedKernel, once per row instead of once per element) and leaves its
// offset and length in LDS.  The counts stay in registers, are added inside the wave with
// integer shuffles and leave the block as one 64-bit integer atomic per counter.  The
// histograms: one 64-bit integer atomic per element straight to memory, or (kSvHistLds) a
// histogram in LDS per block that is added to memory once, bucket by bucket, when the block
// ends.  Integer adds commute: the same bits on every run.  No float atomics.  The total is a
// second launch of one block whose order is a function of B alone.
#include <hip/hip_runtime.h>

#include "device_fns.h"
#include "device_mem.h"
#include "half_cvt.h"
#include "supervise.h"

namespace euler_gpu {
namespace {

#ifndef EULER_GPU_SV_HIST_LDS
#define EULER_GPU_SV_HIST_LDS 1
#endif
constexpr bool kSvHistLds = EULER_GPU_SV_HIST_LDS != 0;

constexpr int kSvBlock = 256;
constexpr int kSvColTile = 64;                     // columns of a chunk
constexpr int kSvTileFloats = 64 * (kSvColTile + 1);   // 64 rows of stride 65, or 256 rows of stride <= 15
constexpr int kSvWideRows = 256, kSvNarrowRows = 64, kSvWideMaxC = 15;
// the carve of the dynamic LDS: terms | slot offsets | slot lengths | per-wave counts | histogram
constexpr int kSvOffBase = kSvTileFloats * 4;
constexpr int kSvOffLen = kSvOffBase + kSvWideRows * 8;
constexpr int kSvOffCnt = kSvOffLen + kSvWideRows * 4;
constexpr int kSvOffHist = kSvOffCnt + 4 * 4 * 4;
constexpr int kSvLdsLimit = 64 * 1024;             // without the dynamic-LDS attribute
static_assert(kSvOffBase % 16 == 0 && kSvOffHist % 16 == 0, "the carve keeps 16-byte offsets");
static_assert(kSvWideRows * kSvWideMaxC <= kSvTileFloats, "the wide tile fits");

enum { kHistNone = 0, kHistGlobal = 1, kHistLds = 2 };

struct SvArgs {
  const void* x; int32_t x_dt;
  const void* z; int32_t z_dt;                      // tensor form, or the graph's table (graph form)
  const uint64_t* nodes; int32_t fid;               // graph form: nodes != nullptr
  int64_t b, c;
  int32_t t;                                        // thresholds
  int32_t rows, stride;                             // R and the LDS stride of a tile row
  float* prob; float* diff; float* row_loss;
  unsigned long long* counts; unsigned long long* hist;
};

__device__ __forceinline__ float SvLoad(const void* p, int32_t dt, int64_t i) {
  if (dt == kF32) return static_cast<const float*>(p)[i];
  const uint16_t h = static_cast<const uint16_t*>(p)[i];
  return dt == kBF16 ? HalfCvt<kBF16>::Widen(h) : HalfCvt<kF16>::Widen(h);
}

__device__ __forceinline__ uint32_t SvWaveSum(uint32_t v) {
  for (int32_t off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int32_t)v, off);
  return v;
}

extern __shared__ __attribute__((aligned(16))) char sv_lds[];

template <int HIST>
__global__ __launch_bounds__(kSvBlock) void SuperviseLossKernel(const SvArgs a, const GraphView g) {
  float* tile = reinterpret_cast<float*>(sv_lds);
  int64_t* slot_at = reinterpret_cast<int64_t*>(sv_lds + kSvOffBase);
  int32_t* slot_len = reinterpret_cast<int32_t*>(sv_lds + kSvOffLen);
  uint32_t* wave_cnt = reinterpret_cast<uint32_t*>(sv_lds + kSvOffCnt);
  uint32_t* lds_hist = reinterpret_cast<uint32_t*>(sv_lds + kSvOffHist);
  const int32_t tid = threadIdx.x;
  const int32_t bins = a.t + 1;
  if constexpr (HIST == kHistLds) {
    for (int32_t i = tid; i < 2 * bins; i += kSvBlock) lds_hist[i] = 0u;
  }
  const bool graph = a.nodes != nullptr;
  uint32_t tp = 0, fp = 0, fn = 0, ok = 0;
  const int64_t tiles = (a.b + a.rows - 1) / a.rows;
  for (int64_t tile_i = blockIdx.x; tile_i < tiles; tile_i += gridDim.x) {
    const int64_t r0 = tile_i * a.rows;
    const int32_t rows = (int32_t)(a.b - r0 < a.rows ? a.b - r0 : a.rows);
    if (graph && tid < rows) {
      int64_t at = 0;
      int32_t len = 0;
      const int64_t row = FindRow(g, a.nodes[r0 + tid]);
      if (row >= 0 && a.fid >= 0 && a.fid < g.n_float) {
        const int32_t* idx = g.feat_idx + (g.feat_uniform ? 0 : row * g.n_float);
        const int32_t pre = a.fid == 0 ? 0 : idx[a.fid - 1];
        len = idx[a.fid] - pre;
        at = (g.feat_uniform ? row * g.feat_stride : g.feat_ptr[row]) + pre;
      }
      slot_at[tid] = at;
      slot_len[tid] = len;
    }
    float sum = 0.f;
    for (int64_t c0 = 0; c0 < a.c; c0 += kSvColTile) {
      const int32_t cols = (int32_t)(a.c - c0 < kSvColTile ? a.c - c0 : kSvColTile);
      __syncthreads();                              // the tile is free; the slots are known
      const int32_t n = rows * cols;
      for (int32_t e = tid; e < n; e += kSvBlock) {
        const int32_t r = e / cols, cc = e - r * cols;
        const int64_t col = c0 + cc;
        const int64_t at = (r0 + r) * a.c + col;
        const float x = SvLoad(a.x, a.x_dt, at);
        float z;
        if (graph) z = col < slot_len[r] ? SvLoad(a.z, a.z_dt, slot_at[r] + col) : 0.f;
        else z = SvLoad(a.z, a.z_dt, at);
        const SvElem el = SvElement(x, z);
        tile[r * a.stride + cc] = el.term;
        if (a.prob) a.prob[at] = el.p;
        if (a.diff) a.diff[at] = el.diff;
        tp += el.label && el.pred;
        fp += !el.label && el.pred;
        fn += el.label && !el.pred;
        ok += el.correct;
        if constexpr (HIST != kHistNone) {
          const int32_t bin = (el.label ? 0 : bins) + SvBucket(el.p, a.t);
          if constexpr (HIST == kHistLds) atomicAdd(&lds_hist[bin], 1u);
          else atomicAdd(&a.hist[bin], 1ull);
        }
      }
      __syncthreads();
      if (tid < rows) {
        const float* mine = tile + tid * a.stride;
        for (int32_t cc = 0; cc < cols; ++cc) sum = SvRowAdd(sum, mine[cc], c0 == 0 && cc == 0);
      }
    }
    if (tid < rows) a.row_loss[r0 + tid] = sum;
  }
  tp = SvWaveSum(tp); fp = SvWaveSum(fp); fn = SvWaveSum(fn); ok = SvWaveSum(ok);
  if ((tid & 63) == 0) {
    uint32_t* mine = wave_cnt + (tid >> 6) * 4;
    mine[0] = tp; mine[1] = fp; mine[2] = fn; mine[3] = ok;
  }
  __syncthreads();
  if (tid < 4) {
    const uint64_t v = (uint64_t)wave_cnt[tid] + wave_cnt[4 + tid] + wave_cnt[8 + tid] + wave_cnt[12 + tid];
    if (v) atomicAdd(&a.counts[tid], (unsigned long long)v);
  } else if (tid == 4 && blockIdx.x == 0) {
    atomicAdd(&a.counts[4], (unsigned long long)(a.b * a.c));
  }
  if constexpr (HIST == kHistLds) {
    for (int32_t i = tid; i < 2 * bins; i += kSvBlock) {
      const uint32_t v = lds_hist[i];
      if (v) atomicAdd(&a.hist[i], (unsigned long long)v);
    }
  }
}

// one block of kSgPartials threads: the total of skipgram.h over the row sums, divided by float(b * c)
__global__ __launch_bounds__(kSgPartials) void SuperviseTotalKernel(const float* row_loss, int64_t b, int64_t c,
                                                                    float* loss) {
  __shared__ float run[kSgPartials / 64];
  const int32_t l = threadIdx.x;
  float s = SgLanePartial(row_loss, l, b);
  for (int32_t off = 32; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off));
  if ((l & 63) == 0) run[l >> 6] = s;
  __syncthreads();
  if (l == 0) *loss = SgFinish(SmxCombine4(run[0], run[1], run[2], run[3]), b, c, 0);
}

__global__ __launch_bounds__(256) void SuperviseLossGradKernel(const float* __restrict__ diff,
                                                               const float* __restrict__ g, int64_t b, int64_t c,
                                                               void* __restrict__ out, int32_t dt) {
  const int64_t n = b * c;
  const float gs = SvScale(g[0], b, c);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float v = SvGrad(gs, diff[i]);
    if (dt == kF32) static_cast<float*>(out)[i] = v;
    else static_cast<uint16_t*>(out)[i] = dt == kBF16 ? HalfCvt<kBF16>::Narrow(v) : HalfCvt<kF16>::Narrow(v);
  }
}

uintptr_t SvElemSize(int32_t t) { return t == EULER_GPU_F32 ? 4 : 2; }

// b and c of both entries
int CheckSuperviseShape(const std::string& w, int64_t b, int64_t c) {
  if (b < 0 || c < 1) return Fail(EULER_GPU_EINVAL, w + ": b < 0 or c < 1");
  if (b >= (1LL << 31) || c >= (1LL << 31) || b * c >= (1LL << 31))
    return Fail(EULER_GPU_EINVAL, w + ": b * c >= 2^31");
  return EULER_GPU_OK;
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_supervise_loss(void* stream, const void* logits_dev, int32_t logits_dtype, int64_t b, int64_t c,
                             const void* labels_dev, int32_t labels_dtype, const euler_gpu_graph* graph,
                             const uint64_t* nodes_dev, int32_t fid, int32_t thresholds, float* prob_dev,
                             float* diff_dev, float* row_loss_dev, float* loss_dev, int64_t* counts_dev,
                             int64_t* hist_dev) {
  const std::string w("supervise_loss");
  const bool tensor_form = labels_dev != nullptr, graph_form = graph != nullptr;
  if (!KnownDtype(logits_dtype) || (tensor_form && !KnownDtype(labels_dtype)))
    return Fail(EULER_GPU_EINVAL, w + ": unknown dtype" + kDtypeCodes);
  const int rs = CheckSuperviseShape(w, b, c);
  if (rs != EULER_GPU_OK) return rs;
  if (hist_dev && thresholds < 2) return Fail(EULER_GPU_EINVAL, w + ": fewer than 2 thresholds");
  // (b == 0: nothing is read, and a tensor without elements has no address)
  if ((tensor_form && graph_form) || (b > 0 && !tensor_form && !graph_form))
    return Fail(EULER_GPU_EINVAL, w + ": the labels are either a tensor or (graph, nodes, fid), one of the two");
  if (!loss_dev || !counts_dev) return Fail(EULER_GPU_EINVAL, w + ": null output buffer");
  if (b > 0 && (!logits_dev || !row_loss_dev || (graph_form && !nodes_dev)))
    return Fail(EULER_GPU_EINVAL, w + ": null buffer");
  if ((uintptr_t)logits_dev % SvElemSize(logits_dtype) != 0 ||
      (tensor_form && (uintptr_t)labels_dev % SvElemSize(labels_dtype) != 0) ||
      ((uintptr_t)prob_dev | (uintptr_t)diff_dev | (uintptr_t)row_loss_dev | (uintptr_t)loss_dev) % 4 != 0 ||
      ((uintptr_t)nodes_dev | (uintptr_t)counts_dev | (uintptr_t)hist_dev) % 8 != 0)
    return Fail(EULER_GPU_EINVAL, w + ": a buffer is not aligned to its type");
  hipStream_t st = (hipStream_t)stream;
  if (b > 0) {
    SvArgs a{};
    a.x = logits_dev; a.x_dt = logits_dtype;
    a.b = b; a.c = c; a.t = hist_dev ? thresholds : 1;
    a.prob = prob_dev; a.diff = diff_dev; a.row_loss = row_loss_dev;
    a.counts = reinterpret_cast<unsigned long long*>(counts_dev);
    a.hist = reinterpret_cast<unsigned long long*>(hist_dev);
    GraphView view{};
    if (graph_form) {
      view = graph->view;
      a.nodes = nodes_dev; a.fid = fid;
      a.z_dt = graph->feat_dtype;
      a.z = graph->feat_dtype == EULER_GPU_F32 ? static_cast<const void*>(view.feat_val) : graph->feat16;
      if (!a.z || !view.feat_idx) view.n_float = 0;   // a graph without dense features: every label is 0
    } else {
      a.z = labels_dev; a.z_dt = labels_dtype;
    }
    const bool wide = c <= kSvWideMaxC;
    a.rows = wide ? kSvWideRows : kSvNarrowRows;
    a.stride = wide ? ((int32_t)c | 1) : kSvColTile + 1;   // odd: lane r's reads spread over the banks
    const int64_t tiles = (b + a.rows - 1) / a.rows;
    const int64_t hist_bytes = 2 * ((int64_t)thresholds + 1) * 4;
    const int mode = !hist_dev ? kHistNone
                     : (kSvHistLds && kSvOffHist + hist_bytes <= kSvLdsLimit) ? kHistLds : kHistGlobal;
    // a block that keeps a histogram in LDS adds it to memory once: fewer, longer-lived blocks
    const int64_t cap = mode == kHistLds ? 512 : 4096;
    const dim3 grid((unsigned)(tiles < cap ? tiles : cap));
    if (mode == kHistLds)
      hipLaunchKernelGGL(SuperviseLossKernel<kHistLds>, grid, dim3(kSvBlock), (size_t)(kSvOffHist + hist_bytes), st,
                         a, view);
    else if (mode == kHistGlobal)
      hipLaunchKernelGGL(SuperviseLossKernel<kHistGlobal>, grid, dim3(kSvBlock), (size_t)kSvOffHist, st, a, view);
    else
      hipLaunchKernelGGL(SuperviseLossKernel<kHistNone>, grid, dim3(kSvBlock), (size_t)kSvOffHist, st, a, view);
    EG_HIP(hipGetLastError());
  }
  // b == 0: the loss alone, +0
  hipLaunchKernelGGL(SuperviseTotalKernel, dim3(1), dim3(kSgPartials), 0, st, row_loss_dev, b, c, loss_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_supervise_loss_grad(void* stream, const float* diff_dev, const float* g_dev, int64_t b, int64_t c,
                                  void* g_logits_dev, int32_t logits_dtype) {
  const std::string w("supervise_loss_grad");
  if (!KnownDtype(logits_dtype)) return Fail(EULER_GPU_EINVAL, w + ": unknown dtype" + kDtypeCodes);
  const int rs = CheckSuperviseShape(w, b, c);
  if (rs != EULER_GPU_OK) return rs;
  if (b == 0) return EULER_GPU_OK;
  if (!diff_dev || !g_dev || !g_logits_dev) return Fail(EULER_GPU_EINVAL, w + ": null buffer");
  if (((uintptr_t)diff_dev | (uintptr_t)g_dev) % 4 != 0 || (uintptr_t)g_logits_dev % SvElemSize(logits_dtype) != 0)
    return Fail(EULER_GPU_EINVAL, w + ": a buffer is not aligned to its type");
  hipLaunchKernelGGL(SuperviseLossGradKernel, dim3(GridFor(b * c, 256)), dim3(256), 0, (hipStream_t)stream, diff_dev,
                     g_dev, b, c, g_logits_dev, logits_dtype);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

}  // extern "C"
