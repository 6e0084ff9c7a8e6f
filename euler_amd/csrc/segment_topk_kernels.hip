// Fused per-column top-k over the gathered rows of a segment (LGCN: LGCEncoder of the reference,
// tf_euler/python/utils/encoders.py:911-914) on gfx950 and the helper of its gradient, with their
// C-ABI entry points.  The semantics - segment forms, range rule, order, fill, storage - and the
// sticky-shift insertion are stated in mp_topk.h, which the host check compiles too.
//
// FORWARD.  One lane owns (destination r, a chunk of V adjacent columns); adjacent lanes take
// adjacent chunks, so the lanes of a wave read a row with 16-byte loads side by side.  The lane
// walks its segment in order and keeps V lists of K slots - values, and positions only when sel
// is wanted - in registers: K is a template capacity (1, 2, 4, 8, 16; k is rounded up and only k
// entries are stored), every slot loop is fully unrolled and no array is indexed at run time.  V
// follows the rule of TkChunkWidth: 8 / 4 / 1 by d % V and the alignment of params, out and sel,
// lowered until the slots fit 64 registers.  The candidates are taken NB at a time: the NB index
// loads first, then the NB row loads, then the NB insertions in position order, so the latencies
// of a batch overlap while the order of mp_topk.h holds.  An index the range rule removes loads
// row 0 - which exists - and its words are masked to +0: the row it names is never dereferenced.
// No LDS, no atomics, no host wait; everything is enqueued on the caller's stream.
//
// GRADIENT.  per_edge [e, d] is set to +0 (one fill) and every selected position receives its
// element of grad: per_edge[sel[r][j][c]][c] = grad[r][j][c].  A candidate is selected at most
// once per column, so every element has one writer at most.
#include <hip/hip_runtime.h>

#include "device_fns.h"
#include "device_mem.h"
#include "mp_topk.h"

namespace euler_gpu {
namespace {

constexpr int kTkBytes[3] = {4, 2, 2};

// the 32-bit words that hold V adjacent elements
template <int DT, int V>
constexpr int TkWords() { return DT == kF32 ? V : (V == 1 ? 1 : V / 2); }

template <int DT, int V>
__device__ __forceinline__ void TkLoad(const void* base, int64_t at, uint32_t* w) {
  if constexpr (DT == kF32) {
    const uint32_t* p = static_cast<const uint32_t*>(base) + at;
    if constexpr (V == 1) {
      w[0] = *p;
    } else {
#pragma unroll
      for (int q = 0; q < V / 4; ++q) {
        const uint4 v = reinterpret_cast<const uint4*>(p)[q];
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
      }
    }
  } else {
    const uint16_t* p = static_cast<const uint16_t*>(base) + at;
    if constexpr (V == 1) {
      w[0] = *p;
    } else if constexpr (V == 4) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      w[0] = v.x; w[1] = v.y;
    } else {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
  }
}

// element k of the words of a chunk, widened
template <int DT, int V>
__device__ __forceinline__ float TkElem(const uint32_t* w, int k) {
  if constexpr (DT == kF32 || V == 1) return TkWiden<DT>(w[k]);
  else return TkWiden<DT>((k & 1) ? w[k / 2] >> 16 : w[k / 2] & 0xffffu);
}

// V adjacent elements, each the bits of one element in a uint32, as 4-byte (F32) or 2-byte items
template <bool F32, int V>
__device__ __forceinline__ void TkStore(void* base, int64_t at, const uint32_t* r) {
  if constexpr (F32) {
    uint32_t* p = static_cast<uint32_t*>(base) + at;
    if constexpr (V == 1) {
      *p = r[0];
    } else {
#pragma unroll
      for (int q = 0; q < V / 4; ++q)
        reinterpret_cast<uint4*>(p)[q] = make_uint4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
    }
  } else {
    uint16_t* p = static_cast<uint16_t*>(base) + at;
    if constexpr (V == 1) {
      *p = (uint16_t)r[0];
    } else if constexpr (V == 4) {
      *reinterpret_cast<uint2*>(p) = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
    } else {
      *reinterpret_cast<uint4*>(p) =
          make_uint4(r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16));
    }
  }
}

struct TkArgs {
  const void* params; int64_t rows;
  const void* gather; int32_t is_ids;
  const int64_t* seg_ptr; int64_t count, e, d;
  int32_t size, k;
  float fill;
  void* out; int32_t out_f32;
  int32_t* sel;
};

template <int DT, int V, int K, bool SEL>
__global__ __launch_bounds__(256) void TkKernel(const TkArgs a) {
  constexpr int NB = K <= 4 ? 8 : 4;
  constexpr int W = TkWords<DT, V>();
  const int64_t chunks = a.d / V, total = (int64_t)a.size * chunks;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool out_f32 = DT == kF32 || a.out_f32 != 0;
  const uint32_t fill = TkStored<DT>(a.fill, out_f32);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t r = t / chunks, c0 = (t - r * chunks) * V;
    int64_t b, en;
    TkSegment(a.seg_ptr, a.count, a.e, r, &b, &en);
    float slot[V][K];
    int32_t pos[V][SEL ? K : 1];
#pragma unroll
    for (int k = 0; k < V; ++k) {
#pragma unroll
      for (int j = 0; j < K; ++j) slot[k][j] = 0.f;
#pragma unroll
      for (int j = 0; j < (SEL ? K : 1); ++j) pos[k][j] = -1;
    }
    int32_t seen = 0;
    for (int64_t q = b; q < en; q += NB) {
      bool ok[NB];
      int64_t row[NB];
      uint32_t raw[NB][W];
#pragma unroll
      for (int x = 0; x < NB; ++x) {
        ok[x] = q + x < en;
        row[x] = TkRow(a.gather, a.is_ids, ok[x] ? q + x : b, a.rows);
      }
#pragma unroll
      for (int x = 0; x < NB; ++x) TkLoad<DT, V>(a.params, (row[x] < 0 ? 0 : row[x]) * a.d + c0, raw[x]);
#pragma unroll
      for (int x = 0; x < NB; ++x) {
        const uint32_t keep = row[x] < 0 ? 0u : ~0u;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          uint32_t w[W];
#pragma unroll
          for (int i = 0; i < W; ++i) w[i] = raw[x][i] & keep;
          TkInsert<K, SEL>(ok[x], TkElem<DT, V>(w, k), (int32_t)(q + x), seen, slot[k], pos[k]);
        }
        seen += ok[x] ? 1 : 0;
      }
    }
    // the first k entries; entry j of a segment shorter than j + 1 is the fill
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (j < a.k) {
        const int64_t at = ((int64_t)r * a.k + j) * a.d + c0;
        uint32_t o[V];
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = j < seen ? TkStored<DT>(slot[k][j], out_f32) : fill;
        if (out_f32) TkStore<true, V>(a.out, at, o);
        else TkStore<false, V>(a.out, at, o);
        if constexpr (SEL) {
#pragma unroll
          for (int k = 0; k < V; ++k) o[k] = (uint32_t)(j < seen ? pos[k][j] : -1);
          TkStore<true, V>(a.sel, at, o);
        }
      }
    }
  }
}

int64_t TkBlocks(int64_t lanes) {
  const int64_t blocks = (lanes + 255) / 256;
  return blocks > (1 << 20) ? (1 << 20) : blocks;
}

template <int DT, int V, int K, bool SEL>
int TkLaunch(hipStream_t st, const TkArgs& a) {
  if constexpr (!TkFits(V, K, SEL)) {
    return Fail(EULER_GPU_EINVAL, "gather_segment_topk: no kernel for this chunk width");   // (TkChunkWidth never asks)
  } else {
    const int64_t lanes = (int64_t)a.size * (a.d / V);
    hipLaunchKernelGGL((TkKernel<DT, V, K, SEL>), dim3((unsigned)TkBlocks(lanes)), dim3(256), 0, st, a);
    EG_HIP(hipGetLastError());
    return EULER_GPU_OK;
  }
}

template <int DT, int V, int K>
int TkDispatchSel(hipStream_t st, const TkArgs& a) {
  return a.sel ? TkLaunch<DT, V, K, true>(st, a) : TkLaunch<DT, V, K, false>(st, a);
}

template <int DT, int V>
int TkDispatchK(hipStream_t st, const TkArgs& a, int32_t cap) {
  switch (cap) {
    case 1: return TkDispatchSel<DT, V, 1>(st, a);
    case 2: return TkDispatchSel<DT, V, 2>(st, a);
    case 4: return TkDispatchSel<DT, V, 4>(st, a);
    case 8: return TkDispatchSel<DT, V, 8>(st, a);
    default: return TkDispatchSel<DT, V, 16>(st, a);
  }
}

template <int DT>
int TkDispatchV(hipStream_t st, const TkArgs& a) {
  const int32_t cap = TkCapacity(a.k);
  const int32_t v = TkChunkWidth(a.d, (uintptr_t)a.params, DT == kF32, (uintptr_t)a.out, DT == kF32 || a.out_f32,
                                 (uintptr_t)a.sel, cap);
  if (v == 8) return TkDispatchK<DT, 8>(st, a, cap);
  if (v == 4) return TkDispatchK<DT, 4>(st, a, cap);
  return TkDispatchK<DT, 1>(st, a, cap);
}

template <int DT>
__global__ __launch_bounds__(256) void TkGradKernel(const void* __restrict__ grad, const int32_t* __restrict__ sel,
                                                    int64_t n, int64_t d, int64_t e, float* __restrict__ per_edge) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t s = sel[i];
    if (s < 0 || s >= e) continue;
    const int64_t c = n < (1LL << 32) ? (int64_t)((uint32_t)i % (uint32_t)d) : i % d;
    uint32_t raw;
    if constexpr (DT == kF32) raw = static_cast<const uint32_t*>(grad)[i];
    else raw = static_cast<const uint16_t*>(grad)[i];
    per_edge[s * d + c] = TkWiden<DT>(raw);
  }
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_gather_segment_topk(void* stream, const void* params_dev, int32_t in_dtype, int64_t params_rows,
                                  const void* gather_dev, int32_t gather_is_ids, const int64_t* seg_ptr_dev,
                                  int64_t count, int64_t e, int64_t d, int32_t size, int32_t k, float fill,
                                  void* out_dev, int32_t out_dtype, int32_t* sel_dev) {
  const std::string what("gather_segment_topk");
  if (k < 1 || k > kTkMaxK) return Fail(EULER_GPU_EINVAL, what + ": k outside 1..16");
  if (!KnownDtype(in_dtype) || !KnownDtype(out_dtype))
    return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (out_dtype != EULER_GPU_F32 && out_dtype != in_dtype)
    return Fail(EULER_GPU_EINVAL, what + ": out is fp32 or of the input's dtype");
  if (size < 0 || e < 0 || d < 0 || count < 0) return Fail(EULER_GPU_EINVAL, what + ": size, e, d or count < 0");
  if (e >= (1LL << 31) || d >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, what + ": e or d >= 2^31");
  if ((seg_ptr_dev != nullptr) == (count > 0))
    return Fail(EULER_GPU_EINVAL, what + ": exactly one of seg_ptr and count");
  if (!seg_ptr_dev && e != (int64_t)size * count) return Fail(EULER_GPU_EINVAL, what + ": count needs e == size * count");
  if (size == 0 || d == 0) return EULER_GPU_OK;
  if (!params_dev || !out_dev) return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  if (params_rows < 1) return Fail(EULER_GPU_EINVAL, what + ": a table with fewer than 1 row");
  if ((uintptr_t)params_dev % kTkBytes[in_dtype] != 0 || (uintptr_t)out_dev % kTkBytes[out_dtype] != 0 ||
      (uintptr_t)sel_dev % 4 != 0 || (uintptr_t)seg_ptr_dev % 8 != 0 ||
      (uintptr_t)gather_dev % (gather_is_ids ? 8 : 4) != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  TkArgs a{};
  a.params = params_dev; a.rows = params_rows; a.gather = gather_dev; a.is_ids = gather_is_ids != 0;
  a.seg_ptr = seg_ptr_dev; a.count = count; a.e = e; a.d = d; a.size = size; a.k = k; a.fill = fill;
  a.out = out_dev; a.out_f32 = out_dtype == EULER_GPU_F32; a.sel = sel_dev;
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == EULER_GPU_F32) return TkDispatchV<kF32>(st, a);
  if (in_dtype == EULER_GPU_BF16) return TkDispatchV<kBF16>(st, a);
  return TkDispatchV<kF16>(st, a);
}

int euler_gpu_segment_topk_grad(void* stream, const void* grad_dev, int32_t grad_dtype, const int32_t* sel_dev,
                                int64_t e, int64_t d, int32_t size, int32_t k, float* per_edge_dev) {
  const std::string what("segment_topk_grad");
  if (k < 1 || k > kTkMaxK) return Fail(EULER_GPU_EINVAL, what + ": k outside 1..16");
  if (!KnownDtype(grad_dtype)) return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (size < 0 || e < 0 || d < 0) return Fail(EULER_GPU_EINVAL, what + ": size, e or d < 0");
  if (e >= (1LL << 31) || d >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, what + ": e or d >= 2^31");
  if (e == 0 || d == 0) return EULER_GPU_OK;
  if (!per_edge_dev || (size > 0 && (!grad_dev || !sel_dev))) return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  if ((uintptr_t)grad_dev % kTkBytes[grad_dtype] != 0 || (uintptr_t)sel_dev % 4 != 0 || (uintptr_t)per_edge_dev % 4 != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  hipStream_t st = (hipStream_t)stream;
  EG_HIP(hipMemsetAsync(per_edge_dev, 0, (size_t)e * (size_t)d * 4, st));
  if (size == 0) return EULER_GPU_OK;
  const int64_t n = (int64_t)size * k * d;
  const dim3 grid((unsigned)TkBlocks(n)), block(256);
  if (grad_dtype == EULER_GPU_F32)
    hipLaunchKernelGGL(TkGradKernel<kF32>, grid, block, 0, st, grad_dev, sel_dev, n, d, e, per_edge_dev);
  else if (grad_dtype == EULER_GPU_BF16)
    hipLaunchKernelGGL(TkGradKernel<kBF16>, grid, block, 0, st, grad_dev, sel_dev, n, d, e, per_edge_dev);
  else
    hipLaunchKernelGGL(TkGradKernel<kF16>, grid, block, 0, st, grad_dev, sel_dev, n, d, e, per_edge_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

}  // extern "C"
