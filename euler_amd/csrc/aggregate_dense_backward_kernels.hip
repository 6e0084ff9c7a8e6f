// The fused backward of aggregate_dense (MeanAggregator / GCNAggregator: tf_euler/python/utils/
// aggregators.py:25-72; SAGEConv, GraphConv, GINConv) on the matrix units of gfx950, with its C-ABI
// entry point.  The contract, the order of every sum and the three kernels are stated in
// mp_dense_backward.h; the fold, the fragments and the W^T staging are the forward's (mp_dense_frag.h).
// No atomics, no scratch, no host wait: at most seven launches on the caller's stream.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mp_dense_backward.h"
#include "mp_dense_backward_frag.h"
#include "mp_dense_frag.h"

namespace euler_gpu {
namespace {

// ---- kernel 1: A, Zn, Zs as the forward forms them -> the narrowed A, dZn, dZs ---------------------
struct DenseBwdZArgs {
  const void* table; int64_t rows;
  const void* weight;
  const void* bias; int32_t bias_f32;
  const void* gather; int32_t is_ids;
  const int64_t* seg_ptr; int64_t count, e;
  const void* root; const void* root_weight;
  float root_scale; int32_t has_scale;
  int32_t d, ds, f, fs, size, op, combine;
  int32_t need_z;                       // relu: the pre-activations decide; none: dZ is grad narrowed
  const void* grad; int32_t grad_f32;
  void* a_out;                          // [size, d] of the table's dtype, 16-byte aligned | NULL
  void* dzn;                            // [size, f] | NULL
  void* dzs;                            // [size, fs] | NULL
  DensePlan plan;
};

// the 8 elements k .. k + 8 of a finished A fragment to row `at` of a_out; nothing from d on
template <int DT>
__device__ __forceinline__ void DenseBwdStoreA(void* a_out, int64_t at, int32_t k, int32_t d, const DenseWords* w) {
  if constexpr (DT == kF32) {
    uint32_t* p = static_cast<uint32_t*>(a_out) + at;
    if (d % 4 == 0) {
      if (k < d) *reinterpret_cast<DenseWords*>(p + k) = w[0];
      if (k + 4 < d) *reinterpret_cast<DenseWords*>(p + k + 4) = w[1];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (k + j < d) p[k + j] = w[j / 4][j % 4];
    }
  } else {
    uint16_t* p = static_cast<uint16_t*>(a_out) + at;
    if (d % 8 == 0) {
      if (k < d) *reinterpret_cast<DenseWords*>(p + k) = w[0];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (k + j < d) p[k + j] = (uint16_t)(w[0][j / 2] >> (16 * (j % 2)));
    }
  }
}

template <int DT, int NT, bool VEC>
__global__ __launch_bounds__(64 * kDenseWaves, 2) void DenseBwdZKernel(const DenseBwdZArgs a) {
  constexpr int FW = DenseFragWords<DT>();
  constexpr int PB = DenseBatch<DT, VEC>();
  constexpr int kEsz = DT == kF32 ? 4 : 2;
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  const bool self = a.dzs != nullptr && a.need_z, fold_root = a.combine == kDenseFold;
  unsigned char* wt_n = dense_bwd_lds;
  unsigned char* wt_s = dense_bwd_lds + 16 * NT * a.plan.stride_n;
  const int32_t d32 = (a.d + kPoolChunk - 1) / kPoolChunk * kPoolChunk;
  const int32_t s32 = (a.ds + kPoolChunk - 1) / kPoolChunk * kPoolChunk;
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kDenseWaves - 1) / kDenseWaves;
  const bool mean = a.op == kPoolMean;
  const int32_t g_cols = a.combine == kDenseConcat ? a.fs + a.f : a.f;
  const int32_t g_n0 = a.combine == kDenseConcat ? a.fs : 0;

  for (int32_t fp = 0; fp < a.plan.f_passes; ++fp) {
    const int32_t f0 = fp * 16 * NT;
    const bool mma_n = a.need_z && a.dzn && f0 < a.f, mma_s = self && f0 < a.fs;
    const bool fold_n = mma_n || (fp == 0 && a.a_out);
    __syncthreads();
    if (mma_n) DenseStageW<DT, NT>(a.weight, a.d, a.f, f0, 0, d32, a.plan.stride_n, wt_n);
    if (mma_s) DenseStageW<DT, NT>(a.root_weight, a.ds, a.fs, f0, 0, s32, a.plan.stride_s, wt_s);
    __syncthreads();
    float bv[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int32_t col = f0 + 16 * n + c;
      bv[n] = 0.f;
      if (a.bias && col < a.f)
        bv[n] = a.bias_f32 ? static_cast<const float*>(a.bias)[col]
                           : TkWiden<DT>(DT == kF32 ? static_cast<const uint32_t*>(a.bias)[col]
                                                    : (uint32_t)static_cast<const uint16_t*>(a.bias)[col]);
    }

    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
      const int64_t r0 = (grp * kDenseWaves + wave) * kPoolTile;
      const int32_t nr = r0 >= a.size ? 0 : (a.size - r0 < kPoolTile ? (int32_t)(a.size - r0) : kPoolTile);
      if (nr == 0) continue;
      int64_t seg_b = 0, seg_e = 0;
      if (c < nr) TkSegment(a.seg_ptr, a.count, a.e, r0 + c, &seg_b, &seg_e);
      const int32_t len = (int32_t)(seg_e - seg_b);
      int32_t trips;
      if (a.seg_ptr) {
        int32_t m = len;
#pragma unroll
        for (int s = 1; s < 16; s <<= 1) {
          const int32_t o = __shfl_xor(m, s);
          m = o > m ? o : m;
        }
        trips = __builtin_amdgcn_readfirstlane(m);
      } else {
        trips = (int32_t)a.count;
      }
      const int64_t root_at = (a.root && c < nr) ? (r0 + c) * a.ds : -1;
      const float denom = DenseDenominator((int64_t)len + (fold_root ? 1 : 0));

      DenseAcc acc_n[NT], acc_s[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) acc_n[n] = acc_s[n] = DenseAcc{0.f, 0.f, 0.f, 0.f};

      // the neighbour path, fold tile by fold tile: the forward's walk
      if (fold_n) {
#pragma unroll 1
        for (int32_t k0 = 0; k0 < d32; k0 += kDenseFoldTile) {
          const int32_t live = (d32 - k0) / kPoolChunk < kDenseChunks ? (d32 - k0) / kPoolChunk : kDenseChunks;
          float fold[kDenseChunks][8];
#pragma unroll
          for (int x = 0; x < kDenseChunks; ++x)
#pragma unroll
            for (int j = 0; j < 8; ++j) fold[x][j] = 0.f;
          if (fold_root) {
            DenseWords rw[kDenseChunks][FW];
#pragma unroll
            for (int x = 0; x < kDenseChunks; ++x)
              DenseLoadA<DT, VEC>(a.root, root_at, k0 + x * kPoolChunk + 8 * g, a.d, rw[x]);
#pragma unroll
            for (int x = 0; x < kDenseChunks; ++x) DenseFoldAdd<DT>(rw[x], fold[x], a.has_scale != 0, a.root_scale);
          }
#pragma unroll 1
          for (int32_t j0 = 0; j0 < trips; j0 += PB) {
            int64_t at[PB];
#pragma unroll
            for (int y = 0; y < PB; ++y) {
              const int64_t row = j0 + y < len ? TkRow(a.gather, a.is_ids, seg_b + j0 + y, a.rows) : -1;
              at[y] = row < 0 ? -1 : row * a.d;
            }
            DenseWords rw[PB][kDenseChunks][FW];
#pragma unroll
            for (int y = 0; y < PB; ++y)
#pragma unroll
              for (int x = 0; x < kDenseChunks; ++x)
                DenseLoadA<DT, VEC>(a.table, at[y], k0 + x * kPoolChunk + 8 * g, a.d, rw[y][x]);
#pragma unroll
            for (int y = 0; y < PB; ++y)
#pragma unroll
              for (int x = 0; x < kDenseChunks; ++x) DenseFoldAdd<DT>(rw[y][x], fold[x], false, 0.f);
          }
#pragma unroll
          for (int x = 0; x < kDenseChunks; ++x) {
            if (x < live) {
              DenseWords af[FW];
              DenseFragment<DT>(fold[x], mean, denom, af);
              if (fp == 0 && a.a_out && c < nr)
                DenseBwdStoreA<DT>(a.a_out, (r0 + c) * a.d, k0 + x * kPoolChunk + 8 * g, a.d, af);
              if (mma_n)
                DenseChunkMma<DT, NT>(af, wt_n, a.plan.stride_n, (k0 + x * kPoolChunk + 8 * g) * kEsz, c, acc_n);
            }
          }
        }
      }

      // the self path: A fragments straight from the root rows
      if (mma_s) {
#pragma unroll 1
        for (int32_t k0 = 0; k0 < s32; k0 += kDenseFoldTile) {
          const int32_t live = (s32 - k0) / kPoolChunk < kDenseChunks ? (s32 - k0) / kPoolChunk : kDenseChunks;
          DenseWords rw[kDenseChunks][FW];
#pragma unroll
          for (int x = 0; x < kDenseChunks; ++x)
            DenseLoadA<DT, VEC>(a.root, root_at, k0 + x * kPoolChunk + 8 * g, a.ds, rw[x]);
#pragma unroll
          for (int x = 0; x < kDenseChunks; ++x)
            if (x < live)
              DenseChunkMma<DT, NT>(rw[x], wt_s, a.plan.stride_s, (k0 + x * kPoolChunk + 8 * g) * kEsz, c, acc_s);
        }
      }

      // the epilogue, in the accumulator layout: grad under the forward's masks, narrowed once
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int32_t col = f0 + 16 * n + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int32_t ri = 4 * g + i;
          if (ri >= nr) continue;
          const int64_t at = (r0 + ri) * g_cols;
          if (a.dzn && col < a.f) {
            const float gv = DenseBwdGrad<DT>(a.grad, a.grad_f32, at + g_n0 + col);
            const bool on = !a.need_z || MpwAdd(acc_n[n][i], bv[n]) > 0.f;
            DenseBwdPut<DT>(a.dzn, (r0 + ri) * a.f + col, on ? gv : 0.f);
          }
          if (a.dzs && col < a.fs) {
            const float gv = DenseBwdGrad<DT>(a.grad, a.grad_f32, at + col);
            const bool on = !a.need_z || acc_s[n][i] > 0.f;
            DenseBwdPut<DT>(a.dzs, (r0 + ri) * a.fs + col, on ? gv : 0.f);
          }
        }
      }
    }
  }
}

template <int DT, int NT, bool VEC>
int DenseBwdZLaunch(hipStream_t st, const DenseBwdZArgs& a) {
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kDenseWaves - 1) / kDenseWaves;
  const unsigned blocks = (unsigned)(groups > kDenseMaxBlocks ? kDenseMaxBlocks : groups);
  hipLaunchKernelGGL((DenseBwdZKernel<DT, NT, VEC>), dim3(blocks), dim3(64 * kDenseWaves), (size_t)a.plan.lds_bytes, st, a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DT, int NT>
int DenseBwdZLoads(hipStream_t st, const DenseBwdZArgs& a) {
  const bool vec = PoolVectorLoads(a.d, (uintptr_t)a.table, DT == kF32) &&
                   (!a.root || PoolVectorLoads(a.ds, (uintptr_t)a.root, DT == kF32));
  return vec ? DenseBwdZLaunch<DT, NT, true>(st, a) : DenseBwdZLaunch<DT, NT, false>(st, a);
}

template <int DT>
int DenseBwdZ(hipStream_t st, const DenseBwdZArgs& a) {
  switch (a.plan.nt) {
    case 1: return DenseBwdZLoads<DT, 1>(st, a);
    case 2: return DenseBwdZLoads<DT, 2>(st, a);
    case 4: return DenseBwdZLoads<DT, 4>(st, a);
    default: return DenseBwdZLoads<DT, 8>(st, a);
  }
}

// ---- kernels 2 and 3 and the ordered slab sum: mp_dense_backward_frag.h -----------------------------
struct DenseBwdCall {
  DenseBwdZArgs z;
  bool rows_n, rows_s, weight_n, weight_s;
  DenseBwdRowsArgs rn, rs;
  DenseBwdWeightArgs wn, ws;
  void* d_weight; void* d_bias; int32_t bias_dtype; void* d_root_weight; int32_t dtype;
};

template <int DT>
int DenseBwdRun(hipStream_t st, const DenseBwdCall& k) {
  int rc = DenseBwdZ<DT>(st, k.z);
  if (rc == EULER_GPU_OK && k.rows_n) rc = DenseBwdRows<DT>(st, k.rn);
  if (rc == EULER_GPU_OK && k.rows_s) rc = DenseBwdRows<DT>(st, k.rs);
  if (rc == EULER_GPU_OK && k.weight_n) {
    rc = DenseBwdWeight<DT>(st, k.wn);
    const int64_t n = (int64_t)k.wn.kx * k.wn.fy;
    if (rc == EULER_GPU_OK && k.d_weight) rc = DenseBwdSum(st, k.wn.partial, k.wn.slabs, n, k.d_weight, k.dtype);
    if (rc == EULER_GPU_OK && k.d_bias) rc = DenseBwdSum(st, k.wn.bias_partial, k.wn.slabs, k.wn.fy, k.d_bias, k.bias_dtype);
  }
  if (rc == EULER_GPU_OK && k.weight_s) {             // (the workspace is reused: the stream orders the two paths)
    rc = DenseBwdWeight<DT>(st, k.ws);
    if (rc == EULER_GPU_OK)
      rc = DenseBwdSum(st, k.ws.partial, k.ws.slabs, (int64_t)k.ws.kx * k.ws.fy, k.d_root_weight, k.dtype);
  }
  return rc;
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_aggregate_dense_backward(void* stream, int32_t op, int32_t act, int32_t combine, const void* table_dev,
                                       int32_t dtype, int64_t rows, const void* weight_dev, const void* bias_dev,
                                       int32_t bias_dtype, const void* gather_dev, int32_t gather_is_ids,
                                       const int64_t* seg_ptr_dev, int64_t count, int64_t e, int64_t d, int64_t f,
                                       int64_t size, const void* root_dev, const void* root_weight_dev, int64_t ds,
                                       int64_t fs, int32_t has_root_scale, float root_scale, const void* grad_dev,
                                       int32_t grad_dtype, void* a_ws_dev, void* dzn_ws_dev, void* dzs_ws_dev,
                                       float* partial_ws_dev, int64_t partial_ws_floats, float* d_agg_dev,
                                       void* d_weight_dev, void* d_bias_dev, void* d_root_dev, void* d_root_weight_dev) {
  const std::string what("aggregate_dense_backward");
  if (op != kPoolMean && op != kPoolAdd) return Fail(EULER_GPU_EINVAL, what + ": op is 1 mean, 2 add");
  if (act != kPoolRelu && act != kPoolNone) return Fail(EULER_GPU_EINVAL, what + ": activation is 0 relu, 1 none");
  if (combine < kDenseNone || combine > kDenseFold)
    return Fail(EULER_GPU_EINVAL, what + ": combine is 0 none, 1 add, 2 concat, 3 fold");
  if (!KnownDtype(dtype) || !KnownDtype(grad_dtype) || (bias_dev && !KnownDtype(bias_dtype)))
    return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (grad_dtype != EULER_GPU_F32 && grad_dtype != dtype)
    return Fail(EULER_GPU_EINVAL, what + ": grad is fp32 or of the table's dtype");
  if (bias_dev && bias_dtype != EULER_GPU_F32 && bias_dtype != dtype)
    return Fail(EULER_GPU_EINVAL, what + ": bias is fp32 or of the table's dtype");
  if (size < 0 || e < 0 || count < 0) return Fail(EULER_GPU_EINVAL, what + ": size, e or count < 0");
  if (e >= (1LL << 31) || size >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, what + ": e or size >= 2^31");
  if (d < 1 || d > kDenseBwdMaxK || f < 1 || f > kDenseBwdMaxF)
    return Fail(EULER_GPU_EINVAL, what + ": d outside 1..256 (kDenseBwdMaxK) or F outside 1..512 (kDenseBwdMaxF)");
  const bool two = combine == kDenseAdd || combine == kDenseConcat, fold = combine == kDenseFold;
  if (two && (ds < 1 || ds > kDenseBwdMaxK || fs < 1 || fs > kDenseBwdMaxF))
    return Fail(EULER_GPU_EINVAL, what + ": ds outside 1..256 (kDenseBwdMaxK) or Fs outside 1..512 (kDenseBwdMaxF)");
  if (combine == kDenseAdd && fs != f) return Fail(EULER_GPU_EINVAL, what + ": combine add needs Fs == F");
  if (fold && ds != d) return Fail(EULER_GPU_EINVAL, what + ": combine fold needs ds == d");
  if ((seg_ptr_dev != nullptr) == (count > 0))
    return Fail(EULER_GPU_EINVAL, what + ": exactly one of seg_ptr and count");
  if (!seg_ptr_dev && (count >= (1LL << 31) || e != size * count))
    return Fail(EULER_GPU_EINVAL, what + ": count needs e == size * count");
  if (size == 0) return EULER_GPU_OK;
  if (!table_dev || !weight_dev || !grad_dev) return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  if ((combine != kDenseNone) != (root_dev != nullptr) || two != (root_weight_dev != nullptr))
    return Fail(EULER_GPU_EINVAL, what + ": root goes with add, concat and fold, root_weight with add and concat");
  if (rows < 1) return Fail(EULER_GPU_EINVAL, what + ": a table with fewer than 1 row");
  if (d_bias_dev && !bias_dev) return Fail(EULER_GPU_EINVAL, what + ": d_bias without a bias");
  if (d_root_dev && !root_dev) return Fail(EULER_GPU_EINVAL, what + ": d_root without a root");
  if (d_root_weight_dev && !root_weight_dev) return Fail(EULER_GPU_EINVAL, what + ": d_root_weight without a root_weight");
  const bool want_wn = d_weight_dev || d_bias_dev, want_ws = d_root_weight_dev != nullptr;
  const bool want_n = d_agg_dev || want_wn || (fold && d_root_dev);
  const bool want_s = two && (d_root_dev || want_ws);
  if (!want_n && !want_s) return EULER_GPU_OK;
  if ((want_n && !dzn_ws_dev) || (want_s && !dzs_ws_dev) || (want_wn && !a_ws_dev) ||
      ((want_wn || want_ws) && !partial_ws_dev))
    return Fail(EULER_GPU_EINVAL, what + ": a wanted gradient without its workspace");
  if ((want_wn || want_ws) &&
      partial_ws_floats < DenseBwdWorkspaceFloats(size, want_wn ? d : 0, want_wn ? f : 0, want_ws ? ds : 0, want_ws ? fs : 0))
    return Fail(EULER_GPU_EINVAL, what + ": partial_ws holds fewer than DenseBwdWorkspaceFloats fp32");
  const uintptr_t esz = dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)table_dev % esz != 0 || (uintptr_t)weight_dev % esz != 0 || (uintptr_t)root_dev % esz != 0 ||
      (uintptr_t)root_weight_dev % esz != 0 || (uintptr_t)bias_dev % (bias_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)grad_dev % (grad_dtype == EULER_GPU_F32 ? 4 : 2) != 0 || (uintptr_t)seg_ptr_dev % 8 != 0 ||
      (uintptr_t)gather_dev % (gather_is_ids ? 8 : 4) != 0 || (uintptr_t)a_ws_dev % 16 != 0 ||
      (uintptr_t)dzn_ws_dev % esz != 0 || (uintptr_t)dzs_ws_dev % esz != 0 || (uintptr_t)partial_ws_dev % 4 != 0 ||
      (uintptr_t)d_agg_dev % 4 != 0 || (uintptr_t)d_weight_dev % esz != 0 || (uintptr_t)d_root_dev % esz != 0 ||
      (uintptr_t)d_root_weight_dev % esz != 0 || (uintptr_t)d_bias_dev % (bias_dtype == EULER_GPU_F32 ? 4 : 2) != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type (a_ws: to 16 bytes)");
  const bool f32 = dtype == EULER_GPU_F32;
  DenseBwdCall k{};
  DenseBwdZArgs& z = k.z;
  z.table = table_dev; z.rows = rows; z.weight = weight_dev;
  z.bias = bias_dev; z.bias_f32 = bias_dtype == EULER_GPU_F32;
  z.gather = gather_dev; z.is_ids = gather_is_ids != 0;
  z.seg_ptr = seg_ptr_dev; z.count = count; z.e = e;
  z.root = root_dev; z.root_weight = root_weight_dev;
  z.root_scale = root_scale; z.has_scale = fold && has_root_scale != 0;
  z.d = (int32_t)d; z.f = (int32_t)f; z.size = (int32_t)size; z.op = op; z.combine = combine;
  z.ds = combine == kDenseNone ? 0 : (int32_t)ds;
  z.fs = two ? (int32_t)fs : 0;
  z.need_z = act == kPoolRelu;
  z.grad = grad_dev; z.grad_f32 = grad_dtype == EULER_GPU_F32;
  z.a_out = want_wn ? a_ws_dev : nullptr;
  z.dzn = want_n ? dzn_ws_dev : nullptr;
  z.dzs = want_s ? dzs_ws_dev : nullptr;
  z.plan = DenseMakePlan(d, two ? ds : 0, two && fs > f ? fs : f, f32);     // the forward's plan
  if (z.plan.w_tiles != 1) return Fail(EULER_GPU_EINVAL, what + ": the shape needs the forward's K tiling");

  k.rows_n = d_agg_dev || (fold && d_root_dev);
  k.rn.x = dzn_ws_dev; k.rn.w = weight_dev; k.rn.k_all = (int32_t)f; k.rn.n_all = (int32_t)d; k.rn.size = (int32_t)size;
  k.rn.seg_ptr = seg_ptr_dev; k.rn.count = count; k.rn.e = e;
  k.rn.mean = op == kPoolMean; k.rn.extra = fold ? 1 : 0;
  k.rn.out32 = d_agg_dev; k.rn.out_dt = fold ? d_root_dev : nullptr;
  k.rn.scale = root_scale; k.rn.has_scale = z.has_scale;
  k.rn.plan = DenseBwdRowsPlan(f, d, f32);
  k.rows_s = two && d_root_dev;
  k.rs = DenseBwdRowsArgs{};
  k.rs.x = dzs_ws_dev; k.rs.w = root_weight_dev; k.rs.k_all = (int32_t)fs; k.rs.n_all = (int32_t)ds; k.rs.size = (int32_t)size;
  k.rs.out_dt = d_root_dev;
  k.rs.plan = DenseBwdRowsPlan(two ? fs : 1, two ? ds : 1, f32);
  if ((k.rows_n && k.rn.plan.w_tiles != 1) || (k.rows_s && k.rs.plan.w_tiles != 1))
    return Fail(EULER_GPU_EINVAL, what + ": the shape needs a K tiling of W");

  const int64_t slabs = DenseBwdSlabs(size);
  k.weight_n = want_wn;
  k.wn.x = a_ws_dev; k.wn.kx = (int32_t)d; k.wn.vec_x = PoolVectorLoads(d, (uintptr_t)a_ws_dev, f32);
  k.wn.y = dzn_ws_dev; k.wn.fy = (int32_t)f; k.wn.vec_y = PoolVectorLoads(f, (uintptr_t)dzn_ws_dev, f32);
  k.wn.size = (int32_t)size; k.wn.slab_rows = (int32_t)DenseBwdSlabRows(size); k.wn.slabs = (int32_t)slabs;
  k.wn.partial = partial_ws_dev;
  k.wn.bias_partial = d_bias_dev ? partial_ws_dev + slabs * d * f : nullptr;
  k.weight_s = want_ws;
  k.ws = k.wn;
  k.ws.x = root_dev; k.ws.kx = (int32_t)ds; k.ws.vec_x = PoolVectorLoads(ds, (uintptr_t)root_dev, f32);
  k.ws.y = dzs_ws_dev; k.ws.fy = (int32_t)fs; k.ws.vec_y = PoolVectorLoads(fs, (uintptr_t)dzs_ws_dev, f32);
  k.ws.bias_partial = nullptr;
  k.d_weight = d_weight_dev; k.d_bias = d_bias_dev; k.bias_dtype = bias_dtype; k.d_root_weight = d_root_weight_dev;
  k.dtype = dtype;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EULER_GPU_F32) return DenseBwdRun<kF32>(st, k);
  if (dtype == EULER_GPU_BF16) return DenseBwdRun<kBF16>(st, k);
  return DenseBwdRun<kF16>(st, k);
}

}  // extern "C"
