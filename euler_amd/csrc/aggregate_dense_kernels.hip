// Fused mean-aggregator layer (MeanAggregator / GCNAggregator: tf_euler/python/utils/
// aggregators.py:25-72; SAGEConv, GraphConv, GINConv) on the matrix units of gfx950, with its
// C-ABI entry point.  The contract, the tiling, the fragment layouts and the LDS budget are stated
// in mp_dense.h; this file is the kernel and its dispatch ladder.
//
// THE KERNEL, per F-tile pass: the workgroup stages both paths' W^T of the pass in LDS (once,
// unless K is tiled), then every wave takes runs of 16 destinations - group `grp` of four runs
// per workgroup, a grid-stride loop beyond the grid cap.  Lane l reads the [begin, end) of
// destination l % 16; the trip count of the walk is the run's longest segment (the scalar count in
// the count form).  Per fold tile of 128 k: the lane walks its positions in batches - the indices
// of a batch, then all its row loads, then the adds in increasing p - into 32 fp32 registers,
// divides for mean, narrows, and feeds the registers to the MFMAs as A fragments, one B read from
// LDS per chunk and fragment.  The self path's A fragments come straight from root rows.  The
// epilogue applies bias, activation and the combine in the accumulator layout and stores.
// No staging LDS, no atomics, no scratch, no host wait: one launch on the caller's stream.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mp_dense_frag.h"

namespace euler_gpu {
namespace {

struct DenseArgs {
  const void* table; int64_t rows;
  const void* weight;
  const void* bias; int32_t bias_f32;
  const void* gather; int32_t is_ids;
  const int64_t* seg_ptr; int64_t count, e;
  const void* root; const void* root_weight;
  float root_scale; int32_t has_scale;
  int32_t d, ds, f, fs, size, op, act, combine;
  void* out; int32_t out_f32;
  DensePlan plan;
};

template <int DT>
__device__ __forceinline__ void DenseStore(const DenseArgs& a, int64_t at, float v) {
  if (DT == kF32 || a.out_f32) static_cast<float*>(a.out)[at] = v;
  else if constexpr (DT != kF32) static_cast<uint16_t*>(a.out)[at] = HalfCvt<DT>::Narrow(v);
}

extern __shared__ __align__(16) unsigned char dense_lds[];

template <int DT, int NT, bool VEC>
__global__ __launch_bounds__(64 * kDenseWaves, 2) void DenseKernel(const DenseArgs a) {
  constexpr int FW = DenseFragWords<DT>();
  constexpr int PB = DenseBatch<DT, VEC>();
  constexpr int kEsz = DT == kF32 ? 4 : 2;
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  const bool self = a.root_weight != nullptr, fold_root = a.combine == kDenseFold;
  unsigned char* wt_n = dense_lds;
  unsigned char* wt_s = dense_lds + 16 * NT * a.plan.stride_n;
  const int32_t d32 = (a.d + kPoolChunk - 1) / kPoolChunk * kPoolChunk;
  const int32_t s32 = self ? (a.ds + kPoolChunk - 1) / kPoolChunk * kPoolChunk : 0;
  const bool lock = a.plan.w_tiles > 1;
  const int32_t w_tile = a.plan.w_tile;
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kDenseWaves - 1) / kDenseWaves;
  const bool mean = a.op == kPoolMean;
  const int32_t out_cols = a.combine == kDenseConcat ? a.fs + a.f : a.f;
  const int32_t out_n0 = a.combine == kDenseConcat ? a.fs : 0;

  for (int32_t fp = 0; fp < a.plan.f_passes; ++fp) {
    const int32_t f0 = fp * 16 * NT;
    if (!lock) {
      __syncthreads();
      if (f0 < a.f) DenseStageW<DT, NT>(a.weight, a.d, a.f, f0, 0, d32, a.plan.stride_n, wt_n);
      if (self && f0 < a.fs) DenseStageW<DT, NT>(a.root_weight, a.ds, a.fs, f0, 0, s32, a.plan.stride_s, wt_s);
      __syncthreads();
    }
    // the bias of column f0 + 16 n + c, the column this lane holds of fragment n
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
      // this lane's destination: its positions [seg_b, seg_b + len) and its root row
      int64_t seg_b = 0, seg_e = 0;
      if (c < nr) TkSegment(a.seg_ptr, a.count, a.e, r0 + c, &seg_b, &seg_e);
      const int32_t len = (int32_t)(seg_e - seg_b);
      int32_t trips;                              // the run's longest segment, a scalar
      if (a.seg_ptr) {
        int32_t m = len;
#pragma unroll
        for (int s = 1; s < 16; s <<= 1) {
          const int32_t o = __shfl_xor(m, s);
          m = o > m ? o : m;
        }
        trips = __builtin_amdgcn_readfirstlane(m);
      } else {
        trips = nr > 0 ? (int32_t)a.count : 0;
      }
      const int64_t root_at = (a.root && c < nr) ? (r0 + c) * a.ds : -1;
      const float denom = DenseDenominator((int64_t)len + (fold_root ? 1 : 0));

      DenseAcc acc_n[NT], acc_s[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) acc_n[n] = acc_s[n] = DenseAcc{0.f, 0.f, 0.f, 0.f};

      for (int32_t wk = 0; wk < a.plan.w_tiles; ++wk) {
        const int32_t k_base = wk * w_tile;
        if (lock) {
          __syncthreads();
          if (k_base < d32 && f0 < a.f)
            DenseStageW<DT, NT>(a.weight, a.d, a.f, f0, k_base, d32 - k_base < w_tile ? d32 - k_base : w_tile,
                                a.plan.stride_n, wt_n);
          if (k_base < s32 && f0 < a.fs)
            DenseStageW<DT, NT>(a.root_weight, a.ds, a.fs, f0, k_base, s32 - k_base < w_tile ? s32 - k_base : w_tile,
                                a.plan.stride_s, wt_s);
          __syncthreads();
        }
        if (nr == 0) continue;

        // the neighbour path: fold tile by fold tile
        const int32_t n_end = d32 < k_base + w_tile ? d32 : k_base + w_tile;
        if (f0 < a.f) {
#pragma unroll 1
          for (int32_t k0 = k_base; k0 < n_end; k0 += kDenseFoldTile) {
            const int32_t live = (n_end - k0) / kPoolChunk < kDenseChunks ? (n_end - k0) / kPoolChunk : kDenseChunks;
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
                DenseChunkMma<DT, NT>(af, wt_n, a.plan.stride_n, (k0 - k_base + x * kPoolChunk + 8 * g) * kEsz, c, acc_n);
              }
            }
          }
        }

        // the self path: A fragments straight from the root rows
        const int32_t s_end = s32 < k_base + w_tile ? s32 : k_base + w_tile;
        if (self && f0 < a.fs) {
#pragma unroll 1
          for (int32_t k0 = k_base; k0 < s_end; k0 += kDenseFoldTile) {
            const int32_t live = (s_end - k0) / kPoolChunk < kDenseChunks ? (s_end - k0) / kPoolChunk : kDenseChunks;
            DenseWords rw[kDenseChunks][FW];
#pragma unroll
            for (int x = 0; x < kDenseChunks; ++x)
              DenseLoadA<DT, VEC>(a.root, root_at, k0 + x * kPoolChunk + 8 * g, a.ds, rw[x]);
#pragma unroll
            for (int x = 0; x < kDenseChunks; ++x)
              if (x < live)
                DenseChunkMma<DT, NT>(rw[x], wt_s, a.plan.stride_s, (k0 - k_base + x * kPoolChunk + 8 * g) * kEsz, c, acc_s);
          }
        }
      }

      // the epilogue, in the accumulator layout: rows 4 g + i of column c of every fragment
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int32_t col = f0 + 16 * n + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int32_t ri = 4 * g + i;
          if (ri >= nr) continue;
          const int64_t at = (r0 + ri) * out_cols;
          const float vn = PoolAct(a.act, MpwAdd(acc_n[n][i], bv[n]));
          if (a.combine == kDenseConcat) {
            if (col < a.fs) DenseStore<DT>(a, at + col, PoolAct(a.act, acc_s[n][i]));
            if (col < a.f) DenseStore<DT>(a, at + out_n0 + col, vn);
          } else if (col < a.f) {
            DenseStore<DT>(a, at + col, self ? MpwAdd(vn, PoolAct(a.act, acc_s[n][i])) : vn);
          }
        }
      }
    }
  }
}

template <int DT, int NT, bool VEC>
int DenseLaunch(hipStream_t st, const DenseArgs& a) {
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kDenseWaves - 1) / kDenseWaves;
  const unsigned blocks = (unsigned)(groups > kDenseMaxBlocks ? kDenseMaxBlocks : groups);
  hipLaunchKernelGGL((DenseKernel<DT, NT, VEC>), dim3(blocks), dim3(64 * kDenseWaves), (size_t)a.plan.lds_bytes, st, a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DT, int NT>
int DenseDispatchLoads(hipStream_t st, const DenseArgs& a) {
  const bool vec = PoolVectorLoads(a.d, (uintptr_t)a.table, DT == kF32) &&
                   (!a.root || PoolVectorLoads(a.ds, (uintptr_t)a.root, DT == kF32));
  return vec ? DenseLaunch<DT, NT, true>(st, a) : DenseLaunch<DT, NT, false>(st, a);
}

template <int DT>
int DenseDispatchTile(hipStream_t st, const DenseArgs& a) {
  switch (a.plan.nt) {
    case 1: return DenseDispatchLoads<DT, 1>(st, a);
    case 2: return DenseDispatchLoads<DT, 2>(st, a);
    case 4: return DenseDispatchLoads<DT, 4>(st, a);
    default: return DenseDispatchLoads<DT, 8>(st, a);
  }
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_aggregate_dense(void* stream, int32_t op, int32_t act, int32_t combine, const void* table_dev,
                              int32_t dtype, int64_t rows, const void* weight_dev, const void* bias_dev,
                              int32_t bias_dtype, const void* gather_dev, int32_t gather_is_ids,
                              const int64_t* seg_ptr_dev, int64_t count, int64_t e, int64_t d, int64_t f, int64_t size,
                              const void* root_dev, const void* root_weight_dev, int64_t ds, int64_t fs,
                              int32_t has_root_scale, float root_scale, void* out_dev, int32_t out_dtype) {
  const std::string what("aggregate_dense");
  if (op != kPoolMean && op != kPoolAdd) return Fail(EULER_GPU_EINVAL, what + ": op is 1 mean, 2 add");
  if (act != kPoolRelu && act != kPoolNone) return Fail(EULER_GPU_EINVAL, what + ": activation is 0 relu, 1 none");
  if (combine < kDenseNone || combine > kDenseFold)
    return Fail(EULER_GPU_EINVAL, what + ": combine is 0 none, 1 add, 2 concat, 3 fold");
  if (!KnownDtype(dtype) || !KnownDtype(out_dtype) || (bias_dev && !KnownDtype(bias_dtype)))
    return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (out_dtype != EULER_GPU_F32 && out_dtype != dtype)
    return Fail(EULER_GPU_EINVAL, what + ": out is fp32 or of the table's dtype");
  if (bias_dev && bias_dtype != EULER_GPU_F32 && bias_dtype != dtype)
    return Fail(EULER_GPU_EINVAL, what + ": bias is fp32 or of the table's dtype");
  if (size < 0 || e < 0 || count < 0) return Fail(EULER_GPU_EINVAL, what + ": size, e or count < 0");
  if (e >= (1LL << 31) || size >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, what + ": e or size >= 2^31");
  if (d < 1 || d > kDenseMaxK || f < 1 || f > kDenseMaxF)
    return Fail(EULER_GPU_EINVAL, what + ": d outside 1..1024 or F outside 1..4096");
  const bool two = combine == kDenseAdd || combine == kDenseConcat;
  if (two && (ds < 1 || ds > kDenseMaxK || fs < 1 || fs > kDenseMaxF))
    return Fail(EULER_GPU_EINVAL, what + ": ds outside 1..1024 or Fs outside 1..4096");
  if (combine == kDenseAdd && fs != f) return Fail(EULER_GPU_EINVAL, what + ": combine add needs Fs == F");
  if (combine == kDenseFold && ds != d) return Fail(EULER_GPU_EINVAL, what + ": combine fold needs ds == d");
  if ((seg_ptr_dev != nullptr) == (count > 0))
    return Fail(EULER_GPU_EINVAL, what + ": exactly one of seg_ptr and count");
  if (!seg_ptr_dev && (count >= (1LL << 31) || e != size * count))
    return Fail(EULER_GPU_EINVAL, what + ": count needs e == size * count");
  if (size == 0) return EULER_GPU_OK;
  if (!table_dev || !weight_dev || !out_dev) return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  if ((combine != kDenseNone) != (root_dev != nullptr) || two != (root_weight_dev != nullptr))
    return Fail(EULER_GPU_EINVAL, what + ": root goes with add, concat and fold, root_weight with add and concat");
  if (rows < 1) return Fail(EULER_GPU_EINVAL, what + ": a table with fewer than 1 row");
  const uintptr_t esz = dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)table_dev % esz != 0 || (uintptr_t)weight_dev % esz != 0 || (uintptr_t)root_dev % esz != 0 ||
      (uintptr_t)root_weight_dev % esz != 0 || (uintptr_t)bias_dev % (bias_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)out_dev % (out_dtype == EULER_GPU_F32 ? 4 : 2) != 0 || (uintptr_t)seg_ptr_dev % 8 != 0 ||
      (uintptr_t)gather_dev % (gather_is_ids ? 8 : 4) != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  DenseArgs a{};
  a.table = table_dev; a.rows = rows; a.weight = weight_dev;
  a.bias = bias_dev; a.bias_f32 = bias_dtype == EULER_GPU_F32;
  a.gather = gather_dev; a.is_ids = gather_is_ids != 0;
  a.seg_ptr = seg_ptr_dev; a.count = count; a.e = e;
  a.root = root_dev; a.root_weight = root_weight_dev;
  a.root_scale = root_scale; a.has_scale = combine == kDenseFold && has_root_scale != 0;
  a.d = (int32_t)d; a.f = (int32_t)f; a.size = (int32_t)size; a.op = op; a.act = act; a.combine = combine;
  a.ds = combine == kDenseNone ? 0 : (int32_t)ds;
  a.fs = two ? (int32_t)fs : 0;
  a.out = out_dev; a.out_f32 = out_dtype == EULER_GPU_F32;
  a.plan = DenseMakePlan(d, two ? ds : 0, two && fs > f ? fs : f, dtype == EULER_GPU_F32);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EULER_GPU_F32) return DenseDispatchTile<kF32>(st, a);
  if (dtype == EULER_GPU_BF16) return DenseDispatchTile<kBF16>(st, a);
  return DenseDispatchTile<kF16>(st, a);
}

}  // extern "C"
