// Fused RelationConv (RGCN: tf_euler/python/convolution/relation_conv.py:53-70) on the matrix
// units of gfx950, with its C-ABI entry point: the typed reduce of relation_reduce and the
// per-relation matmul in one pass, without the [size, R, F] block between them.  The contract, the
// work split, the LDS layout and the plan are stated in mp_relation_dense.h; this file is the
// kernel and its dispatch ladder.
//
// THE KERNEL, per group of waves x m runs of 16 destinations: every wave reads the type column of
// its runs once (the set of relations of each destination, n_valid, the set of the run), then
// walks the relations that are present in increasing t.  Per relation and fold tile of 128 k the
// lanes of a run walk their segments in lockstep, predicated on edge_type == t - the indices of a
// batch, then all its row loads, then the adds in increasing p - into 32 fp32 registers, divide
// for the means, narrow, and feed the registers to the MFMAs as A fragments against weight[t] in
// LDS.  RESIDENT instantiations stage all R matrices once and let the waves run free; PHASED ones
// stage one W tile per (relation, fold tile, column tile) between two barriers, for the relations
// some wave of the workgroup has.  The accumulators of a run live across all relations and are
// stored once.  No staging of A, no atomics, no scratch, no host wait: one launch on the
// caller's stream.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mp_dense_frag.h"
#include "mp_relation_dense.h"

namespace euler_gpu {
namespace {

struct RelDenseArgs {
  const void* x;
  const void* weight;       // [R, dim, F]
  MpwIndex ix;              // perm is nullptr: a grouped position is an input position
  const int32_t* type;      // [e]
  const int64_t* seg_ptr; int64_t count, e;
  int32_t f, dim, size, num_relations, mode;
  int32_t wvec;             // weight may be copied in 16-byte loads
  void* out; int32_t out_f32;
  RelDensePlan plan;
};

extern __shared__ __align__(16) unsigned char rel_dense_lds[];

__device__ __forceinline__ uint64_t RelDenseOrXor(uint64_t v, int s) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, s), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s);
  return v | ((uint64_t)hi << 32 | lo);
}

__device__ __forceinline__ uint64_t RelDenseScalar(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (uint64_t)hi << 32 | lo;
}

// columns c0 .. c0 + ncols and k_base .. k_base + k_len (a multiple of 32) of weight[t] into wt in the
// DenseWtByte layout, 16 bytes a step; +0 from dim and from F on
template <int DT>
__device__ __forceinline__ void RelDenseStageW(const RelDenseArgs& a, int32_t t, int32_t c0, int32_t ncols,
                                               int32_t k_base, int32_t k_len, unsigned char* wt) {
  using Elem = std::conditional_t<DT == kF32, uint32_t, uint16_t>;
  constexpr int kPer = 16 / (int)sizeof(Elem);
  const int32_t upc = k_len / kPer, total = ncols * upc;
  const Elem* w = static_cast<const Elem*>(a.weight) + (int64_t)t * a.dim * a.f;
  for (int32_t i = threadIdx.x; i < total; i += blockDim.x) {
    const int32_t cc = i / upc, u = i - cc * upc;
    const int32_t col = c0 + cc, k = k_base + u * kPer;
    DenseWords v = {0u, 0u, 0u, 0u};
    if (col < a.dim && k < a.f) {
      const Elem* p = w + (int64_t)col * a.f + k;
      if (a.wvec) {                       // (F % kPer == 0: a unit that starts inside a row ends inside it)
        v = *reinterpret_cast<const DenseWords*>(p);
      } else if constexpr (DT == kF32) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = k + j < a.f ? p[j] : 0u;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t lo = k + 2 * j < a.f ? p[2 * j] : 0u;
          const uint32_t hi = k + 2 * j + 1 < a.f ? p[2 * j + 1] : 0u;
          v[j] = lo | (hi << 16);
        }
      }
    }
    *reinterpret_cast<DenseWords*>(wt + DenseWtByte(cc, u * 16, a.plan.stride)) = v;
  }
}

template <int DT>
__device__ __forceinline__ void RelDenseStore(const RelDenseArgs& a, int64_t at, float v) {
  if (DT == kF32 || a.out_f32) static_cast<float*>(a.out)[at] = v;
  else if constexpr (DT != kF32) static_cast<uint16_t*>(a.out)[at] = HalfCvt<DT>::Narrow(v);
}

template <int DT, int NT, bool VEC, bool RES>
__global__ __launch_bounds__(64 * kRelDenseWaves, 2) void RelDenseKernel(const RelDenseArgs a) {
  constexpr int M = NT <= 8 ? 2 : 1;
  constexpr int FW = DenseFragWords<DT>();
  constexpr int PB = DenseBatch<DT, VEC>();
  constexpr int kEsz = DT == kF32 ? 4 : 2;
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  unsigned char* wt = rel_dense_lds;
  uint64_t* wave_sets = reinterpret_cast<uint64_t*>(rel_dense_lds);     // (phased: the window, between two groups)
  const int32_t f32k = (a.f + kPoolChunk - 1) / kPoolChunk * kPoolChunk;
  constexpr int32_t kCols = 16 * NT;
  const int32_t stride = a.plan.stride;
  const int32_t mat_bytes = kCols * stride;                     // of a resident matrix
  const int32_t col_tiles = M == 1 ? a.plan.col_tiles : 1;      // (a plan tiles the columns at nt = 16 only)
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kRelDenseWaves * M - 1) / (kRelDenseWaves * M);
  const bool mean = a.mode != kRelAdd;

  if constexpr (RES) {
    for (int32_t t = 0; t < a.num_relations; ++t) RelDenseStageW<DT>(a, t, 0, kCols, 0, f32k, wt + t * mat_bytes);
    __syncthreads();
  }

  for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    // the runs of this wave: per lane its destination's [seg_b, seg_b + len), the relations it has and
    // the destination's denominator; per run the trip count and the relations it has
    int64_t seg_b[M];
    int32_t len[M], trips[M], nr[M];
    uint64_t mine[M], run_set[M];
    float dst_denom[M];
    uint64_t wave_set = 0;
#pragma unroll
    for (int mi = 0; mi < M; ++mi) {
      const int64_t r0 = ((grp * kRelDenseWaves + wave) * M + mi) * kPoolTile;
      nr[mi] = r0 >= a.size ? 0 : (a.size - r0 < kPoolTile ? (int32_t)(a.size - r0) : kPoolTile);
      int64_t sb = 0, se = 0;
      if (c < nr[mi]) TkSegment(a.seg_ptr, a.count, a.e, r0 + c, &sb, &se);
      seg_b[mi] = sb;
      len[mi] = (int32_t)(se - sb);
      if (a.seg_ptr) {
        int32_t mx = len[mi];
#pragma unroll
        for (int s = 1; s < 16; s <<= 1) {
          const int32_t o = __shfl_xor(mx, s);
          mx = o > mx ? o : mx;
        }
        trips[mi] = __builtin_amdgcn_readfirstlane(mx);
      } else {
        trips[mi] = nr[mi] > 0 ? (int32_t)a.count : 0;
      }
      // the type column, once: the four lanes of a destination take every fourth position
      uint64_t set = 0;
      int32_t nv = 0;
      for (int32_t j = g; j < len[mi]; j += 4) {
        const int32_t ty = a.type[sb + j];
        if ((uint32_t)ty < (uint32_t)a.num_relations) {
          set |= 1ull << ty;
          ++nv;
        }
      }
      set = RelDenseOrXor(set, 16);
      set = RelDenseOrXor(set, 32);
      nv += __shfl_xor(nv, 16);
      nv += __shfl_xor(nv, 32);
      mine[mi] = set;
      dst_denom[mi] = MpwAdd((float)nv, 1e-7f);
#pragma unroll
      for (int s = 1; s < 16; s <<= 1) set = RelDenseOrXor(set, s);
      run_set[mi] = RelDenseScalar(set);
      wave_set |= run_set[mi];
    }

    uint64_t todo = wave_set;
    if constexpr (!RES) {                // the relations some wave of the workgroup has
      __syncthreads();                   // (every wave has read the last tile of the group before)
      if (lane == 0) wave_sets[wave] = wave_set;
      __syncthreads();
      todo = 0;
#pragma unroll
      for (int w = 0; w < kRelDenseWaves; ++w) todo |= wave_sets[w];
      todo = RelDenseScalar(todo);
    }

    DenseAcc acc[M][NT];
#pragma unroll
    for (int mi = 0; mi < M; ++mi)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[mi][n] = DenseAcc{0.f, 0.f, 0.f, 0.f};

    while (todo != 0) {
      const int32_t t = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
#pragma unroll 1
      for (int32_t k0 = 0; k0 < f32k; k0 += kDenseFoldTile) {
        const int32_t live = (f32k - k0) / kPoolChunk < kDenseChunks ? (f32k - k0) / kPoolChunk : kDenseChunks;
        DenseWords af[M][kDenseChunks][FW];
#pragma unroll 1
        for (int32_t ct = 0; ct < col_tiles; ++ct) {
          const int32_t c0 = RES ? 0 : ct * a.plan.tile_cols;
          const int32_t ncols = RES ? kCols : (kCols - c0 < a.plan.tile_cols ? kCols - c0 : a.plan.tile_cols);
          if constexpr (!RES) {
            __syncthreads();
            RelDenseStageW<DT>(a, t, c0, ncols, k0, live * kPoolChunk, wt);
            __syncthreads();
          }
          const unsigned char* wb = RES ? wt + t * mat_bytes : wt;
          const int32_t kb0 = RES ? k0 : 0;
#pragma unroll
          for (int mi = 0; mi < M; ++mi) {
            if (((run_set[mi] >> t) & 1) == 0) continue;
            if (ct == 0) {
              // the fold of bucket (r, t) over this tile's k, in input order
              const bool has = (mine[mi] >> t) & 1;
              float fold[kDenseChunks][8];
#pragma unroll
              for (int x = 0; x < kDenseChunks; ++x)
#pragma unroll
                for (int j = 0; j < 8; ++j) fold[x][j] = 0.f;
              int32_t cnt = 0;
#pragma unroll 1
              for (int32_t j0 = 0; j0 < trips[mi]; j0 += PB) {
                int64_t at[PB];
                bool any = false;
#pragma unroll
                for (int y = 0; y < PB; ++y) {
                  const int64_t pos = seg_b[mi] + j0 + y;
                  const bool hit = has && j0 + y < len[mi] && a.type[pos] == t;
                  at[y] = hit ? a.ix.Row(pos) * a.f : -1;
                  cnt += hit;
                  any |= hit;
                }
                if (!__any(any)) continue;
                DenseWords rw[PB][kDenseChunks][FW];
#pragma unroll
                for (int y = 0; y < PB; ++y)
#pragma unroll
                  for (int x = 0; x < kDenseChunks; ++x)
                    DenseLoadA<DT, VEC>(a.x, at[y], k0 + x * kPoolChunk + 8 * g, a.f, rw[y][x]);
#pragma unroll
                for (int y = 0; y < PB; ++y)
#pragma unroll
                  for (int x = 0; x < kDenseChunks; ++x) DenseFoldAdd<DT>(rw[y][x], fold[x], false, 0.f);
              }
              const float denom = a.mode == kRelMeanDst ? dst_denom[mi] : MpwAdd((float)cnt, 1e-7f);
#pragma unroll
              for (int x = 0; x < kDenseChunks; ++x) DenseFragment<DT>(fold[x], mean, denom, af[mi][x]);
            }
#pragma unroll
            for (int x = 0; x < kDenseChunks; ++x) {
              if (x >= live) continue;
              const int32_t kb = (kb0 + x * kPoolChunk + 8 * g) * kEsz;
#pragma unroll
              for (int n = 0; n < NT; ++n) {          // (columns from dim on are +0 in LDS)
                const int32_t cc = 16 * n - c0;
                if (cc < 0 || cc >= ncols) continue;
                DenseWords bw[FW];
#pragma unroll
                for (int q = 0; q < FW; ++q)
                  bw[q] = *reinterpret_cast<const DenseWords*>(wb + DenseWtByte(cc + c, kb + 16 * q, stride));
                acc[mi][n] = DenseMma<DT>(af[mi][x], bw, acc[mi][n]);
              }
            }
          }
        }
      }
    }

    // the store, in the accumulator layout: rows 4 g + i of column c of every fragment
#pragma unroll
    for (int mi = 0; mi < M; ++mi) {
      const int64_t r0 = ((grp * kRelDenseWaves + wave) * M + mi) * kPoolTile;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int32_t col = 16 * n + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int32_t ri = 4 * g + i;
          if (ri < nr[mi] && col < a.dim) RelDenseStore<DT>(a, (r0 + ri) * a.dim + col, acc[mi][n][i]);
        }
      }
    }
  }
}

template <int DT, int NT, bool VEC>
int RelDenseLaunch(hipStream_t st, const RelDenseArgs& a) {
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t per = (int64_t)kRelDenseWaves * a.plan.m;
  const int64_t groups = (runs + per - 1) / per;
  const unsigned blocks = (unsigned)(groups > kRelDenseMaxBlocks ? kRelDenseMaxBlocks : groups);
  if (a.plan.resident)
    hipLaunchKernelGGL((RelDenseKernel<DT, NT, VEC, true>), dim3(blocks), dim3(64 * kRelDenseWaves),
                       (size_t)a.plan.lds_bytes, st, a);
  else
    hipLaunchKernelGGL((RelDenseKernel<DT, NT, VEC, false>), dim3(blocks), dim3(64 * kRelDenseWaves),
                       (size_t)a.plan.lds_bytes, st, a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DT, int NT>
int RelDenseDispatchLoads(hipStream_t st, const RelDenseArgs& a) {
  return PoolVectorLoads(a.f, (uintptr_t)a.x, DT == kF32) ? RelDenseLaunch<DT, NT, true>(st, a)
                                                           : RelDenseLaunch<DT, NT, false>(st, a);
}

template <int DT>
int RelDenseDispatchTile(hipStream_t st, const RelDenseArgs& a) {
  switch (a.plan.nt) {
    case 1: return RelDenseDispatchLoads<DT, 1>(st, a);
    case 2: return RelDenseDispatchLoads<DT, 2>(st, a);
    case 4: return RelDenseDispatchLoads<DT, 4>(st, a);
    case 8: return RelDenseDispatchLoads<DT, 8>(st, a);
    default: return RelDenseDispatchLoads<DT, 16>(st, a);
  }
}

int RelDenseFail(const std::string& why) { return Fail(EULER_GPU_EINVAL, "relation_dense: " + why); }

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" int euler_gpu_relation_dense(void* stream, int32_t mode, const void* x_dev, int32_t dtype, int64_t rows,
                                        const void* gather_dev, int32_t gather_is_ids, const int32_t* edge_type_dev,
                                        int32_t num_relations, const void* weight_dev, const int64_t* seg_ptr_dev,
                                        int64_t count, int64_t e, int64_t f, int64_t dim, int64_t size, void* out_dev,
                                        int32_t out_dtype) {
  if (mode != kRelAdd && mode != kRelMeanDst && mode != kRelMeanRel)
    return RelDenseFail("mode is 0 add, 2 mean over the destination, 3 mean over the bucket");
  if (!KnownDtype(dtype) || !KnownDtype(out_dtype)) return RelDenseFail(std::string("unknown dtype") + kDtypeCodes);
  if (out_dtype != EULER_GPU_F32 && out_dtype != dtype) return RelDenseFail("out is fp32 or of x's dtype");
  if (f < 1 || f > kRelDenseMaxF) return RelDenseFail("F outside 1..256 (kRelDenseMaxF)");
  if (dim < 1 || dim > kRelDenseMaxDim) return RelDenseFail("dim outside 1..256 (kRelDenseMaxDim)");
  if (num_relations < 1 || num_relations > kRelDenseMaxR)
    return RelDenseFail("num_relations outside 1..64 (kRelDenseMaxR)");
  if (size < 0 || e < 0 || count < 0 || rows < 0) return RelDenseFail("size, e, count or rows < 0");
  if (e >= (1LL << 31) || size >= (1LL << 31)) return RelDenseFail("e or size >= 2^31");
  if ((seg_ptr_dev != nullptr) == (count > 0)) return RelDenseFail("exactly one of seg_ptr and count");
  if (!seg_ptr_dev && (count >= (1LL << 31) || e != size * count)) return RelDenseFail("count needs e == size * count");
  if (mode != kRelAdd && (e >= (1LL << 24) || count >= (1LL << 24)))
    return RelDenseFail("a mean needs fewer than 2^24 updates (its counts are exact fp32)");
  if (size == 0) return EULER_GPU_OK;
  if (!weight_dev || !out_dev) return RelDenseFail("null buffer");
  if (e > 0) {
    if (!x_dev || !edge_type_dev) return RelDenseFail("null buffer");
    if (rows < 1 || (gather_dev == nullptr && rows < e)) return RelDenseFail("the table has fewer rows than the updates read");
  }
  const uintptr_t esz = dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)x_dev % esz != 0 || (uintptr_t)weight_dev % esz != 0 ||
      (uintptr_t)out_dev % (out_dtype == EULER_GPU_F32 ? 4 : 2) != 0 || (uintptr_t)seg_ptr_dev % 8 != 0 ||
      (uintptr_t)edge_type_dev % 4 != 0 || (uintptr_t)gather_dev % (gather_is_ids ? 8 : 4) != 0)
    return RelDenseFail("a buffer is not aligned to its type");
  RelDenseArgs a{};
  a.x = x_dev; a.weight = weight_dev;
  // every index is clamped to the table's last row (int64 ids: the low word), as relation_reduce clamps it
  const uint32_t row_max = (uint32_t)std::min<int64_t>(rows > 0 ? rows - 1 : 0, 0x7FFFFFFF);
  a.ix = MpwIndex{nullptr, static_cast<const int32_t*>(gather_dev), gather_is_ids ? 2 : 1, row_max};
  a.type = edge_type_dev;
  a.seg_ptr = seg_ptr_dev; a.count = count; a.e = e;
  a.f = (int32_t)f; a.dim = (int32_t)dim; a.size = (int32_t)size; a.num_relations = num_relations; a.mode = mode;
  a.wvec = PoolVectorLoads(f, (uintptr_t)weight_dev, dtype == EULER_GPU_F32);
  a.out = out_dev; a.out_f32 = out_dtype == EULER_GPU_F32;
  a.plan = RelDenseMakePlan(f, dim, num_relations, dtype == EULER_GPU_F32);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EULER_GPU_F32) return RelDenseDispatchTile<kF32>(st, a);
  if (dtype == EULER_GPU_BF16) return RelDenseDispatchTile<kBF16>(st, a);
  return RelDenseDispatchTile<kF16>(st, a);
}
