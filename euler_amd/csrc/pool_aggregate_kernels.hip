// Fused pooling aggregation (GraphSAGE meanpool / maxpool: tf_euler/python/utils/aggregators.py:
// 75-114) on the matrix units of gfx950, with its C-ABI entry point.  The contract, the tiling, the
// fragment layouts and the LDS budget are stated in mp_pool.h; this file is the kernel and its
// dispatch ladder.
//
// THE KERNEL, per F-tile pass: the workgroup stages W^T of the pass in LDS (once, unless K is
// tiled), then every wave takes runs of 16 destinations - group `grp` of four runs per workgroup,
// a grid-stride loop beyond the grid cap.  For a run, lanes 0..16 read its 17 segment boundaries
// and a prefix max makes them non-decreasing; the wave then walks the run's positions in tiles of
// 16.  Per tile: the index of position p0 + l % 16 (that of the NEXT tile is requested before the
// matrix work of this one), then per batch of 4 K chunks the A fragments straight from global
// memory - all loads of a batch before its first MFMA - and per chunk and fragment one B read from
// LDS and one MFMA (fp32: eight).  The epilogue writes 64 columns of the accumulators to the
// wave's staging rows, lane l walks column l down the rows in increasing p - bias, activation,
// fold - and stores a destination when the walk passes its end.  Running values live in registers
// across tiles, so a segment may span any number of tiles.  Only LDS a wave owns is touched
// between its own writes and reads, so a wave-level fence orders them; __syncthreads appears only
// around the staging of W^T.
// No atomics, no scratch, no host wait: one launch on the caller's stream.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mp_pool.h"
#include "mp_pool_frag.h"

namespace euler_gpu {
namespace {

struct PoolArgs {
  const void* table; int64_t rows;
  const void* weight;
  const void* bias; int32_t bias_f32;
  const void* gather; int32_t is_ids;
  const int64_t* seg_ptr; int64_t count, e;
  int32_t d, f, size, op, act;
  void* out; int32_t out_f32;
  PoolPlan plan;
};

template <int DT>
__device__ __forceinline__ void PoolStore(const PoolArgs& a, int64_t r, int32_t col, float v) {
  if (col >= a.f) return;
  const int64_t at = r * a.f + col;
  if (DT == kF32 || a.out_f32) static_cast<float*>(a.out)[at] = v;
  else if constexpr (DT != kF32) static_cast<uint16_t*>(a.out)[at] = HalfCvt<DT>::Narrow(v);
}

template <int DT, int NT, bool VEC>
__global__ __launch_bounds__(64 * kPoolWaves, 3) void PoolKernel(const PoolArgs a) {
  constexpr int FW = PoolFragWords<DT>();
  constexpr int NH = (NT + 3) / 4;                // halves of 64 columns the fold takes in turn
  constexpr int kEsz = DT == kF32 ? 4 : 2;
  __shared__ int32_t s_tiles[kPoolWaves];
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  float* stage = reinterpret_cast<float*>(pool_lds) + wave * kPoolTile * kPoolStageStride;
  unsigned char* wt = pool_lds + kPoolStageBytes;
  const int32_t d32 = (a.d + kPoolChunk - 1) / kPoolChunk * kPoolChunk;
  const bool multi_k = a.plan.k_tiles > 1;
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kPoolWaves - 1) / kPoolWaves;

  for (int32_t fp = 0; fp < a.plan.f_passes; ++fp) {
    const int32_t f0 = fp * 16 * NT;
    const int32_t left = (a.f - f0 + 15) / 16, nt_live = left < NT ? left : NT;
    if (!multi_k) {
      __syncthreads();
      PoolStageW<DT, NT>(a, f0, 0, wt);
      __syncthreads();
    }
    // the column lane l folds in half h; a.f (stored nowhere) for a lane beyond the tile's 16 NT columns or beyond F
    float bv[NH];
    int32_t cols[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int32_t col = f0 + 64 * h + lane;
      cols[h] = (64 * h + lane < 16 * NT && col < a.f) ? col : a.f;
      bv[h] = 0.f;
      if (a.bias && cols[h] < a.f)
        bv[h] = a.bias_f32 ? static_cast<const float*>(a.bias)[col]
                           : TkWiden<DT>(DT == kF32 ? static_cast<const uint32_t*>(a.bias)[col]
                                                    : (uint32_t)static_cast<const uint16_t*>(a.bias)[col]);
    }

    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
      const int64_t r0 = (grp * kPoolWaves + wave) * kPoolTile;
      const int32_t nr = r0 >= a.size ? 0 : (a.size - r0 < kPoolTile ? (int32_t)(a.size - r0) : kPoolTile);
      // boundary i of the run in lane i (0 .. nr), non-decreasing within the run
      // (e < 2^31: a boundary fits 32 bits; the reads below take a wave-uniform lane, so every
      // position of the walk is a scalar)
      int32_t bound = 0;
      if (nr > 0 && lane <= nr) bound = (int32_t)PoolBoundary(a.seg_ptr, a.count, a.e, r0 + lane);
#pragma unroll
      for (int s = 1; s < 32; s <<= 1) {
        const int32_t below = __shfl_up(bound, s);
        if (lane >= s && below > bound) bound = below;
      }
      const int32_t pb = __builtin_amdgcn_readlane(bound, 0), pe = __builtin_amdgcn_readlane(bound, nr);
      const int32_t mine = (int32_t)(((int64_t)pe - pb + kPoolTile - 1) / kPoolTile);
      int32_t tiles = mine;
      if (multi_k) {                              // the waves of the workgroup move in lockstep
        s_tiles[wave] = mine;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kPoolWaves; ++w) tiles = s_tiles[w] > tiles ? s_tiles[w] : tiles;
        __syncthreads();
      }
      // the fold's walk: destination r0 + ri owns [seg_b, seg_e)
      int32_t ri = 0;
      int32_t seg_b = pb, seg_e = __builtin_amdgcn_readlane(bound, 1);
      float run[NH];
#pragma unroll
      for (int h = 0; h < NH; ++h) run[h] = 0.f;

      int64_t row = (int64_t)pb + c < pe ? TkRow(a.gather, a.is_ids, (int64_t)pb + c, a.rows) : -1;
      for (int32_t t = 0; t < tiles; ++t) {
        const bool active = t < mine;
        const int32_t p0 = pb + t * kPoolTile;
        const int64_t at = row < 0 ? -1 : row * a.d;
        const int64_t next = (int64_t)p0 + kPoolTile + c;      // (e may be 2^31 - 1: not in 32 bits)
        row = next < pe ? TkRow(a.gather, a.is_ids, next, a.rows) : -1;
        PoolAcc acc[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = PoolAcc{0.f, 0.f, 0.f, 0.f};

        for (int32_t kt = 0; kt < a.plan.k_tiles; ++kt) {
          if (multi_k) {
            __syncthreads();
            PoolStageW<DT, NT>(a, f0, kt, wt);
            __syncthreads();
          }
          if (!active) continue;
          const int32_t k_base = kt * a.plan.k_tile;
          const int32_t k_len = d32 - k_base < a.plan.k_tile ? d32 - k_base : a.plan.k_tile;
          const int32_t chunks = k_len / kPoolChunk;
#pragma unroll 1
          for (int32_t kc = 0; kc < chunks; kc += kPoolBatch) {
            PoolWords av[kPoolBatch][FW];
#pragma unroll
            for (int x = 0; x < kPoolBatch; ++x)
              PoolLoadA<DT, VEC>(a.table, kc + x < chunks ? at : -1, k_base + (kc + x) * kPoolChunk + 8 * g, a.d, av[x]);
#pragma unroll
            for (int x = 0; x < kPoolBatch; ++x) {
              if (kc + x < chunks) {
#pragma unroll
                for (int n = 0; n < NT; ++n) {      // (columns from F on are +0 in LDS: no branch here)
                  const unsigned char* bp =
                      wt + ((size_t)(n * 16 + c) * a.plan.k_stride + (kc + x) * kPoolChunk + 8 * g) * kEsz;
                  PoolWords bw[FW];
#pragma unroll
                  for (int q = 0; q < FW; ++q) bw[q] = reinterpret_cast<const PoolWords*>(bp)[q];
                  acc[n] = PoolMma<DT>(av[x], bw, acc[n]);
                }
                __builtin_amdgcn_sched_barrier(0);      // (keeps the B reads of later chunks out of this one's registers)
              }
            }
          }
        }
        if (!active) continue;

        const int32_t rows_here = pe - p0 < kPoolTile ? pe - p0 : kPoolTile;
        const int32_t ri_s = ri;
        const int32_t seg_b_s = seg_b, seg_e_s = seg_e;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
          if (4 * h >= nt_live) continue;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (4 * h + q < NT && 4 * h + q < nt_live) {
#pragma unroll
              for (int i = 0; i < 4; ++i) stage[(4 * g + i) * kPoolStageStride + q * 16 + c] = acc[(4 * h + q) % NT][i];
            }
          }
          PoolWaveFence();
          ri = ri_s; seg_b = seg_b_s; seg_e = seg_e_s;
          for (int32_t j = 0; j < rows_here; ++j) {
            const int32_t p = p0 + j;
            while (p >= seg_e) {                  // (ends at the run's last boundary, pe > p, at the latest)
              PoolStore<DT>(a, r0 + ri, cols[h], PoolFinish(a.op, run[h], seg_e - seg_b));
              ++ri;
              seg_b = seg_e;
              seg_e = __builtin_amdgcn_readlane(bound, ri + 1);
            }
            const float v = PoolAct(a.act, (cols[h] < a.f ? stage[j * kPoolStageStride + lane] : 0.f) + bv[h]);
            run[h] = PoolFold(a.op, run[h], v, p == seg_b);
          }
          PoolWaveFence();
        }
      }
      // what the walk has not passed: the run's last segment and the empty ones after it
      while (ri < nr) {
#pragma unroll
        for (int h = 0; h < NH; ++h)
          if (4 * h < nt_live) PoolStore<DT>(a, r0 + ri, cols[h], PoolFinish(a.op, run[h], seg_e - seg_b));
        ++ri;
        seg_b = seg_e;
        seg_e = __builtin_amdgcn_readlane(bound, ri + 1);
      }
    }
  }
}

template <int DT, int NT, bool VEC>
int PoolLaunch(hipStream_t st, const PoolArgs& a) {
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kPoolWaves - 1) / kPoolWaves;
  const unsigned blocks = (unsigned)(groups > kPoolMaxBlocks ? kPoolMaxBlocks : groups);
  hipLaunchKernelGGL((PoolKernel<DT, NT, VEC>), dim3(blocks), dim3(64 * kPoolWaves), (size_t)a.plan.lds_bytes, st, a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DT, int NT>
int PoolDispatchLoads(hipStream_t st, const PoolArgs& a) {
  return PoolVectorLoads(a.d, (uintptr_t)a.table, DT == kF32) ? PoolLaunch<DT, NT, true>(st, a)
                                                              : PoolLaunch<DT, NT, false>(st, a);
}

template <int DT>
int PoolDispatchTile(hipStream_t st, const PoolArgs& a) {
  switch (a.plan.nt) {
    case 1: return PoolDispatchLoads<DT, 1>(st, a);
    case 2: return PoolDispatchLoads<DT, 2>(st, a);
    case 4: return PoolDispatchLoads<DT, 4>(st, a);
    default: return PoolDispatchLoads<DT, 8>(st, a);
  }
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_pool_aggregate(void* stream, int32_t op, int32_t act, const void* table_dev, int32_t dtype,
                             int64_t rows, const void* weight_dev, const void* bias_dev, int32_t bias_dtype,
                             const void* gather_dev, int32_t gather_is_ids, const int64_t* seg_ptr_dev,
                             int64_t count, int64_t e, int64_t d, int64_t f, int64_t size, void* out_dev,
                             int32_t out_dtype) {
  const std::string what("pool_aggregate");
  if (op != kPoolMax && op != kPoolMean && op != kPoolAdd) return Fail(EULER_GPU_EINVAL, what + ": op is 0 max, 1 mean, 2 add");
  if (act != kPoolRelu && act != kPoolNone) return Fail(EULER_GPU_EINVAL, what + ": activation is 0 relu, 1 none");
  if (!KnownDtype(dtype) || !KnownDtype(out_dtype) || (bias_dev && !KnownDtype(bias_dtype)))
    return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (out_dtype != EULER_GPU_F32 && out_dtype != dtype)
    return Fail(EULER_GPU_EINVAL, what + ": out is fp32 or of the table's dtype");
  if (bias_dev && bias_dtype != EULER_GPU_F32 && bias_dtype != dtype)
    return Fail(EULER_GPU_EINVAL, what + ": bias is fp32 or of the table's dtype");
  if (size < 0 || e < 0 || count < 0) return Fail(EULER_GPU_EINVAL, what + ": size, e or count < 0");
  if (e >= (1LL << 31) || size >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, what + ": e or size >= 2^31");
  if (d < 1 || d > kPoolMaxDim || f < 1 || f > kPoolMaxDim) return Fail(EULER_GPU_EINVAL, what + ": d or F outside 1..4096");
  if ((seg_ptr_dev != nullptr) == (count > 0))
    return Fail(EULER_GPU_EINVAL, what + ": exactly one of seg_ptr and count");
  if (!seg_ptr_dev && (count >= (1LL << 31) || e != size * count)) return Fail(EULER_GPU_EINVAL, what + ": count needs e == size * count");
  if (size == 0) return EULER_GPU_OK;
  if (!table_dev || !weight_dev || !out_dev) return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  if (rows < 1) return Fail(EULER_GPU_EINVAL, what + ": a table with fewer than 1 row");
  const uintptr_t esz = dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)table_dev % esz != 0 || (uintptr_t)weight_dev % esz != 0 ||
      (uintptr_t)bias_dev % (bias_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)out_dev % (out_dtype == EULER_GPU_F32 ? 4 : 2) != 0 || (uintptr_t)seg_ptr_dev % 8 != 0 ||
      (uintptr_t)gather_dev % (gather_is_ids ? 8 : 4) != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  PoolArgs a{};
  a.table = table_dev; a.rows = rows; a.weight = weight_dev;
  a.bias = bias_dev; a.bias_f32 = bias_dtype == EULER_GPU_F32;
  a.gather = gather_dev; a.is_ids = gather_is_ids != 0;
  a.seg_ptr = seg_ptr_dev; a.count = count; a.e = e;
  a.d = (int32_t)d; a.f = (int32_t)f; a.size = (int32_t)size; a.op = op; a.act = act;
  a.out = out_dev; a.out_f32 = out_dtype == EULER_GPU_F32;
  a.plan = PoolMakePlan(d, f, dtype == EULER_GPU_F32);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EULER_GPU_F32) return PoolDispatchTile<kF32>(st, a);
  if (dtype == EULER_GPU_BF16) return PoolDispatchTile<kBF16>(st, a);
  return PoolDispatchTile<kF16>(st, a);
}

}  // extern "C"
