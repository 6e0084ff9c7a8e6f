// The fused backward of pool_aggregate (GraphSAGE meanpool / maxpool: tf_euler/python/utils/aggregators.py:
// 75-114) on the matrix units of gfx950, with its C-ABI entry point.  The contract, the order of every sum
// and the split into kernels are stated in mp_pool_backward.h; the fragments, the W^T staging and the
// staging rows of the walk are the forward's (mp_pool_frag.h), dZ W^T and the slab-wise X^T dZ are the dense
// backward's (mp_dense_backward_frag.h).
//
// THE WALK KERNEL is the forward's kernel with another walk.  Per F-tile pass the workgroup stages W^T, then
// every wave takes runs of 16 destinations; per tile of 16 positions it recomputes the 16 x 16 NT block of
// pre-activations with the forward's loads and MFMAs in the forward's order, writes 64 columns of it to its
// staging rows, and lane l walks column l down the rows in increasing p.
//   ZPASS false (op max): bias, activation, fold with a tie counter; at a segment's end m and grad / ties.
//   ZPASS true: at a segment's begin the lane reads its column's share (and m); per row it decides the
//   position's dZ and stores it - the 64 lanes of a wave write 64 adjacent columns of row p.
// No atomics, no scratch, no host wait: at most eight launches on the caller's stream.
#include <hip/hip_runtime.h>

#include "common.h"
#include "mp_dense_backward_frag.h"
#include "mp_pool_backward.h"
#include "mp_pool_frag.h"

namespace euler_gpu {
namespace {

struct PoolBwdArgs {
  const void* table; int64_t rows;
  const void* weight;
  const void* bias; int32_t bias_f32;
  const void* gather; int32_t is_ids;
  const int64_t* seg_ptr; int64_t count, e;
  int32_t d, f, size, op, act;
  int32_t need_z;                       // max or relu: the recomputed values decide; else dZ is the share
  const void* grad; int32_t grad_f32;
  float* m_ws; float* share_ws;         // [size, f] fp32, op max
  void* dz;                             // [e, f] of the table's dtype
  PoolPlan plan;
};

// the finished (segment, column) of the max pass: its maximum and the share of one maximal position
template <int DT>
__device__ __forceinline__ void PoolBwdStoreMax(const PoolBwdArgs& a, int64_t r, int32_t col, float m, int32_t ties) {
  if (col >= a.f) return;
  const int64_t at = r * a.f + col;
  a.m_ws[at] = ties ? m : 0.f;
  a.share_ws[at] = ties ? MpwDiv(DenseBwdGrad<DT>(a.grad, a.grad_f32, at), (float)ties) : 0.f;
}

// the share (and, for max, the maximum) of column col of destination r, a segment of len positions
template <int DT>
__device__ __forceinline__ void PoolBwdShare(const PoolBwdArgs& a, int64_t r, int32_t col, int32_t len, float* share,
                                             float* m) {
  *share = 0.f;
  *m = 0.f;
  if (col >= a.f || len <= 0) return;
  const int64_t at = r * a.f + col;
  if (a.op == kPoolMax) {
    *share = a.share_ws[at];
    *m = a.m_ws[at];
  } else {
    const float gv = DenseBwdGrad<DT>(a.grad, a.grad_f32, at);
    *share = a.op == kPoolMean ? MpwMul(gv, MpwDiv(1.f, (float)len)) : gv;
  }
}

template <int DT, int NT, bool VEC, bool ZPASS>
__global__ __launch_bounds__(64 * kPoolWaves, 3) void PoolBwdWalkKernel(const PoolBwdArgs a) {
  constexpr int FW = PoolFragWords<DT>();
  constexpr int NH = (NT + 3) / 4;                // halves of 64 columns the walk takes in turn
  constexpr int kEsz = DT == kF32 ? 4 : 2;
  const int32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  float* stage = reinterpret_cast<float*>(pool_lds) + wave * kPoolTile * kPoolStageStride;
  unsigned char* wt = pool_lds + kPoolStageBytes;
  const int32_t chunks = (a.d + kPoolChunk - 1) / kPoolChunk;     // (k_tiles == 1: one K tile holds them all)
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kPoolWaves - 1) / kPoolWaves;
  const bool need_z = !ZPASS || a.need_z != 0;
  const bool is_max = a.op == kPoolMax, relu = a.act == kPoolRelu;

  for (int32_t fp = 0; fp < a.plan.f_passes; ++fp) {
    const int32_t f0 = fp * 16 * NT;
    const int32_t left = (a.f - f0 + 15) / 16, nt_live = left < NT ? left : NT;
    if (need_z) {
      __syncthreads();
      PoolStageW<DT, NT>(a, f0, 0, wt);
      __syncthreads();
    }
    // the column lane l walks in half h; a.f (stored nowhere) beyond the tile's 16 NT columns or beyond F
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
      // boundary i of the run in lane i (0 .. nr), non-decreasing within the run: the forward's
      int32_t bound = 0;
      if (nr > 0 && lane <= nr) bound = (int32_t)PoolBoundary(a.seg_ptr, a.count, a.e, r0 + lane);
#pragma unroll
      for (int s = 1; s < 32; s <<= 1) {
        const int32_t below = __shfl_up(bound, s);
        if (lane >= s && below > bound) bound = below;
      }
      const int32_t pb = __builtin_amdgcn_readlane(bound, 0), pe = __builtin_amdgcn_readlane(bound, nr);
      const int32_t tiles = (int32_t)(((int64_t)pe - pb + kPoolTile - 1) / kPoolTile);
      // the walk: destination r0 + ri owns [seg_b, seg_e)
      int32_t ri = 0;
      int32_t seg_b = pb, seg_e = __builtin_amdgcn_readlane(bound, 1);
      float run[NH], share[NH];                   // ZPASS: the maximum and the share of destination r0 + ri
      int32_t ties[NH];
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        run[h] = share[h] = 0.f;
        ties[h] = 0;
        if (ZPASS && nr > 0) PoolBwdShare<DT>(a, r0, cols[h], seg_e - seg_b, &share[h], &run[h]);
      }

      int64_t row = (need_z && (int64_t)pb + c < pe) ? TkRow(a.gather, a.is_ids, (int64_t)pb + c, a.rows) : -1;
      for (int32_t t = 0; t < tiles; ++t) {
        const int32_t p0 = pb + t * kPoolTile;
        PoolAcc acc[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = PoolAcc{0.f, 0.f, 0.f, 0.f};
        if (need_z) {
          const int64_t at = row < 0 ? -1 : row * a.d;
          const int64_t next = (int64_t)p0 + kPoolTile + c;      // (e may be 2^31 - 1: not in 32 bits)
          row = next < pe ? TkRow(a.gather, a.is_ids, next, a.rows) : -1;
#pragma unroll 1
          for (int32_t kc = 0; kc < chunks; kc += kPoolBatch) {
            PoolWords av[kPoolBatch][FW];
#pragma unroll
            for (int x = 0; x < kPoolBatch; ++x)
              PoolLoadA<DT, VEC>(a.table, kc + x < chunks ? at : -1, (kc + x) * kPoolChunk + 8 * g, a.d, av[x]);
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

        const int32_t rows_here = pe - p0 < kPoolTile ? pe - p0 : kPoolTile;
        const int32_t ri_s = ri;
        const int32_t seg_b_s = seg_b, seg_e_s = seg_e;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
          if (4 * h >= nt_live) continue;
          if (need_z) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              if (4 * h + q < NT && 4 * h + q < nt_live) {
#pragma unroll
                for (int i = 0; i < 4; ++i) stage[(4 * g + i) * kPoolStageStride + q * 16 + c] = acc[(4 * h + q) % NT][i];
              }
            }
            PoolWaveFence();
          }
          ri = ri_s; seg_b = seg_b_s; seg_e = seg_e_s;
          for (int32_t j = 0; j < rows_here; ++j) {
            const int32_t p = p0 + j;
            bool moved = false;
            while (p >= seg_e) {                  // (ends at the run's last boundary, pe > p, at the latest)
              if constexpr (!ZPASS) PoolBwdStoreMax<DT>(a, r0 + ri, cols[h], run[h], seg_e > seg_b ? ties[h] : 0);
              ++ri;
              seg_b = seg_e;
              seg_e = __builtin_amdgcn_readlane(bound, ri + 1);
              moved = true;
            }
            const float z = (need_z && cols[h] < a.f ? stage[j * kPoolStageStride + lane] : 0.f) + bv[h];
            const float v = PoolAct(a.act, z);
            if constexpr (ZPASS) {
              if (moved) PoolBwdShare<DT>(a, r0 + ri, cols[h], seg_e - seg_b, &share[h], &run[h]);
              const bool on = (!is_max || v == run[h]) && (!relu || z > 0.f);
              if (cols[h] < a.f) DenseBwdPut<DT>(a.dz, (int64_t)p * a.f + cols[h], on ? share[h] : 0.f);
            } else {
              if (p == seg_b || (v > run[h]) | (v != v)) {
                run[h] = v;
                ties[h] = 1;
              } else if (v == run[h]) {
                ++ties[h];
              }
            }
          }
          if (need_z) PoolWaveFence();
        }
      }
      // what the walk has not passed: the run's last segment and the empty ones after it
      if constexpr (!ZPASS) {
        while (ri < nr) {
#pragma unroll
          for (int h = 0; h < NH; ++h)
            if (4 * h < nt_live) PoolBwdStoreMax<DT>(a, r0 + ri, cols[h], run[h], seg_e > seg_b ? ties[h] : 0);
          ++ri;
          seg_b = seg_e;
          seg_e = __builtin_amdgcn_readlane(bound, ri + 1);
        }
      }
    }
  }
}

template <int DT, int NT, bool VEC, bool ZPASS>
int PoolBwdWalkLaunch(hipStream_t st, const PoolBwdArgs& a) {
  const int64_t runs = ((int64_t)a.size + kPoolTile - 1) / kPoolTile;
  const int64_t groups = (runs + kPoolWaves - 1) / kPoolWaves;
  const unsigned blocks = (unsigned)(groups > kPoolMaxBlocks ? kPoolMaxBlocks : groups);
  hipLaunchKernelGGL((PoolBwdWalkKernel<DT, NT, VEC, ZPASS>), dim3(blocks), dim3(64 * kPoolWaves), (size_t)a.plan.lds_bytes, st, a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DT, int NT, bool ZPASS>
int PoolBwdWalkLoads(hipStream_t st, const PoolBwdArgs& a) {
  return PoolVectorLoads(a.d, (uintptr_t)a.table, DT == kF32) ? PoolBwdWalkLaunch<DT, NT, true, ZPASS>(st, a)
                                                              : PoolBwdWalkLaunch<DT, NT, false, ZPASS>(st, a);
}

template <int DT, bool ZPASS>
int PoolBwdWalk(hipStream_t st, const PoolBwdArgs& a) {
  switch (a.plan.nt) {
    case 1: return PoolBwdWalkLoads<DT, 1, ZPASS>(st, a);
    case 2: return PoolBwdWalkLoads<DT, 2, ZPASS>(st, a);
    case 4: return PoolBwdWalkLoads<DT, 4, ZPASS>(st, a);
    default: return PoolBwdWalkLoads<DT, 8, ZPASS>(st, a);
  }
}

// +0 to the dZ rows no segment owns: the positions before boundary 0 and from boundary `size` on
template <int DT>
__global__ __launch_bounds__(256) void PoolBwdEdgesKernel(const PoolBwdArgs a) {
  const int64_t head = PoolBoundary(a.seg_ptr, a.count, a.e, 0) * a.f;
  int64_t last = PoolBoundary(a.seg_ptr, a.count, a.e, a.size) * a.f;
  if (last < head) last = head;
  const int64_t tail = a.e * a.f - last;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < head + tail; i += (int64_t)gridDim.x * blockDim.x)
    DenseBwdPut<DT>(a.dz, i < head ? i : last + (i - head), 0.f);
}

struct PoolBwdCall {
  PoolBwdArgs z;
  bool rows, weight;
  DenseBwdRowsArgs rn;
  DenseBwdWeightArgs wn;
  void* d_weight; void* d_bias; int32_t bias_dtype, dtype;
};

template <int DT>
int PoolBwdRun(hipStream_t st, const PoolBwdCall& k) {
  int rc = EULER_GPU_OK;
  if (k.z.e > 0) {
    if (k.z.seg_ptr) {
      hipLaunchKernelGGL((PoolBwdEdgesKernel<DT>), dim3(kPoolMaxBlocks), dim3(256), 0, st, k.z);
      EG_HIP(hipGetLastError());
    }
    if (k.z.op == kPoolMax) rc = PoolBwdWalk<DT, false>(st, k.z);
    if (rc == EULER_GPU_OK) rc = PoolBwdWalk<DT, true>(st, k.z);
    if (rc == EULER_GPU_OK && k.rows) rc = DenseBwdRows<DT>(st, k.rn);
    if (rc == EULER_GPU_OK && k.weight) rc = DenseBwdWeight<DT, true>(st, k.wn);
  }
  // (e == 0: no slab, and the ordered sum of no partial is +0)
  const int64_t n = (int64_t)k.wn.kx * k.wn.fy;
  if (rc == EULER_GPU_OK && k.d_weight) rc = DenseBwdSum(st, k.wn.partial, k.wn.slabs, n, k.d_weight, k.dtype);
  if (rc == EULER_GPU_OK && k.d_bias) rc = DenseBwdSum(st, k.wn.bias_partial, k.wn.slabs, k.wn.fy, k.d_bias, k.bias_dtype);
  return rc;
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_pool_aggregate_backward(void* stream, int32_t op, int32_t act, const void* table_dev, int32_t dtype,
                                      int64_t rows, const void* weight_dev, const void* bias_dev, int32_t bias_dtype,
                                      const void* gather_dev, int32_t gather_is_ids, const int64_t* seg_ptr_dev,
                                      int64_t count, int64_t e, int64_t d, int64_t f, int64_t size,
                                      const void* grad_dev, int32_t grad_dtype, void* dz_ws_dev, float* m_ws_dev,
                                      float* share_ws_dev, float* partial_ws_dev, int64_t partial_ws_floats,
                                      float* d_rows_dev, void* d_weight_dev, void* d_bias_dev) {
  const std::string what("pool_aggregate_backward");
  if (op != kPoolMax && op != kPoolMean && op != kPoolAdd) return Fail(EULER_GPU_EINVAL, what + ": op is 0 max, 1 mean, 2 add");
  if (act != kPoolRelu && act != kPoolNone) return Fail(EULER_GPU_EINVAL, what + ": activation is 0 relu, 1 none");
  if (!KnownDtype(dtype) || !KnownDtype(grad_dtype) || (bias_dev && !KnownDtype(bias_dtype)))
    return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (grad_dtype != EULER_GPU_F32 && grad_dtype != dtype)
    return Fail(EULER_GPU_EINVAL, what + ": grad is fp32 or of the table's dtype");
  if (bias_dev && bias_dtype != EULER_GPU_F32 && bias_dtype != dtype)
    return Fail(EULER_GPU_EINVAL, what + ": bias is fp32 or of the table's dtype");
  if (size < 0 || e < 0 || count < 0) return Fail(EULER_GPU_EINVAL, what + ": size, e or count < 0");
  if (e >= (1LL << 31) || size >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, what + ": e or size >= 2^31");
  if (d < 1 || d > kPoolBwdMaxK || f < 1 || f > kPoolBwdMaxF)
    return Fail(EULER_GPU_EINVAL, what + ": d outside 1..256 (kPoolBwdMaxK) or F outside 1..512 (kPoolBwdMaxF)");
  if ((seg_ptr_dev != nullptr) == (count > 0))
    return Fail(EULER_GPU_EINVAL, what + ": exactly one of seg_ptr and count");
  if (!seg_ptr_dev && (count >= (1LL << 31) || e != size * count))
    return Fail(EULER_GPU_EINVAL, what + ": count needs e == size * count");
  if (size == 0) return EULER_GPU_OK;
  if (d_bias_dev && !bias_dev) return Fail(EULER_GPU_EINVAL, what + ": d_bias without a bias");
  const bool want_w = d_weight_dev || d_bias_dev;
  if (!want_w && !d_rows_dev) return EULER_GPU_OK;
  if (!table_dev || !weight_dev || !grad_dev) return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  if (rows < 1) return Fail(EULER_GPU_EINVAL, what + ": a table with fewer than 1 row");
  // (e == 0: no position, no slab - the workspaces are empty and may be null)
  if (e > 0 && (!dz_ws_dev || (op == kPoolMax && (!m_ws_dev || !share_ws_dev)) || (want_w && !partial_ws_dev)))
    return Fail(EULER_GPU_EINVAL, what + ": a wanted gradient without its workspace");
  if (want_w && partial_ws_floats < PoolBwdWorkspaceFloats(e, d, f))
    return Fail(EULER_GPU_EINVAL, what + ": partial_ws holds fewer than PoolBwdWorkspaceFloats fp32");
  const uintptr_t esz = dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)table_dev % esz != 0 || (uintptr_t)weight_dev % esz != 0 ||
      (uintptr_t)bias_dev % (bias_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)grad_dev % (grad_dtype == EULER_GPU_F32 ? 4 : 2) != 0 || (uintptr_t)seg_ptr_dev % 8 != 0 ||
      (uintptr_t)gather_dev % (gather_is_ids ? 8 : 4) != 0 || (uintptr_t)dz_ws_dev % 16 != 0 ||
      (uintptr_t)m_ws_dev % 4 != 0 || (uintptr_t)share_ws_dev % 4 != 0 || (uintptr_t)partial_ws_dev % 4 != 0 ||
      (uintptr_t)d_rows_dev % 4 != 0 || (uintptr_t)d_weight_dev % esz != 0 ||
      (uintptr_t)d_bias_dev % (bias_dtype == EULER_GPU_F32 ? 4 : 2) != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type (dz_ws: to 16 bytes)");
  const bool f32 = dtype == EULER_GPU_F32;
  PoolBwdCall k{};
  PoolBwdArgs& z = k.z;
  z.table = table_dev; z.rows = rows; z.weight = weight_dev;
  z.bias = bias_dev; z.bias_f32 = bias_dtype == EULER_GPU_F32;
  z.gather = gather_dev; z.is_ids = gather_is_ids != 0;
  z.seg_ptr = seg_ptr_dev; z.count = count; z.e = e;
  z.d = (int32_t)d; z.f = (int32_t)f; z.size = (int32_t)size; z.op = op; z.act = act;
  z.need_z = op == kPoolMax || act == kPoolRelu;
  z.grad = grad_dev; z.grad_f32 = grad_dtype == EULER_GPU_F32;
  z.m_ws = m_ws_dev; z.share_ws = share_ws_dev; z.dz = dz_ws_dev;
  z.plan = PoolMakePlan(d, f, f32);                                   // the forward's plan
  if (z.plan.k_tiles != 1) return Fail(EULER_GPU_EINVAL, what + ": the shape needs the forward's K tiling");

  k.rows = d_rows_dev != nullptr;
  k.rn.x = dz_ws_dev; k.rn.w = weight_dev; k.rn.k_all = (int32_t)f; k.rn.n_all = (int32_t)d; k.rn.size = (int32_t)e;
  k.rn.out32 = d_rows_dev;
  k.rn.plan = DenseBwdRowsPlan(f, d, f32);
  if (k.rows && k.rn.plan.w_tiles != 1) return Fail(EULER_GPU_EINVAL, what + ": the shape needs a K tiling of W");

  const int64_t slabs = PoolBwdSlabs(e);
  k.weight = want_w;
  k.wn.x = table_dev; k.wn.kx = (int32_t)d; k.wn.vec_x = PoolVectorLoads(d, (uintptr_t)table_dev, f32);
  k.wn.y = dz_ws_dev; k.wn.fy = (int32_t)f; k.wn.vec_y = PoolVectorLoads(f, (uintptr_t)dz_ws_dev, f32);
  k.wn.size = (int32_t)e; k.wn.slab_rows = (int32_t)DenseBwdSlabRows(e); k.wn.slabs = (int32_t)slabs;
  k.wn.partial = partial_ws_dev;
  k.wn.bias_partial = d_bias_dev ? partial_ws_dev + slabs * d * f : nullptr;
  k.wn.gather = gather_dev; k.wn.is_ids = gather_is_ids != 0; k.wn.x_rows = rows;
  k.d_weight = d_weight_dev; k.d_bias = d_bias_dev; k.bias_dtype = bias_dtype; k.dtype = dtype;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EULER_GPU_F32) return PoolBwdRun<kF32>(st, k);
  if (dtype == EULER_GPU_BF16) return PoolBwdRun<kBF16>(st, k);
  return PoolBwdRun<kF16>(st, k);
}

}  // extern "C"
