// Per-edge dot products of two gathered rows for gfx950, and their C-ABI entry points:
//   out[p][h] = sum_c a[ai[p]][h * dh + c] * b[bi[p]][h * dh + c],   c in [0, dh), d = heads * dh
// - the gradient of an edge-weighted aggregation with respect to its weights, and AGNN's attention
// logit sum(beta * norm_i * norm_j) (agnn_conv.py:43-47) - without materialising either [E, d]
// block of gathered rows.  The tables are fp32, bf16 or fp16 (each its own type, widened
// exactly); every product and every sum is a correctly rounded fp32 operation; the result is
// stored as fp32 or rounded once to a 16-bit type.
//
// The kernel is bound by two random row reads per edge.  A (edge, head) pair is a task of dh
// columns; it is given L lanes of a wave, a wave holds 64 / L tasks, partial sums stay in
// registers and the lanes are combined inside the wave (__shfl_xor) - no LDS, no atomics.
//
// SUMMATION ORDER (fixed: the same call gives the same bits, whatever E and the grid are).
// The columns of a task are cut into chunks of V adjacent columns: V = 8 when dh % 8 == 0 and
// both tables start on a 16-byte boundary, else V = 4 when dh % 4 == 0 and the tables start on a
// 16-byte (fp32) / 8-byte (16-bit) boundary, else V = 1.  L = min(64, the power of two >= dh / V).
// Lane l takes the chunks l, l + L, l + 2 L, ... and adds their products one by one in increasing
// column order, starting FROM its first product (so dh = 1 returns the product itself); a lane
// without a chunk holds +0.  The L lane sums are then combined by a butterfly:
// for off = L / 2, L / 4, ..., 1:  s = s + s[lane ^ off].
#include <hip/hip_runtime.h>

#include "device_fns.h"
#include "device_mem.h"
#include "half_cvt.h"

namespace euler_gpu {
namespace {

// V adjacent elements of a table, widened: one 16-byte load where the type and V allow
template <int DT, int V>
__device__ __forceinline__ void LoadChunk(const void* base, int64_t at, float f[V]) {
  if constexpr (DT == kF32) {
    const float* p = static_cast<const float*>(base) + at;
    if constexpr (V == 1) {
      f[0] = *p;
    } else {
#pragma unroll
      for (int q = 0; q < V / 4; ++q) {
        const float4 v = reinterpret_cast<const float4*>(p)[q];
        f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
      }
    }
  } else {
    const uint16_t* p = static_cast<const uint16_t*>(base) + at;
    if constexpr (V == 1) {
      f[0] = HalfCvt<DT>::Widen(*p);
    } else if constexpr (V == 4) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      Widen2<DT>(v.x, &f[0], &f[1]);
      Widen2<DT>(v.y, &f[2], &f[3]);
    } else {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      Widen8<DT>(w, f);
    }
  }
}

template <int DTA, int DTB, int V>
__global__ __launch_bounds__(256) void EdgeDotKernel(
    const void* __restrict__ a, const int32_t* __restrict__ ai, const void* __restrict__ b,
    const int32_t* __restrict__ bi, const int64_t e, const int32_t heads, const int32_t dh,
    const int32_t log_l, void* __restrict__ out, const int32_t out_dtype) {
  const int32_t lanes = 1 << log_l;                 // L lanes a task
  const int32_t lane = threadIdx.x & 63;
  const int32_t sub = lane >> log_l, l = lane & (lanes - 1);
  const int64_t tasks_per_wave = 64 >> log_l;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t tasks = e * heads;
  const int64_t d = (int64_t)heads * dh;
  const int32_t chunks = dh / V;
  // the trip count is the same for every lane of a wave: the shuffles see all of them
  for (int64_t t0 = wave * tasks_per_wave; t0 < tasks; t0 += waves * tasks_per_wave) {
    const int64_t t = t0 + sub;
    const bool live = t < tasks;
    float s = 0.f;
    if (live) {
      const int64_t p = t / heads;
      const int64_t h = t - p * heads;
      const int64_t base_a = (ai ? (int64_t)ai[p] : p) * d + h * dh;
      const int64_t base_b = (bi ? (int64_t)bi[p] : p) * d + h * dh;
      bool first = true;
      for (int32_t j = l; j < chunks; j += lanes) {
        float fa[V], fb[V];
        LoadChunk<DTA, V>(a, base_a + (int64_t)j * V, fa);
        LoadChunk<DTB, V>(b, base_b + (int64_t)j * V, fb);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float m = __fmul_rn(fa[k], fb[k]);
          s = first ? m : __fadd_rn(s, m);
          first = false;
        }
      }
    }
    for (int32_t off = lanes >> 1; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off));
    if (live && l == 0) {
      if (out_dtype == EULER_GPU_F32) static_cast<float*>(out)[t] = s;
      else if (out_dtype == EULER_GPU_BF16) static_cast<uint16_t*>(out)[t] = HalfCvt<kBF16>::Narrow(s);
      else static_cast<uint16_t*>(out)[t] = HalfCvt<kF16>::Narrow(s);
    }
  }
}

template <int DTA, int DTB>
int LaunchEdgeDot(hipStream_t st, const void* a, const int32_t* ai, const void* b, const int32_t* bi,
                  int64_t e, int32_t heads, int32_t dh, void* out, int32_t out_dtype) {
  const uintptr_t al_a = (uintptr_t)a, al_b = (uintptr_t)b;
  const bool a16 = al_a % 16 == 0 && al_b % 16 == 0;
  const bool a4 = al_a % (DTA == kF32 ? 16 : 8) == 0 && al_b % (DTB == kF32 ? 16 : 8) == 0;
  const int32_t v = (dh % 8 == 0 && a16) ? 8 : (dh % 4 == 0 && a4) ? 4 : 1;
  const int32_t chunks = dh / v;
  int32_t log_l = 0;
  while (log_l < 6 && (1 << log_l) < chunks) ++log_l;
  const int64_t tasks_per_wave = 64 >> log_l;
  const int64_t waves = (e * heads + tasks_per_wave - 1) / tasks_per_wave;
  int64_t blocks = (waves + 3) / 4;
  if (blocks > 256 * 32) blocks = 256 * 32;
  const dim3 grid((unsigned)blocks), block(256);
  if (v == 8)
    hipLaunchKernelGGL((EdgeDotKernel<DTA, DTB, 8>), grid, block, 0, st, a, ai, b, bi, e, heads, dh, log_l, out, out_dtype);
  else if (v == 4)
    hipLaunchKernelGGL((EdgeDotKernel<DTA, DTB, 4>), grid, block, 0, st, a, ai, b, bi, e, heads, dh, log_l, out, out_dtype);
  else
    hipLaunchKernelGGL((EdgeDotKernel<DTA, DTB, 1>), grid, block, 0, st, a, ai, b, bi, e, heads, dh, log_l, out, out_dtype);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int DTA>
int DispatchEdgeDotB(hipStream_t st, const void* a, const int32_t* ai, const void* b, int32_t b_dtype,
                     const int32_t* bi, int64_t e, int32_t heads, int32_t dh, void* out, int32_t out_dtype) {
  if (b_dtype == EULER_GPU_F32) return LaunchEdgeDot<DTA, kF32>(st, a, ai, b, bi, e, heads, dh, out, out_dtype);
  if (b_dtype == EULER_GPU_BF16) return LaunchEdgeDot<DTA, kBF16>(st, a, ai, b, bi, e, heads, dh, out, out_dtype);
  return LaunchEdgeDot<DTA, kF16>(st, a, ai, b, bi, e, heads, dh, out, out_dtype);
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_edge_dot_t(void* stream, const void* a_dev, int32_t a_dtype, const int32_t* a_index_dev,
                         const void* b_dev, int32_t b_dtype, const int32_t* b_index_dev, int64_t e,
                         int64_t d, int32_t heads, void* out_dev, int32_t out_dtype) {
  if (!KnownDtype(a_dtype) || !KnownDtype(b_dtype) || !KnownDtype(out_dtype))
    return Fail(EULER_GPU_EINVAL, std::string("edge_dot: unknown dtype") + kDtypeCodes);
  if (heads < 1) return Fail(EULER_GPU_EINVAL, "edge_dot: heads < 1");
  if (e < 0 || d < 0 || d % heads != 0) return Fail(EULER_GPU_EINVAL, "edge_dot: heads must divide d");
  if (e == 0 || d == 0) return EULER_GPU_OK;
  if (!a_dev || !b_dev || !out_dev) return Fail(EULER_GPU_EINVAL, "edge_dot: null buffer");
  if (e >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, "edge_dot: e >= 2^31");
  if ((uintptr_t)a_dev % (a_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)b_dev % (b_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)out_dev % (out_dtype == EULER_GPU_F32 ? 4 : 2) != 0)
    return Fail(EULER_GPU_EINVAL, "edge_dot: a buffer is not aligned to its type");
  hipStream_t st = (hipStream_t)stream;
  const int32_t dh = (int32_t)(d / heads);
  if (a_dtype == EULER_GPU_F32)
    return DispatchEdgeDotB<kF32>(st, a_dev, a_index_dev, b_dev, b_dtype, b_index_dev, e, heads, dh, out_dev, out_dtype);
  if (a_dtype == EULER_GPU_BF16)
    return DispatchEdgeDotB<kBF16>(st, a_dev, a_index_dev, b_dev, b_dtype, b_index_dev, e, heads, dh, out_dev, out_dtype);
  return DispatchEdgeDotB<kF16>(st, a_dev, a_index_dev, b_dev, b_dtype, b_index_dev, e, heads, dh, out_dev, out_dtype);
}

int euler_gpu_edge_dot(void* stream, const float* a_dev, const int32_t* a_index_dev, const float* b_dev,
                       const int32_t* b_index_dev, int64_t e, int64_t d, int32_t heads, float* out_dev) {
  return euler_gpu_edge_dot_t(stream, a_dev, EULER_GPU_F32, a_index_dev, b_dev, EULER_GPU_F32, b_index_dev,
                              e, d, heads, out_dev, EULER_GPU_F32);
}

}  // extern "C"
