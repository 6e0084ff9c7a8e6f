// edge_softmax for gfx950: the softmax of the [e, heads] logits over the updates of every
// destination, and its gradient, each in one read and one write - and their C-ABI entry points.
// The arithmetic (a project-owned exp, the summation order, the backward formula) is defined in
// mp_softmax.h; the kernels here only decide which lane holds what:
//
//  - EdgeSoftmaxShortKernel: one lane per (destination, head) with 1..32 updates - what a sampled
//    block has (10..25 a destination).  The lane reads its values once into registers and keeps
//    them across max, sum and normalise.  A destination's len * heads values are adjacent, so the
//    64 lanes of a wave own one contiguous stretch of the input (64 * len values) - but ONE load
//    instruction is not contiguous: for a given k, lanes of different destinations are len * heads
//    elements apart (runs of `heads` adjacent lanes).  The unrolled loads k = 0 .. len - 1 are
//    issued back to back and walk through the same cache lines, so a line comes from L2 once and
//    its other uses hit in the L1; nothing is staged through LDS (times: DESIGN 4.11).
//  - EdgeSoftmaxLongKernel: a 256-thread block per longer destination (full-neighbour blocks,
//    hubs), three passes over it (max, sum, normalise; the second and third out of L2).  When
//    heads divides 64 a lane keeps one head and the block reads the destination's rows
//    contiguously; otherwise the block takes one head at a time.  The four wave results meet in
//    LDS (64 floats a wave, written and read between barriers; no atomics anywhere).
//    Each block scans 256 destinations for long ones with one ballot per wave.
//
// The destinations come as a SegSpec (mp_segments.h): grouped scatter keys (with `perm` when the
// keys had to be sorted: values are read from and written to their INPUT position), seg_ptr, or a
// uniform count - with a count the host knows which of the two kernels is needed, otherwise both
// run and each skips what belongs to the other.  Bounds are clamped to [0, e].
#include <hip/hip_runtime.h>

#include "device_fns.h"
#include "device_mem.h"
#include "half_cvt.h"
#include "mp_segments.h"
#include "mp_softmax.h"

namespace euler_gpu {
namespace {

__device__ __forceinline__ float LoadWide(const void* p, int32_t dt, int64_t i) {
  if (dt == EULER_GPU_F32) return static_cast<const float*>(p)[i];
  const uint16_t h = static_cast<const uint16_t*>(p)[i];
  return dt == EULER_GPU_BF16 ? HalfCvt<kBF16>::Widen(h) : HalfCvt<kF16>::Widen(h);
}

__device__ __forceinline__ void StoreNarrow(void* p, int32_t dt, int64_t i, float v) {
  if (dt == EULER_GPU_F32) static_cast<float*>(p)[i] = v;
  else if (dt == EULER_GPU_BF16) static_cast<uint16_t*>(p)[i] = HalfCvt<kBF16>::Narrow(v);
  else static_cast<uint16_t*>(p)[i] = HalfCvt<kF16>::Narrow(v);
}

// what both kernels take.  Forward: a = the logits (b unused); backward: a = y, b = g.
struct SmxArgs {
  const void* a; int32_t a_dt;
  const void* b; int32_t b_dt;
  SegSpec seg;
  const uint32_t* perm;
  int64_t e;
  int32_t heads;
  void* out; int32_t out_dt;
};

__device__ __forceinline__ void ClampedBounds(const SmxArgs& A, int64_t r, int64_t* b, int64_t* en) {
  SegBounds(A.seg, r, b, en);
  *b = *b < 0 ? 0 : (*b > A.e ? A.e : *b);
  *en = *en < *b ? *b : (*en > A.e ? A.e : *en);
}

template <int K, bool GRAD>
__global__ __launch_bounds__(256) void EdgeSoftmaxShortKernel(const SmxArgs A) {
  const int64_t tasks = (int64_t)A.seg.size * A.heads;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t threads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = tid; t < tasks; t += threads) {
    const int64_t r = t / A.heads;
    const int64_t h = t - r * A.heads;
    int64_t b, en;
    ClampedBounds(A, r, &b, &en);
    const int64_t len = en - b;
    if (len < 1 || len > K) continue;           // (longer: EdgeSoftmaxLongKernel)
    const int32_t n = (int32_t)len;
    float x[K], g[K], y[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (k < n) {
        const int64_t at = (A.perm ? (int64_t)A.perm[b + k] : b + k) * A.heads + h;
        x[k] = LoadWide(A.a, A.a_dt, at);
        if (GRAD) g[k] = LoadWide(A.b, A.b_dt, at);
      }
    }
    if (GRAD) SmxShortBackward<K>(x, g, n, y);
    else SmxShortForward<K>(x, n, y);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (k < n) {
        const int64_t at = (A.perm ? (int64_t)A.perm[b + k] : b + k) * A.heads + h;
        StoreNarrow(A.out, A.out_dt, at, y[k]);
      }
    }
  }
  // updates that belong to no destination get 0: keys outside [0, size) (they are the first and
  // the last of the grouped array, found by two looks in the common case of none), and what lies
  // before seg_ptr[0] or from seg_ptr[size] on
  int64_t lo = 0, hi = A.e;
  if (A.seg.keys != nullptr) {
    if (A.e > 0 && (A.seg.keys[0] < 0 || A.seg.keys[A.e - 1] >= A.seg.size)) {
      lo = LowerBound(A.seg.keys, A.e, 0);
      hi = LowerBound(A.seg.keys, A.e, A.seg.size);
    }
  } else if (A.seg.ptr != nullptr) {
    int64_t unused;
    hi = 0;                                             // (size == 0: every update is outside)
    if (A.seg.size > 0) {
      ClampedBounds(A, 0, &lo, &unused);
      ClampedBounds(A, A.seg.size - 1, &unused, &hi);
    }
  }
  if (lo > 0 || hi < A.e) {
    const int64_t outside = (lo + (A.e - hi)) * A.heads;
    for (int64_t j = tid; j < outside; j += threads) {
      const int64_t q = j / A.heads, h = j - q * A.heads;
      const int64_t p = q < lo ? q : hi + (q - lo);
      StoreNarrow(A.out, A.out_dt, (A.perm ? (int64_t)A.perm[p] : p) * A.heads + h, 0.f);
    }
  }
}

// One (destination, unit) by the whole block: unit = every head at once (hc == heads) or head u.
template <bool GRAD>
__device__ __forceinline__ void LongUnit(const SmxArgs& A, int64_t r, int32_t u, int32_t hc,
                                         float (*red)[4][64]) {
  int64_t b, en;
  ClampedBounds(A, r, &b, &en);
  const int64_t n = en - b;
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t hl = lane % hc;                         // the head's slot among the wave's hc
  const int64_t head = hc == 1 ? u : hl;
  const int64_t w = kSmxBlock / hc;                     // partials of a head
  const int64_t l = (int64_t)wave * (64 / hc) + lane / hc;
  const auto at = [&](int64_t p) { return (A.perm ? (int64_t)A.perm[b + p] : b + p) * A.heads + head; };
  const auto la = [&](int64_t p) { return LoadWide(A.a, A.a_dt, at(p)); };
  float m = 0.f, s;
  if (!GRAD) {
    m = SmxLaneMax(la, l, w, n);
    for (int32_t off = 32; off >= hc; off >>= 1) m = SmxMax(m, __shfl_xor(m, off));
    if (lane < hc) red[0][wave][lane] = m;
    __syncthreads();
    m = SmxMax(SmxMax(red[0][0][hl], red[0][1][hl]), SmxMax(red[0][2][hl], red[0][3][hl]));
    s = SmxLaneExpSum(la, m, l, w, n);
  } else {
    const auto lb = [&](int64_t p) { return LoadWide(A.b, A.b_dt, at(p)); };
    s = SmxLaneDotSum(la, lb, l, w, n);
  }
  for (int32_t off = 32; off >= hc; off >>= 1) s = MpwAdd(s, __shfl_xor(s, off));
  if (lane < hc) red[1][wave][lane] = s;
  __syncthreads();
  s = SmxCombine4(red[1][0][hl], red[1][1][hl], red[1][2][hl], red[1][3][hl]);
  for (int64_t p = l; p < n; p += w) {
    const int64_t i = at(p);
    const float v = LoadWide(A.a, A.a_dt, i);
    StoreNarrow(A.out, A.out_dt, i,
                GRAD ? SmxBackwardValue(v, LoadWide(A.b, A.b_dt, i), s) : SmxForwardValue(v, m, s));
  }
  __syncthreads();                                      // red is free again
}

// gridDim.x chunks of 256 destinations, gridDim.y blocks share the long ones of a chunk
template <bool GRAD>
__global__ __launch_bounds__(kSmxBlock) void EdgeSoftmaxLongKernel(const SmxArgs A, const int32_t hc) {
  __shared__ unsigned long long masks[4];
  __shared__ float red[2][4][64];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t units = hc == 1 ? A.heads : 1;                     // hc == 1: a head at a time
  for (int64_t base = (int64_t)blockIdx.x * kSmxBlock; base < A.seg.size; base += (int64_t)gridDim.x * kSmxBlock) {
    const int64_t r = base + threadIdx.x;
    bool is_long = false;
    if (r < A.seg.size) {
      int64_t b, en;
      ClampedBounds(A, r, &b, &en);
      is_long = en - b > kSmxShort;
    }
    const unsigned long long mine = __ballot(is_long);
    if (lane == 0) masks[wave] = mine;
    __syncthreads();
    uint32_t seen = 0;
    for (int32_t wv = 0; wv < 4; ++wv) {
      unsigned long long mk = masks[wv];
      while (mk) {
        const int32_t bit = __ffsll((long long)mk) - 1;
        mk &= mk - 1;
        if (seen++ % gridDim.y != blockIdx.y) continue;
        for (int32_t u = 0; u < units; ++u) LongUnit<GRAD>(A, base + wv * 64 + bit, u, hc, red);
      }
    }
    __syncthreads();                                    // masks are free again
  }
}

template <bool GRAD>
int Launch(hipStream_t st, const SmxArgs& A, bool uniform, int64_t count) {
  const int64_t tasks = (int64_t)A.seg.size * A.heads;
  if (!uniform || count <= kSmxShort) {
    int64_t blocks = (tasks + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 256 * 32 ? 256 * 32 : blocks);
    if (uniform && count <= 16)
      hipLaunchKernelGGL((EdgeSoftmaxShortKernel<16, GRAD>), dim3((unsigned)blocks), dim3(256), 0, st, A);
    else
      hipLaunchKernelGGL((EdgeSoftmaxShortKernel<kSmxShort, GRAD>), dim3((unsigned)blocks), dim3(256), 0, st, A);
    EG_HIP(hipGetLastError());
  }
  if ((!uniform || count > kSmxShort) && A.seg.size > 0) {
    const SmxLongGrid g = SmxLongGridFor(A.seg.size);
    hipLaunchKernelGGL((EdgeSoftmaxLongKernel<GRAD>), dim3(g.chunks, g.share), dim3(kSmxBlock), 0, st, A,
                       SmxHeadsPerWave(A.heads));
    EG_HIP(hipGetLastError());
  }
  return EULER_GPU_OK;
}

template <bool GRAD>
int EdgeSoftmaxImpl(const char* what, void* stream, const void* a, int32_t a_dt, const void* b, int32_t b_dt,
                    const int32_t* indices, const int64_t* seg_ptr, int64_t count, int64_t e, int32_t heads,
                    int32_t size, void* out, int32_t out_dt) {
  const std::string w(what);
  if (!KnownDtype(a_dt) || !KnownDtype(b_dt) || !KnownDtype(out_dt))
    return Fail(EULER_GPU_EINVAL, w + ": unknown dtype" + kDtypeCodes);
  if (heads < 1) return Fail(EULER_GPU_EINVAL, w + ": heads < 1");
  if (e < 0 || size < 0 || count < 0) return Fail(EULER_GPU_EINVAL, w + ": bad shape");
  hipStream_t st = (hipStream_t)stream;
  SegDest dst(st, indices, seg_ptr, count, e, size);
  if (const char* why = dst.FormError()) return Fail(EULER_GPU_EINVAL, w + ": " + why);
  if (e == 0) return EULER_GPU_OK;
  if (!a || !out || (GRAD && !b)) return Fail(EULER_GPU_EINVAL, w + ": null buffer");
  if (const char* why = dst.LengthError()) return Fail(EULER_GPU_EINVAL, w + ": " + why);
  const int rc = dst.Resolve();
  if (rc != EULER_GPU_OK) return rc;
  const SmxArgs A{a, a_dt, b, b_dt, dst.seg(), dst.perm(), e, heads, out, out_dt};
  return Launch<GRAD>(st, A, count > 0, count);
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_edge_softmax(void* stream, const void* logits_dev, int32_t in_dtype, const int32_t* indices_dev,
                           const int64_t* seg_ptr_dev, int64_t count, int64_t e, int32_t heads, int32_t size,
                           void* out_dev, int32_t out_dtype) {
  if (KnownDtype(in_dtype) && out_dtype != EULER_GPU_F32 && out_dtype != in_dtype)
    return Fail(EULER_GPU_EINVAL, "edge_softmax: out_dtype is fp32 or in_dtype");
  return EdgeSoftmaxImpl<false>("edge_softmax", stream, logits_dev, in_dtype, nullptr, EULER_GPU_F32, indices_dev,
                                seg_ptr_dev, count, e, heads, size, out_dev, out_dtype);
}

int euler_gpu_edge_softmax_grad(void* stream, const void* y_dev, int32_t y_dtype, const void* grad_dev,
                                int32_t grad_dtype, const int32_t* indices_dev, const int64_t* seg_ptr_dev,
                                int64_t count, int64_t e, int32_t heads, int32_t size, void* out_dev,
                                int32_t out_dtype) {
  return EdgeSoftmaxImpl<true>("edge_softmax_grad", stream, y_dev, y_dtype, grad_dev, grad_dtype, indices_dev,
                               seg_ptr_dev, count, e, heads, size, out_dev, out_dtype);
}

}  // extern "C"
