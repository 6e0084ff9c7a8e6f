// Fused segment attention for gfx950 (attention_aggregate): per destination, a logit per
// (update, head), the softmax over the destination's updates and the sum of the source rows
// weighted by it - GATConv, AGNNConv, AttentionPool and Set2SetPool (gat_conv.py:66-72,
// agnn_conv.py:36-54, attention_pool.py:36-40, set2set_pool.py:45-49) - in one pass, and the
// destination-side backward in one pass.  The arithmetic (the order of the dot, the softmax of
// mp_softmax.h, the ordered fold) is defined in mp_attention.h; the kernels here only decide which
// lane holds what.  Forward and backward are the same three phases:
//   A  a dot of the destination's row (forward: q; backward: G) with every gathered row
//      (forward: k; backward: v) - or, additive forward, a sum of two scores;
//   B  the softmax (backward: its gradient on the saved alpha, then the scale / slope);
//   C  the fold of the gathered rows (forward: v; backward, dot: k) with phase B's weights -
//      or, additive backward, the plain sum of the weights.
//
//  - SegAttShortKernel: a group of G lanes of a wave (G a power of two, 1..64) per destination
//    with 1..32 updates - what a sampled block has.  Phase A gives head h the lanes
//    [h L, (h + 1) L) of the group, L = AttLanes(dh); lane l of them holds chunk l of every
//    gathered row and the butterfly leaves every lane of the head with the logits of all updates
//    in registers (x[K], fully unrolled: no register array is indexed by a variable); each lane
//    then runs the short softmax of its head itself - or, in the one-table kernels when the head
//    has at least K lanes, lane k takes update k's exponential and division and the values are
//    shuffled (the same operations in the same order).  When phases A and C read the same table
//    (v = None) the lane keeps its chunk of every row (raw[K][4]) and folds it in phase C: the
//    rows come from memory once.  Otherwise phase C reads its own table, a chunk per lane, and
//    takes the weights of the chunk's head from that head's first lane by a wave shuffle.
//    The loads of a destination go out in three sweeps - positions, row numbers, rows - each
//    complete before its first value is used; that takes branch-free loads, hence the load modes
//    (RawOf, below).  Serves heads * L <= 64 with dh / V <= 64; K = 16 when a uniform count
//    allows, else 32.
//  - SegAttLongKernel: a 256-thread block per longer destination (and per destination of any
//    length when the short kernel does not serve the shape).  Logits go to the alpha buffer (the
//    caller's, or a staging buffer when alpha is not wanted), the softmax runs in place - the
//    short order by one lane a head up to 32 updates, the 256-partial order beyond - and the fold
//    takes a column per lane, eight loads in flight.  A hub is not split over blocks.
// Registers (--save-temps, gfx950): DESIGN 4.20 and profiles/segment_attention_kernels.txt.  No LDS
// beyond the long softmax's 2 KiB, no atomics, sizes stay on the device; the only host wait is
// GroupScatterKeys' for explicit keys.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_fns.h"
#include "device_mem.h"
#include "half_cvt.h"
#include "mp_attention.h"
#include "mp_segments.h"
#include "mp_softmax.h"

namespace euler_gpu {
namespace {

struct Table {
  const void* p;
  int32_t dt;
  uint32_t last;      // rows - 1: every row number is clamped to it
  bool vec;           // rows of 4-column chunks may be read with one 16- / 8-byte access
};

struct AttArgs {
  int32_t kind;
  Table qa; const int32_t* qa_index; int64_t da;      // phase A: the destination's row, the gathered table
  Table ka;
  Table sq; const int32_t* sq_index; Table sk;        // additive: the two score tables [*, heads]
  Table vc; int64_t dc;                               // phase C: the gathered table
  const int32_t* gsrc; int32_t gstride;               // gather indices: int32, or the low words of int64 ids
  SegSpec seg; const uint32_t* perm; int64_t e; int32_t heads;
  float scale, slope;
  const float* alpha_in;                              // backward: the saved alpha
  float* buf;                                         // forward: alpha; backward: ds
  float* logits;                                      // forward: nullptr, or where the logits go
  void* out; int32_t out_dt; bool out_vec;            // [size, dc] (additive backward: [size, heads])
  // the lane layout of phase A and the chunks of phase C
  int32_t la, va, chunks_a; int64_t dha;
  int32_t vcv; int64_t chunks_c, dhc;
  int32_t log_g;
};

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

// the v (1 or 4) columns from element `at` on, widened; f[v .. 4) = 0
__device__ __forceinline__ void LoadChunk(const Table& t, int64_t at, int32_t v, float f[4]) {
  f[1] = f[2] = f[3] = 0.f;
  if (v == 4 && t.vec) {
    if (t.dt == EULER_GPU_F32) {
      const float4 w = *reinterpret_cast<const float4*>(static_cast<const float*>(t.p) + at);
      f[0] = w.x; f[1] = w.y; f[2] = w.z; f[3] = w.w;
    } else {
      const uint2 w = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(t.p) + at);
      if (t.dt == EULER_GPU_BF16) { Widen2<kBF16>(w.x, &f[0], &f[1]); Widen2<kBF16>(w.y, &f[2], &f[3]); }
      else { Widen2<kF16>(w.x, &f[0], &f[1]); Widen2<kF16>(w.y, &f[2], &f[3]); }
    }
  } else {
    f[0] = LoadWide(t.p, t.dt, at);
    if (v == 4) { f[1] = LoadWide(t.p, t.dt, at + 1); f[2] = LoadWide(t.p, t.dt, at + 2); f[3] = LoadWide(t.p, t.dt, at + 3); }
  }
}

__device__ __forceinline__ void StoreChunk(const AttArgs& A, int64_t at, int32_t v, const float f[4]) {
  if (v == 4 && A.out_vec) {
    if (A.out_dt == EULER_GPU_F32) {
      *reinterpret_cast<float4*>(static_cast<float*>(A.out) + at) = make_float4(f[0], f[1], f[2], f[3]);
    } else {
      uint2 w;
      if (A.out_dt == EULER_GPU_BF16) { w.x = Narrow2<kBF16>(f[0], f[1]); w.y = Narrow2<kBF16>(f[2], f[3]); }
      else { w.x = Narrow2<kF16>(f[0], f[1]); w.y = Narrow2<kF16>(f[2], f[3]); }
      *reinterpret_cast<uint2*>(static_cast<uint16_t*>(A.out) + at) = w;
    }
  } else {
    StoreNarrow(A.out, A.out_dt, at, f[0]);
    if (v == 4) { StoreNarrow(A.out, A.out_dt, at + 1, f[1]); StoreNarrow(A.out, A.out_dt, at + 2, f[2]); StoreNarrow(A.out, A.out_dt, at + 3, f[3]); }
  }
}

// the partial of one chunk: the products of its v columns added to s in increasing column order
__device__ __forceinline__ float ChunkDot(const float a[4], const float b[4], int32_t v, float s) {
  if (v == 4) return AttChunkDot<4>(a, b, s);
  return AttChunkDot<1>(a, b, s);
}

__device__ __forceinline__ void ClampedBounds(const AttArgs& A, int64_t r, int64_t* b, int64_t* en) {
  SegBounds(A.seg, r, b, en);
  *b = *b < 0 ? 0 : (*b > A.e ? A.e : *b);
  *en = *en < *b ? *b : (*en > A.e ? A.e : *en);
}

__device__ __forceinline__ int64_t PosOf(const AttArgs& A, int64_t p) { return A.perm ? (int64_t)A.perm[p] : p; }

// the row of table t that the update at input position pos gathers
__device__ __forceinline__ int64_t RowOf(const AttArgs& A, const Table& t, int64_t pos) {
  const uint32_t g = (uint32_t)A.gsrc[pos * A.gstride];
  return (int64_t)(g < t.last ? g : t.last);
}

__device__ __forceinline__ int64_t IndexedRow(const Table& t, const int32_t* index, int64_t r) {
  const uint32_t g = index ? (uint32_t)index[r] : (uint32_t)r;
  return (int64_t)(g < t.last ? g : t.last);
}

// phase B's last step of the backward: dl -> ds
__device__ __forceinline__ float GradOfLogit(const AttArgs& A, float dl, float qs, float ks) {
  return A.kind == kAttDot ? MpwMul(A.scale, dl) : AttAdditiveGrad(dl, qs, ks, A.slope);
}

// How the short kernel reads the gathered tables.  Mode 0 takes any mix of storage types, any
// alignment, chunks of 1 or 4 columns and a `perm`: its loads branch on all of these, and a load
// that sits behind a branch waits for the one before it.  Modes 1 (fp32), 2 (bf16) and 3 (fp16) are
// for grouped keys, gathered tables of ONE storage type on 16- / 8-byte boundaries and chunks of 4
// columns: every load is one branch-free instruction, and the loads of a destination - the row
// numbers, then the rows - are all in flight before the first is used.
template <int M> struct RawOf { using T = float4; };
template <> struct RawOf<2> { using T = uint2; };
template <> struct RawOf<3> { using T = uint2; };

template <int M>
__device__ __forceinline__ typename RawOf<M>::T LoadRaw(const Table& t, int64_t at, int32_t v) {
  if constexpr (M == 0) {
    float f[4];
    LoadChunk(t, at, v, f);
    return make_float4(f[0], f[1], f[2], f[3]);
  } else if constexpr (M == 1) {
    return *reinterpret_cast<const float4*>(static_cast<const float*>(t.p) + at);
  } else {
    return *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(t.p) + at);
  }
}

template <int M>
__device__ __forceinline__ void WidenRaw(const typename RawOf<M>::T& r, float f[4]) {
  if constexpr (M <= 1) {
    f[0] = r.x; f[1] = r.y; f[2] = r.z; f[3] = r.w;
  } else {
    Widen2<M == 2 ? kBF16 : kF16>(r.x, &f[0], &f[1]);
    Widen2<M == 2 ? kBF16 : kF16>(r.y, &f[2], &f[3]);
  }
}

template <int M>
__device__ __forceinline__ float LoadWideM(const Table& t, int64_t i) {
  if constexpr (M == 0) return LoadWide(t.p, t.dt, i);
  else if constexpr (M == 1) return static_cast<const float*>(t.p)[i];
  else return HalfCvt<M == 2 ? kBF16 : kF16>::Widen(static_cast<const uint16_t*>(t.p)[i]);
}

template <int K, bool GRAD, bool SHARED, int M>
__global__ __launch_bounds__(256) void SegAttShortKernel(const AttArgs A) {
  using Raw = typename RawOf<M>::T;
  const int32_t G = 1 << A.log_g;
  const int32_t lane = threadIdx.x & 63;
  const int32_t gl = lane & (G - 1), gbase = lane - gl;
  const int64_t groups_per_wave = 64 >> A.log_g;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int32_t h = gl / A.la, l = gl & (A.la - 1);
  const bool slot = h < A.heads;                        // this lane belongs to a head in phases A and B
  const bool chunk_a = slot && l < A.chunks_a;          // ... and holds a chunk of it
  const bool dot_a = GRAD || A.kind == kAttDot;
  const int32_t va = M ? 4 : A.va, vcv = M ? 4 : A.vcv;
  // the trip count is the same for every lane of a wave: the shuffles see all of them
  for (int64_t r0 = wave * groups_per_wave; r0 < A.seg.size; r0 += waves * groups_per_wave) {
    const int64_t r = r0 + (lane >> A.log_g);
    int64_t b = 0, en = 0;
    if (r < A.seg.size) ClampedBounds(A, r, &b, &en);
    const bool mine = r < A.seg.size && en - b <= K;    // (longer: SegAttLongKernel)
    const int32_t n = mine ? (int32_t)(en - b) : 0;
    float x[K], y[K];
    uint32_t pos[K], g[K];                              // input position and gathered row number
    Raw raw[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { x[k] = 0.f; y[k] = 0.f; pos[k] = 0; g[k] = 0; }
#pragma unroll
    for (int k = 0; k < K; ++k) if (k < n) pos[k] = M ? (uint32_t)(b + k) : (uint32_t)PosOf(A, b + k);
#pragma unroll
    for (int k = 0; k < K; ++k) if (k < n) g[k] = (uint32_t)A.gsrc[(int64_t)pos[k] * A.gstride];
    const auto row = [&](const Table& t, uint32_t gk) { return (int64_t)(gk < t.last ? gk : t.last); };
    float qs = 0.f;                                     // additive: the destination's score
    if (A.kind == kAttAdditive && slot && n > 0 && A.sq.p)
      qs = LoadWide(A.sq.p, A.sq.dt, IndexedRow(A.sq, A.sq_index, r) * A.heads + h);
    float ks[(GRAD || !SHARED) ? K : 1];                // additive: the gathered scores
    if (A.kind == kAttAdditive) {
      if constexpr (GRAD || !SHARED) {
#pragma unroll
        for (int k = 0; k < K; ++k) ks[k] = (k < n && slot) ? LoadWideM<M>(A.sk, row(A.sk, g[k]) * A.heads + h) : 0.f;
      }
    }
    // ---- A ----
    if (dot_a) {
      float qv[4] = {0.f, 0.f, 0.f, 0.f};
      const int64_t col = (int64_t)h * A.dha + (int64_t)l * va;
      if (chunk_a && n > 0) LoadChunk(A.qa, IndexedRow(A.qa, A.qa_index, r) * A.da + col, va, qv);
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (k < n && chunk_a) raw[k] = LoadRaw<M>(A.ka, row(A.ka, g[k]) * A.da + col, va);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (k < n && chunk_a) {
          float kv[4];
          WidenRaw<M>(raw[k], kv);
          x[k] = ChunkDot(qv, kv, va, 0.f);
        }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        if (off < A.la) {
#pragma unroll
          for (int k = 0; k < K; ++k) x[k] = MpwAdd(x[k], __shfl_xor(x[k], off));
        }
      }
      if (!GRAD) {
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = AttDotLogit(x[k], A.scale);
      }
    } else {
      if constexpr (!SHARED) {
#pragma unroll
        for (int k = 0; k < K; ++k) if (k < n && slot) x[k] = AttAdditiveLogit(qs, ks[k], A.slope);
      }
    }
    // ---- B ----
    const bool spread = !GRAD && SHARED && A.la >= K;     // (one-table kernels only: 8-18 VGPRs)
    if (spread) {
      // SmxShortForward with its K exponentials and K divisions spread over the head's lanes (there
      // are at least K): lane k takes those of update k, the sum runs over the shuffled values in
      // the same order - the same operations on the same operands, so the same bits
      float m = SmxNegInf(), xm = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) if (k < n) m = SmxMax(m, x[k]);
#pragma unroll
      for (int k = 0; k < K; ++k) xm = l == k ? x[k] : xm;
      const float em = l < n ? ExpNonPositive(SmxSub(xm, m)) : 0.f;
      const int32_t first = gbase + h * A.la;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float e = __shfl(em, first + k);
        if (k < n) s = MpwAdd(s, e);
      }
      const float ym = l < n ? MpwDiv(em, s) : 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float v = __shfl(ym, first + k);
        if (k < n) y[k] = v;
      }
    }
    if (n > 0) {
      if (!GRAD) {
        if (!spread) SmxShortForward<K>(x, n, y);
      } else {
        float a[K];
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = (k < n && slot) ? A.alpha_in[(int64_t)pos[k] * A.heads + h] : 0.f;
        SmxShortBackward<K>(a, x, n, y);
        if constexpr (GRAD) {
#pragma unroll
          for (int k = 0; k < K; ++k) if (k < n && slot) y[k] = GradOfLogit(A, y[k], qs, ks[k]);
        }
      }
      if (slot && l == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          if (k < n) {
            const int64_t at = (int64_t)pos[k] * A.heads + h;
            if (A.buf) A.buf[at] = y[k];
            if (!GRAD && A.logits) A.logits[at] = x[k];
          }
        }
      }
    }
    // ---- C ----
    if (GRAD && A.kind == kAttAdditive) {
      if (mine && slot && l == 0) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) if (k < n) s = MpwAdd(s, y[k]);
        StoreNarrow(A.out, A.out_dt, r * A.heads + h, s);
      }
    } else if (SHARED) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (k < n && chunk_a) {
          float f[4];
          WidenRaw<M>(raw[k], f);
#pragma unroll
          for (int c = 0; c < 4; ++c) if (c < va) acc[c] = AttFold(acc[c], f[c], y[k]);
        }
      }
      if (mine && chunk_a) StoreChunk(A, r * A.dc + (int64_t)h * A.dha + (int64_t)l * va, va, acc);
    } else {
      for (int64_t c0 = 0; c0 < A.chunks_c; c0 += G) {
        const int64_t c = c0 + gl;
        const bool has = c < A.chunks_c;
        const int64_t col = c * vcv;
        const int32_t src = gbase + (has ? (int32_t)(col / A.dhc) : 0) * A.la;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (k < n && has) raw[k] = LoadRaw<M>(A.vc, row(A.vc, g[k]) * A.dc + col, vcv);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float w = __shfl(y[k], src);
          if (k < n && has) {
            float f[4];
            WidenRaw<M>(raw[k], f);
#pragma unroll
            for (int q = 0; q < 4; ++q) if (q < vcv) acc[q] = AttFold(acc[q], f[q], w);
          }
        }
        if (mine && has) StoreChunk(A, r * A.dc + col, vcv, acc);
      }
    }
  }
}

// updates that belong to no destination get 0 in buf (alpha / ds), as edge_softmax gives them
__device__ __forceinline__ void ZeroOutside(const AttArgs& A, int64_t tid, int64_t threads) {
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
      A.buf[PosOf(A, p) * A.heads + h] = 0.f;
    }
  }
}

// the softmax (backward: its gradient, then GradOfLogit) of one (destination, unit) with more than
// 32 updates, in place on buf, by the whole block: the long unit of edge_softmax_kernels.hip
template <bool GRAD>
__device__ __forceinline__ void LongSoftmaxUnit(const AttArgs& A, int64_t r, int64_t b, int64_t n, int32_t u,
                                                int32_t hc, float (*red)[4][64]) {
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t hl = lane % hc;
  const int64_t head = hc == 1 ? u : hl;
  const int64_t w = kSmxBlock / hc;
  const int64_t l = (int64_t)wave * (64 / hc) + lane / hc;
  const auto at = [&](int64_t p) { return PosOf(A, b + p) * A.heads + head; };
  const auto lx = [&](int64_t p) { return A.buf[at(p)]; };
  float m = 0.f, s;
  if (!GRAD) {
    m = SmxLaneMax(lx, l, w, n);
    for (int32_t off = 32; off >= hc; off >>= 1) m = SmxMax(m, __shfl_xor(m, off));
    if (lane < hc) red[0][wave][lane] = m;
    __syncthreads();
    m = SmxMax(SmxMax(red[0][0][hl], red[0][1][hl]), SmxMax(red[0][2][hl], red[0][3][hl]));
    s = SmxLaneExpSum(lx, m, l, w, n);
  } else {
    const auto ly = [&](int64_t p) { return A.alpha_in[at(p)]; };
    s = SmxLaneDotSum(ly, lx, l, w, n);
  }
  for (int32_t off = 32; off >= hc; off >>= 1) s = MpwAdd(s, __shfl_xor(s, off));
  if (lane < hc) red[1][wave][lane] = s;
  __syncthreads();
  s = SmxCombine4(red[1][0][hl], red[1][1][hl], red[1][2][hl], red[1][3][hl]);
  float qs = 0.f;
  if (GRAD && A.kind == kAttAdditive && A.sq.p)
    qs = LoadWide(A.sq.p, A.sq.dt, IndexedRow(A.sq, A.sq_index, r) * A.heads + head);
  for (int64_t p = l; p < n; p += w) {
    const int64_t i = at(p);
    if (!GRAD) {
      A.buf[i] = SmxForwardValue(A.buf[i], m, s);
    } else {
      const float ks = A.kind == kAttAdditive
          ? LoadWide(A.sk.p, A.sk.dt, RowOf(A, A.sk, PosOf(A, b + p)) * A.heads + head) : 0.f;
      A.buf[i] = GradOfLogit(A, SmxBackwardValue(A.alpha_in[i], A.buf[i], s), qs, ks);
    }
  }
  __syncthreads();                                      // red is free again
}

template <bool GRAD, int M>
__device__ __forceinline__ void LongDestination(const AttArgs& A, int64_t r, int32_t hc, float (*red)[4][64]) {
  using Raw = typename RawOf<M>::T;
  int64_t b, en;
  ClampedBounds(A, r, &b, &en);
  const int64_t n = en - b;
  const int64_t tasks = n * A.heads;
  const int32_t va = M ? 4 : A.va;
  const auto pos_of = [&](int64_t p) { return M ? p : PosOf(A, p); };
  // ---- A: a (update, head) per la lanes of a wave ----
  if (GRAD || A.kind == kAttDot) {
    const int64_t per_block = kSmxBlock / A.la;
    const int64_t sub = threadIdx.x / A.la;
    const int32_t l = threadIdx.x & (A.la - 1);
    const int64_t qrow = IndexedRow(A.qa, A.qa_index, r);
    // four tasks a round, their loads - positions, row numbers, rows - issued before the first is
    // used; a task's head does not change from round to round when heads divides per_block, and q's
    // chunk is then read once
    const bool q_once = per_block % A.heads == 0 && A.chunks_a <= A.la;
    float q1[4] = {0.f, 0.f, 0.f, 0.f};
    if (q_once && l < A.chunks_a) LoadChunk(A.qa, qrow * A.da + (sub % A.heads) * A.dha + (int64_t)l * va, va, q1);
    for (int64_t t0 = 0; t0 < tasks; t0 += per_block * 4) {
      bool live[4];
      int64_t pos[4], krow[4], hh[4];
      float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t t = t0 + u * per_block + sub;
        live[u] = t < tasks;
        const int64_t p = live[u] ? t / A.heads : 0;
        hh[u] = live[u] ? t - p * A.heads : 0;
        pos[u] = live[u] ? pos_of(b + p) : 0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) krow[u] = live[u] ? RowOf(A, A.ka, pos[u]) : 0;
      for (int64_t j = l; j < A.chunks_a; j += A.la) {
        Raw rk[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (live[u]) rk[u] = LoadRaw<M>(A.ka, krow[u] * A.da + hh[u] * A.dha + j * va, va);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (live[u]) {
            float qv[4], kv[4];
            if (q_once) { qv[0] = q1[0]; qv[1] = q1[1]; qv[2] = q1[2]; qv[3] = q1[3]; }
            else LoadChunk(A.qa, qrow * A.da + hh[u] * A.dha + j * va, va, qv);
            WidenRaw<M>(rk[u], kv);
            s[u] = ChunkDot(qv, kv, va, s[u]);
          }
        }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        if (off < A.la) {
#pragma unroll
          for (int u = 0; u < 4; ++u) s[u] = MpwAdd(s[u], __shfl_xor(s[u], off));
        }
      }
      if (l == 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (live[u]) {
            const int64_t at = pos[u] * A.heads + hh[u];
            float v = s[u];
            if (!GRAD) {
              v = AttDotLogit(v, A.scale);
              if (A.logits) A.logits[at] = v;
            }
            A.buf[at] = v;
          }
        }
      }
    }
  } else {
    for (int64_t t = threadIdx.x; t < tasks; t += kSmxBlock) {
      const int64_t p = t / A.heads, h = t - p * A.heads;
      const int64_t pos = PosOf(A, b + p);
      const float qs = A.sq.p ? LoadWide(A.sq.p, A.sq.dt, IndexedRow(A.sq, A.sq_index, r) * A.heads + h) : 0.f;
      const float x = AttAdditiveLogit(qs, LoadWide(A.sk.p, A.sk.dt, RowOf(A, A.sk, pos) * A.heads + h), A.slope);
      if (A.logits) A.logits[pos * A.heads + h] = x;
      A.buf[pos * A.heads + h] = x;
    }
  }
  __syncthreads();
  // ---- B ----
  if (n > kSmxShort) {
    const int32_t units = hc == 1 ? A.heads : 1;
    for (int32_t u = 0; u < units; ++u) LongSoftmaxUnit<GRAD>(A, r, b, n, u, hc, red);
  } else if (n > 0) {
    for (int64_t h = threadIdx.x; h < A.heads; h += kSmxBlock) {
      float x[kSmxShort], a[kSmxShort], y[kSmxShort];
#pragma unroll
      for (int k = 0; k < kSmxShort; ++k) {
        x[k] = a[k] = y[k] = 0.f;
        if (k < n) {
          const int64_t i = PosOf(A, b + k) * A.heads + h;
          x[k] = A.buf[i];
          if (GRAD) a[k] = A.alpha_in[i];
        }
      }
      if (!GRAD) SmxShortForward<kSmxShort>(x, (int32_t)n, y);
      else SmxShortBackward<kSmxShort>(a, x, (int32_t)n, y);
      float qs = 0.f;
      if (GRAD && A.kind == kAttAdditive && A.sq.p)
        qs = LoadWide(A.sq.p, A.sq.dt, IndexedRow(A.sq, A.sq_index, r) * A.heads + h);
#pragma unroll
      for (int k = 0; k < kSmxShort; ++k) {
        if (k < n) {
          const int64_t pos = PosOf(A, b + k);
          float v = y[k];
          if (GRAD) {
            const float ks = A.kind == kAttAdditive ? LoadWide(A.sk.p, A.sk.dt, RowOf(A, A.sk, pos) * A.heads + h) : 0.f;
            v = GradOfLogit(A, v, qs, ks);
          }
          A.buf[pos * A.heads + h] = v;
        }
      }
    }
  }
  __syncthreads();
  // ---- C: a column per lane, the updates in increasing p, eight loads in flight ----
  if (GRAD && A.kind == kAttAdditive) {
    for (int64_t h = threadIdx.x; h < A.heads; h += kSmxBlock) {
      float s = 0.f;
      for (int64_t p = 0; p < n; ++p) s = MpwAdd(s, A.buf[PosOf(A, b + p) * A.heads + h]);
      StoreNarrow(A.out, A.out_dt, r * A.heads + h, s);
    }
  } else {
    for (int64_t c = threadIdx.x; c < A.dc; c += kSmxBlock) {
      const int64_t hd = c / A.dhc;
      float acc = 0.f;
      int64_t p = 0;
      for (; p + 8 <= n; p += 8) {
        int64_t pos[8], row[8];
        float f[8], w[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) pos[q] = pos_of(b + p + q);
#pragma unroll
        for (int q = 0; q < 8; ++q) { row[q] = RowOf(A, A.vc, pos[q]); w[q] = A.buf[pos[q] * A.heads + hd]; }
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = LoadWideM<M>(A.vc, row[q] * A.dc + c);
#pragma unroll
        for (int q = 0; q < 8; ++q) acc = AttFold(acc, f[q], w[q]);
      }
      for (; p < n; ++p) {
        const int64_t pos = pos_of(b + p);
        acc = AttFold(acc, LoadWideM<M>(A.vc, RowOf(A, A.vc, pos) * A.dc + c), A.buf[pos * A.heads + hd]);
      }
      StoreNarrow(A.out, A.out_dt, r * A.dc + c, acc);
    }
  }
  __syncthreads();
}

// gridDim.x chunks of 256 destinations, gridDim.y blocks share the chosen ones of a chunk:
// every destination (all), or those with more than 32 updates
template <bool GRAD, int M>
__global__ __launch_bounds__(kSmxBlock) void SegAttLongKernel(const AttArgs A, const int32_t hc, const bool all) {
  __shared__ unsigned long long masks[4];
  __shared__ float red[2][4][64];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t base = (int64_t)blockIdx.x * kSmxBlock; base < A.seg.size; base += (int64_t)gridDim.x * kSmxBlock) {
    const int64_t r = base + threadIdx.x;
    bool chosen = false;
    if (r < A.seg.size) {
      int64_t b, en;
      ClampedBounds(A, r, &b, &en);
      chosen = all || en - b > kSmxShort;
    }
    const unsigned long long my = __ballot(chosen);
    if (lane == 0) masks[wave] = my;
    __syncthreads();
    uint32_t seen = 0;
    for (int32_t wv = 0; wv < 4; ++wv) {
      unsigned long long mk = masks[wv];
      while (mk) {
        const int32_t bit = __ffsll((long long)mk) - 1;
        mk &= mk - 1;
        if (seen++ % gridDim.y != blockIdx.y) continue;
        LongDestination<GRAD, M>(A, base + wv * 64 + bit, hc, red);
      }
    }
    __syncthreads();                                    // masks are free again
  }
  const int64_t block = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  ZeroOutside(A, block * kSmxBlock + threadIdx.x, (int64_t)gridDim.x * gridDim.y * kSmxBlock);
}

Table MakeTable(const void* p, int32_t dt, int64_t rows) {
  const uintptr_t align = dt == EULER_GPU_F32 ? 16 : 8;
  return Table{p, dt, (uint32_t)(rows > 0 ? rows - 1 : 0), (uintptr_t)p % align == 0};
}

// whether SegAttShortKernel serves a shape: every head's lanes in one group of a wave, a chunk a lane
bool ShortServes(int32_t heads, int64_t dh_a, bool dot_a) {
  if (heads > 64) return false;
  if (!dot_a) return true;
  return (int64_t)heads * AttLanes(dh_a) <= 64 && dh_a / AttChunk(dh_a) <= 64;
}

template <int K, bool GRAD, int M>
void LaunchShortM(hipStream_t st, const AttArgs& A, bool shared, unsigned blocks) {
  if (shared) hipLaunchKernelGGL((SegAttShortKernel<K, GRAD, true, M>), dim3(blocks), dim3(256), 0, st, A);
  else hipLaunchKernelGGL((SegAttShortKernel<K, GRAD, false, M>), dim3(blocks), dim3(256), 0, st, A);
}

template <int K, bool GRAD>
void LaunchShort(hipStream_t st, const AttArgs& A, bool shared, int32_t mode, unsigned blocks) {
  if (mode == 1) LaunchShortM<K, GRAD, 1>(st, A, shared, blocks);
  else if (mode == 2) LaunchShortM<K, GRAD, 2>(st, A, shared, blocks);
  else if (mode == 3) LaunchShortM<K, GRAD, 3>(st, A, shared, blocks);
  else LaunchShortM<kSmxShort, GRAD, 0>(st, A, shared, blocks);      // (one K for the general mode)
}

// the short kernel's load mode (above SegAttShortKernel): 1 + the storage type when every gathered
// table the call reads has that type, 4-column chunks and the alignment for them, and there is no perm
int32_t ShortMode(const AttArgs& A, bool dot_a, bool rows_c) {
  if (A.perm) return 0;
  int32_t dt = -1;
  const auto one = [&](const Table& t, bool chunks) {
    if (dt < 0) dt = t.dt;
    return t.dt == dt && (!chunks || t.vec);
  };
  bool ok = true;
  if (dot_a) ok = ok && A.va == 4 && one(A.ka, true);
  if (rows_c) ok = ok && A.vcv == 4 && one(A.vc, true);
  if (A.kind == kAttAdditive) ok = ok && one(A.sk, false);
  return ok && dt >= 0 ? 1 + dt : 0;
}

// fills the lane layout of A and launches: the short kernel where it serves the shape, the long
// one for what is left
template <bool GRAD>
int Launch(hipStream_t st, AttArgs A, bool uniform, int64_t count) {
  const bool dot_a = GRAD || A.kind == kAttDot;
  A.dha = dot_a ? A.da / A.heads : 1;
  A.va = dot_a ? AttChunk(A.dha) : 1;
  A.chunks_a = (int32_t)(dot_a ? A.dha / A.va : 1);
  A.la = dot_a ? AttLanes(A.dha) : 1;
  const bool rows_c = !(GRAD && A.kind == kAttAdditive);
  A.dhc = rows_c ? A.dc / A.heads : 1;
  A.vcv = rows_c ? AttChunk(A.dhc) : 1;
  A.chunks_c = rows_c ? A.dc / A.vcv : 0;
  const bool shared = rows_c && dot_a && A.ka.p == A.vc.p && A.ka.dt == A.vc.dt && A.da == A.dc;
  const bool short_ok = ShortServes(A.heads, A.dha, dot_a);
  if (A.seg.size == 0) {                                // every update is outside
    if (A.buf && A.e > 0) EG_HIP(hipMemsetAsync(A.buf, 0, (size_t)A.e * A.heads * sizeof(float), st));
    return EULER_GPU_OK;
  }
  int32_t log_g = 0;
  if (short_ok) {
    const int64_t lanes = std::max<int64_t>((int64_t)A.heads * A.la, std::min<int64_t>(64, A.chunks_c));
    while ((1 << log_g) < lanes) ++log_g;
  }
  A.log_g = log_g;
  const bool run_short = short_ok && (!uniform || count <= kSmxShort);
  const bool run_long = A.seg.size > 0 && !(run_short && uniform);
  if (run_short && A.seg.size > 0) {
    const int64_t groups_per_block = 256 >> log_g;
    int64_t blocks = ((int64_t)A.seg.size + groups_per_block - 1) / groups_per_block;
    blocks = blocks < 1 ? 1 : (blocks > 256 * 64 ? 256 * 64 : blocks);
    const int32_t mode = ShortMode(A, dot_a, rows_c);
    if (uniform && count <= 16) LaunchShort<16, GRAD>(st, A, shared, mode, (unsigned)blocks);
    else LaunchShort<kSmxShort, GRAD>(st, A, shared, mode, (unsigned)blocks);
    EG_HIP(hipGetLastError());
  }
  if (run_long) {
    const SmxLongGrid g = SmxLongGridFor(A.seg.size);
    const dim3 grid(g.chunks, g.share);
    const int32_t hc = SmxHeadsPerWave(A.heads);
    switch (ShortMode(A, dot_a, rows_c)) {                // (the same load modes)
      case 1: hipLaunchKernelGGL((SegAttLongKernel<GRAD, 1>), grid, dim3(kSmxBlock), 0, st, A, hc, !run_short); break;
      case 2: hipLaunchKernelGGL((SegAttLongKernel<GRAD, 2>), grid, dim3(kSmxBlock), 0, st, A, hc, !run_short); break;
      case 3: hipLaunchKernelGGL((SegAttLongKernel<GRAD, 3>), grid, dim3(kSmxBlock), 0, st, A, hc, !run_short); break;
      default: hipLaunchKernelGGL((SegAttLongKernel<GRAD, 0>), grid, dim3(kSmxBlock), 0, st, A, hc, !run_short);
    }
    EG_HIP(hipGetLastError());
  }
  return EULER_GPU_OK;
}

struct AttCall {
  const char* name;
  int32_t kind;
  const void* q; int32_t q_dt; int64_t q_rows; const int32_t* q_index;
  const void* k; int32_t k_dt; int64_t k_rows;
  const void* v; int32_t v_dt; int64_t v_rows;
  const void* gather; int32_t gather_is_ids;
  int64_t count, e, d, dv;
  int32_t heads, size;
  float scale, slope;
};

// the argument ladder both entries share (dst: the call's destinations); *nothing: OK and nothing to launch
int CheckCall(const AttCall& c, const SegDest& dst, bool* nothing) {
  const std::string w(c.name);
  *nothing = false;
  if (c.kind != kAttDot && c.kind != kAttAdditive) return Fail(EULER_GPU_EINVAL, w + ": kind is 0 (dot) or 1 (additive)");
  if (!KnownDtype(c.k_dt) || (c.q && !KnownDtype(c.q_dt)) || (c.v && !KnownDtype(c.v_dt)))
    return Fail(EULER_GPU_EINVAL, w + ": unknown dtype" + kDtypeCodes);
  if (c.heads < 1) return Fail(EULER_GPU_EINVAL, w + ": heads < 1");
  if (c.e < 0 || c.size < 0 || c.count < 0 || c.d < 0 || c.dv < 0) return Fail(EULER_GPU_EINVAL, w + ": bad shape");
  if (c.kind == kAttAdditive ? c.d != c.heads : c.d % c.heads != 0)
    return Fail(EULER_GPU_EINVAL, w + ": d is heads (additive) or a multiple of heads (dot)");
  if (c.dv % c.heads != 0) return Fail(EULER_GPU_EINVAL, w + ": heads must divide dv");
  if (c.kind == kAttAdditive && !c.v) return Fail(EULER_GPU_EINVAL, w + ": additive attention needs v");
  if (!c.v && c.dv != c.d) return Fail(EULER_GPU_EINVAL, w + ": without v, dv is d");
  if (const char* why = dst.FormError()) return Fail(EULER_GPU_EINVAL, w + ": " + why);
  if (c.size == 0 && c.e == 0) { *nothing = true; return EULER_GPU_OK; }
  if (const char* why = dst.LengthError()) return Fail(EULER_GPU_EINVAL, w + ": " + why);
  if (c.e > 0 && (!c.k || !c.gather)) return Fail(EULER_GPU_EINVAL, w + ": null buffer");
  if (c.e > 0 && (c.k_rows < 1 || (c.v && c.v_rows < 1) || c.k_rows >= (1LL << 31) || c.v_rows >= (1LL << 31)))
    return Fail(EULER_GPU_EINVAL, w + ": a table has no rows, or 2^31 or more");
  if (c.kind == kAttDot && c.e > 0 && c.size > 0 && (!c.q || c.q_rows < 1))
    return Fail(EULER_GPU_EINVAL, w + ": dot attention needs q");
  if (c.q && c.q_rows < 1 && c.size > 0) return Fail(EULER_GPU_EINVAL, w + ": q has no rows");
  return EULER_GPU_OK;
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_segment_attention(void* stream, int32_t kind, const void* q_dev, int32_t q_dtype, int64_t q_rows,
                                const int32_t* q_index_dev, const void* k_dev, int32_t k_dtype, int64_t k_rows,
                                const void* v_dev, int32_t v_dtype, int64_t v_rows, const void* gather_dev,
                                int32_t gather_is_ids, const int32_t* indices_dev, const int64_t* seg_ptr_dev,
                                int64_t count, int64_t e, int64_t d, int64_t dv, int32_t heads, int32_t size,
                                float scale, float negative_slope, void* out_dev, int32_t out_dtype,
                                float* alpha_dev, float* logits_dev) {
  const AttCall c{"segment_attention", kind, q_dev, q_dtype, q_rows, q_index_dev, k_dev, k_dtype, k_rows,
                  v_dev, v_dtype, v_rows, gather_dev, gather_is_ids, count, e, d, dv, heads, size, scale, negative_slope};
  hipStream_t st = (hipStream_t)stream;
  SegDest dst(st, indices_dev, seg_ptr_dev, count, e, size);
  bool nothing;
  int rc = CheckCall(c, dst, &nothing);
  if (rc != EULER_GPU_OK || nothing) return rc;
  if (!KnownDtype(out_dtype)) return Fail(EULER_GPU_EINVAL, "segment_attention: unknown out_dtype");
  if (size > 0 && dv > 0 && !out_dev) return Fail(EULER_GPU_EINVAL, "segment_attention: null buffer");
  if ((rc = dst.Resolve()) != EULER_GPU_OK) return rc;
  StreamBuf stage(st);
  AttArgs A{};
  A.kind = kind;
  A.qa = MakeTable(q_dev, q_dtype, q_rows); A.qa_index = q_index_dev; A.da = d;
  A.ka = MakeTable(k_dev, k_dtype, k_rows);
  A.sq = A.qa; A.sq_index = q_index_dev; A.sk = A.ka;
  A.vc = v_dev ? MakeTable(v_dev, v_dtype, v_rows) : A.ka; A.dc = dv;
  A.gsrc = static_cast<const int32_t*>(gather_dev); A.gstride = gather_is_ids ? 2 : 1;
  A.seg = dst.seg(); A.perm = dst.perm(); A.e = e; A.heads = heads;
  A.scale = scale; A.slope = negative_slope;
  A.buf = alpha_dev; A.logits = logits_dev;
  A.out = out_dev; A.out_dt = out_dtype;
  A.out_vec = (uintptr_t)out_dev % (out_dtype == EULER_GPU_F32 ? 16 : 8) == 0;
  // the long path keeps its logits in the alpha buffer: stage one when the caller wants none
  const bool uniform = count > 0;
  const bool short_only = uniform && count <= kSmxShort && ShortServes(heads, d / heads, kind == kAttDot);
  if (!A.buf && !short_only && e > 0) {
    if (stage.alloc((size_t)e * heads * sizeof(float)) != hipSuccess)
      return Fail(EULER_GPU_ENOMEM, "segment_attention: no memory for the staged logits");
    A.buf = stage.as<float>();
  }
  return Launch<false>(st, A, uniform, count);
}

int euler_gpu_segment_attention_grad(void* stream, int32_t kind, const void* q_dev, int32_t q_dtype, int64_t q_rows,
                                     const int32_t* q_index_dev, const void* k_dev, int32_t k_dtype,
                                     int64_t k_rows, const void* v_dev, int32_t v_dtype, int64_t v_rows,
                                     const void* gather_dev, int32_t gather_is_ids, const int32_t* indices_dev,
                                     const int64_t* seg_ptr_dev, int64_t count, int64_t e, int64_t d, int64_t dv,
                                     int32_t heads, int32_t size, float scale, float negative_slope,
                                     const float* alpha_dev, const void* grad_dev, int32_t grad_dtype,
                                     float* ds_dev, float* dq_dst_dev) {
  const AttCall c{"segment_attention_grad", kind, q_dev, q_dtype, q_rows, q_index_dev, k_dev, k_dtype, k_rows,
                  v_dev, v_dtype, v_rows, gather_dev, gather_is_ids, count, e, d, dv, heads, size, scale, negative_slope};
  hipStream_t st = (hipStream_t)stream;
  SegDest dst(st, indices_dev, seg_ptr_dev, count, e, size);
  bool nothing;
  int rc = CheckCall(c, dst, &nothing);
  if (rc != EULER_GPU_OK || nothing) return rc;
  if (!KnownDtype(grad_dtype)) return Fail(EULER_GPU_EINVAL, "segment_attention_grad: unknown grad dtype");
  if ((e > 0 && (!alpha_dev || !ds_dev)) || (size > 0 && d > 0 && !dq_dst_dev) || (size > 0 && dv > 0 && !grad_dev))
    return Fail(EULER_GPU_EINVAL, "segment_attention_grad: null buffer");
  if ((rc = dst.Resolve()) != EULER_GPU_OK) return rc;
  const Table tk = MakeTable(k_dev, k_dtype, k_rows);
  AttArgs A{};
  A.kind = kind;
  A.qa = MakeTable(grad_dev, grad_dtype, size); A.qa_index = nullptr; A.da = dv;
  A.ka = v_dev ? MakeTable(v_dev, v_dtype, v_rows) : tk;
  A.sq = MakeTable(q_dev, q_dtype, q_rows); A.sq_index = q_index_dev; A.sk = tk;
  A.vc = tk; A.dc = d;
  A.gsrc = static_cast<const int32_t*>(gather_dev); A.gstride = gather_is_ids ? 2 : 1;
  A.seg = dst.seg(); A.perm = dst.perm(); A.e = e; A.heads = heads;
  A.scale = scale; A.slope = negative_slope;
  A.alpha_in = alpha_dev; A.buf = ds_dev; A.logits = nullptr;
  A.out = dq_dst_dev; A.out_dt = EULER_GPU_F32;
  A.out_vec = (uintptr_t)dq_dst_dev % 16 == 0;
  return Launch<true>(st, A, count > 0, count);
}

}  // extern "C"
