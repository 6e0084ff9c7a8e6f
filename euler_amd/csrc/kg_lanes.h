// The lane helpers of the triple-scoring kernels (kg_score_kernels.hip, kg_proj_kernels.hip,
// kg_matrix_kernels.hip): what one lane of a task sees of a table row, of an fp32 output row and
// of its gy, the butterfly over the lanes of a task, and the steps every family's kernels take
// the same way - ss and inv of a row, the slot of a negative's score and the
// front / tail corruption of one negative, forward and gradient.  Device code only; the
// arithmetic itself is in kg_score.h / kg_proj.h / kg_matrix.h.
#pragma once

#include <hip/hip_runtime.h>

#include "device_fns.h"
#include "half_cvt.h"
#include "kg_score.h"

namespace euler_gpu {
namespace {

// V adjacent elements of a table, widened: 16-byte loads where the type and V allow
template <int DT, int V>
__device__ __forceinline__ void KgLoadChunk(const void* base, int64_t at, float f[V]) {
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

// What a lane sees of one table row (the Row of kg_score.h).  REG: its one chunk, loaded once.
template <int DT, int V, bool REG>
struct LaneRow {
  const void* base;
  int64_t at;
  bool ok;
  float x[REG ? V : 1];
  __device__ __forceinline__ void Open(const void* table, int64_t id, int64_t rows, int64_t d, int32_t l,
                                       int32_t chunks) {
    base = table;
    ok = KgInRange(id, rows);
    at = ok ? id * d : 0;
    if constexpr (REG) {
      if (ok && l < chunks) {
        KgLoadChunk<DT, V>(base, at + (int64_t)l * V, x);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) x[k] = 0.f;
      }
    }
  }
  __device__ __forceinline__ void Chunk(int32_t j, float f[V]) const {
    if constexpr (REG) {
#pragma unroll
      for (int k = 0; k < V; ++k) f[k] = x[k];
    } else if (ok) {
      KgLoadChunk<DT, V>(base, at + (int64_t)j * V, f);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) f[k] = 0.f;
    }
  }
};

// A lane's columns of one fp32 output row; `on` is false for a task past the end.
// vec: the row starts on a 16-byte boundary (V >= 4 has d % 4 == 0).
template <int V>
struct LaneOut {
  float* p;
  bool on, vec;
  __device__ __forceinline__ void Get(int32_t j, float f[V]) const {
    if (!on) {
#pragma unroll
      for (int k = 0; k < V; ++k) f[k] = 0.f;
      return;
    }
    const float* q = p + (int64_t)j * V;
    if constexpr (V >= 4) {
      if (vec) {
#pragma unroll
        for (int i = 0; i < V / 4; ++i) {
          const float4 v = reinterpret_cast<const float4*>(q)[i];
          f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
        }
        return;
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) f[k] = q[k];
  }
  __device__ __forceinline__ void Put(int32_t j, const float f[V]) {
    if (!on) return;
    float* q = p + (int64_t)j * V;
    if constexpr (V >= 4) {
      if (vec) {
#pragma unroll
        for (int i = 0; i < V / 4; ++i)
          reinterpret_cast<float4*>(q)[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
        return;
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) q[k] = f[k];
  }
};

// A lane's gy of one row (the Acc of kg_score.h): registers (REG) or the lane's own columns of
// the output row, which only this lane reads and writes.
template <int V, bool REG>
struct LaneAcc {
  LaneOut<V> mem;
  float g[REG ? V : 1];
  __device__ __forceinline__ void Open(const LaneOut<V>& row, int32_t l, int32_t lanes, int32_t chunks) {
    mem = row;
    if constexpr (REG) {
#pragma unroll
      for (int k = 0; k < V; ++k) g[k] = 0.f;
    } else {
      float z[V];
#pragma unroll
      for (int k = 0; k < V; ++k) z[k] = 0.f;
      for (int32_t j = l; j < chunks; j += lanes) mem.Put(j, z);
    }
  }
  __device__ __forceinline__ void Get(int32_t j, float f[V]) const {
    if constexpr (REG) {
#pragma unroll
      for (int k = 0; k < V; ++k) f[k] = g[k];
    } else {
      mem.Get(j, f);
    }
  }
  __device__ __forceinline__ void Put(int32_t j, const float f[V]) {
    if constexpr (REG) {
#pragma unroll
      for (int k = 0; k < V; ++k) g[k] = f[k];
    } else {
      mem.Put(j, f);
    }
  }
};

// the butterfly over the L lanes of a task; every lane of the wave takes part
__device__ __forceinline__ float KgCombine(float s, int32_t lanes) {
  for (int32_t off = lanes >> 1; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off));
  return s;
}

// ss and inv of a row
template <int V, typename Row>
__device__ __forceinline__ void KgLaneNorm(const Row& x, bool normalize, int32_t l, int32_t lanes, int32_t chunks,
                                           float* ss, float* inv) {
  *ss = normalize ? KgCombine(KgLaneSumSq<V>(x, l, lanes, chunks), lanes) : 0.f;
  *inv = KgInv(*ss, normalize);
}

// Where the score of negative k of triple t stands in neg_out / g_neg: [b, k_total] front or tail
// scores, for corrupt "both" [b, 2 * k_total] with the tail scores behind the front ones
__device__ __forceinline__ int64_t KgNegSlot(int32_t corrupt, int64_t k_total, int64_t t, int64_t k, bool tail) {
  const int64_t kp = corrupt == kKgBoth ? 2 * k_total : k_total;
  return t * kp + (tail && corrupt == kKgBoth ? k_total : 0) + k;
}

// The corruption of a triple (h, r, t) by one negative n: the front score s(n, r, t) and / or the
// tail score s(h, r, n), as `corrupt` asks.  The caller stores them: put(tail, score), each as
// soon as it is known.
template <int V, typename Ent, typename Rel, typename Put>
__device__ __forceinline__ void KgLaneCorrupt(int32_t kind, int32_t corrupt, const Ent& h, float ih, const Rel& r,
                                              float ir, const Ent& t, float it, const Ent& n, float in, int32_t l,
                                              int32_t lanes, int32_t chunks, Put put) {
  if (corrupt != kKgTail)
    put(false, KgFinish(kind, KgCombine(KgLaneScore<V>(kind, n, in, r, ir, t, it, l, lanes, chunks), lanes)));
  if (corrupt != kKgFront)
    put(true, KgFinish(kind, KgCombine(KgLaneScore<V>(kind, h, ih, r, ir, n, in, l, lanes, chunks), lanes)));
}

// Its gradient: g(tail), the incoming gradient of each of the two scores, into the gy of the rows
// that score read.  trans_l2 needs the score again.
template <int V, typename Ent, typename Rel, typename Acc, typename G>
__device__ __forceinline__ void KgLaneCorruptGrad(int32_t kind, int32_t corrupt, G g, const Ent& h, float ih,
                                                  const Rel& r, float ir, const Ent& t, float it, const Ent& n,
                                                  float in, Acc& gh, Acc& gr, Acc& gt, Acc& gn, int32_t l,
                                                  int32_t lanes, int32_t chunks) {
  const bool l2 = kind == kKgTransL2;
  if (corrupt != kKgTail) {
    const float s = l2 ? KgCombine(KgLaneScore<V>(kind, n, in, r, ir, t, it, l, lanes, chunks), lanes) : 0.f;
    KgLaneScoreGrad<V>(kind, KgScale(kind, g(false), s), n, in, r, ir, t, it, gn, gr, gt, l, lanes, chunks);
  }
  if (corrupt != kKgFront) {
    const float s = l2 ? KgCombine(KgLaneScore<V>(kind, h, ih, r, ir, n, in, l, lanes, chunks), lanes) : 0.f;
    KgLaneScoreGrad<V>(kind, KgScale(kind, g(true), s), h, ih, r, ir, n, in, gh, gr, gn, l, lanes, chunks);
  }
}

}  // namespace
}  // namespace euler_gpu
