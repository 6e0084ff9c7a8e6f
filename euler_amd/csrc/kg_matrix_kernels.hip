// Fused triple scoring with TransR's per-relation matrix projection on gfx950 and its gradient,
// with their C-ABI entry points.  The composition looks up one [de, dr] matrix per triple, tiles
// it over the negatives and runs a batched [1, de] x [de, dr] product per entity row; here the
// triples are worked on in an order grouped by relation (the caller's stable sort), a workgroup
// takes a fixed number of consecutive triples of that order and stages M_rho in LDS, tiled over
// its rows c, once per run of equal relation in its share.  The arithmetic, the range rule and
// every summation order are stated in kg_matrix.h and kg_score.h, which the host check compiles
// too; no order depends on the grouping, the tiling or the grid.  No float atomics, no MFMA.
// The argument ladder is kg_entry.h's (MatrixCall states what this family adds); the entries keep
// the rules of the segments and of the gz / G_M buffers.
//
//   TripleScoreMatrixKernel          forward.  A triple is a task of L lanes of a wave, as in
//       kg_score_kernels.hip; a lane owns the columns of its chunks of the dr columns (at most 8,
//       KgmRegs) and adds x_c * M[c, j] over c for four entity rows at once (h, t and the first
//       two negatives, then the negatives four at a time), reading M from the LDS tile.  The dr-sums are
//       KgLaneSumSq / KgLaneScore over those registers and the wave butterfly.
//   TripleScoreMatrixGradKernel      recomputes the forward the same way and writes G_rel and the
//       gz rows (the gradient of every projected row before its normalisation).
//   TripleScoreMatrixRowGradKernel   gx = gz . M^T per occurrence: a lane owns one row c of the
//       LDS tile of M (row stride dr + 1: no bank conflict) and walks j in order; the 16 lanes
//       of a row slot load the gz row together and pass its columns round.
//   TripleScoreMatrixTableGradKernel G_M: one grid cell per (segment, 16 x 64 tile of G_M); a lane
//       owns four [c, j] elements and walks the segment's occurrences in the stated order, x and
//       gz staged in LDS 128 rows at a time.  Every element is one sequential sum, written once.
//
// A launch fixes the share of a workgroup from b and rel_rows alone (Launch below): a batch with
// few triples a relation takes one wave a workgroup, so that its many one-task runs spread out.
// Positions read from `order` and `seg_ptr` come from the caller: a position outside [0, b)
// names no triple and is skipped, so a wrong order cannot make a kernel leave its buffers.
// Every loop that holds a barrier has a block-uniform trip count; a loop that holds a shuffle has
// the same trip count in all the lanes that exchange (a task's lanes, a row slot's 16 lanes).
#include <hip/hip_runtime.h>

#include "device_fns.h"
#include "device_mem.h"
#include "half_cvt.h"
#include "kg_entry.h"
#include "kg_lanes.h"
#include "kg_matrix.h"

namespace euler_gpu {
namespace {

constexpr int kKgmTileFloats = 8192;              // the LDS tile of M of the per-triple kernels: 32 KiB
constexpr int kKgmMaxShare = 256;                 // triples of a workgroup's share (L = 1)
constexpr int kKgmGxRows = 16;                    // rows c of M in the tile of the gx kernel
constexpr int kKgmGxShare = 16;                   // triples of a workgroup's share of the gx kernel, at most
constexpr int kKgmGmC = 16, kKgmGmJ = 64;         // the tile of G_M of a grid cell
constexpr int kKgmGmBatch = 128;                  // occurrence rows staged at a time
constexpr int64_t kKgmMaxBlocks = 2048;           // 8 workgroups a CU

struct KgmArgs : KgTripleArgs {                   // out_vec: g_rel and the gz buffers start on 16 bytes
  int32_t ent_dt, rel_dt, mat_dt;
  int64_t de, dr;
  const void* matrix;
  const int64_t* order;
  const int64_t* seg_ptr; const int64_t* seg_rel; int64_t nseg;                  // gradient
  float* gz_src; float* gz_dst; float* gz_neg_rows;
  void* g_matrix;
  int32_t gx_share;                               // triples of a workgroup's share of the gx kernel
};

// one element of a table of run-time dtype, widened exactly
__device__ __forceinline__ float KgmLoad(const void* base, int32_t dt, int64_t at) {
  if (dt == kF32) return static_cast<const float*>(base)[at];
  const uint16_t w = static_cast<const uint16_t*>(base)[at];
  return dt == kBF16 ? HalfCvt<kBF16>::Widen(w) : HalfCvt<kF16>::Widen(w);
}

__device__ __forceinline__ void KgmStore(void* base, int32_t dt, int64_t at, float v) {
  if (dt == kF32) static_cast<float*>(base)[at] = v;
  else static_cast<uint16_t*>(base)[at] = dt == kBF16 ? HalfCvt<kBF16>::Narrow(v) : HalfCvt<kF16>::Narrow(v);
}

// What a lane sees of rel[rho] (the Row of kg_score.h) for a run-time dtype
template <int V>
struct KgmRelRow {
  const void* base;
  int64_t at;
  int32_t dt;
  bool ok;
  __device__ __forceinline__ void Chunk(int32_t j, float f[V]) const {
    if (!ok) {
#pragma unroll
      for (int k = 0; k < V; ++k) f[k] = 0.f;
    } else if (dt == kF32) {
      KgLoadChunk<kF32, V>(base, at + (int64_t)j * V, f);
    } else if (dt == kBF16) {
      KgLoadChunk<kBF16, V>(base, at + (int64_t)j * V, f);
    } else {
      KgLoadChunk<kF16, V>(base, at + (int64_t)j * V, f);
    }
  }
};

// The relation key of triple t: its rel_id, or R for one that names no relation
__device__ __forceinline__ int64_t KgmKey(const KgmArgs& a, int64_t t) {
  const int64_t rho = a.rel_id[t];
  return KgInRange(rho, a.rel_rows) ? rho : a.rel_rows;
}

// The share [p0, p0 + n) of the grouped order into LDS: the triple of every position (-1 where
// `order` names none) and its key.  Barriers are the caller's.
__device__ __forceinline__ void KgmLoadShare(const KgmArgs& a, int64_t p0, int32_t n, int32_t* s_idx, int64_t* s_key) {
  for (int32_t i = threadIdx.x; i < n; i += blockDim.x) {
    const int64_t t = a.order[p0 + i];
    const bool ok = t >= 0 && t < a.b;
    s_idx[i] = ok ? (int32_t)t : -1;
    s_key[i] = ok ? KgmKey(a, t) : a.rel_rows;
  }
}

// The end of the run of equal keys that starts at position p of the share
__device__ __forceinline__ int32_t KgmRunEnd(const int64_t* s_key, int32_t p, int32_t n) {
  const int64_t rho = s_key[p];
  int32_t q = p + 1;
  while (q < n && s_key[q] == rho) ++q;
  return q;
}

// Rows [c0, c0 + tc) of M_rho, widened, into LDS as one flat copy (the rows are adjacent in M and
// in the tile); +0 for rho == R.  sm is 16-byte aligned.
__device__ __forceinline__ void KgmLoadTile(const KgmArgs& a, int64_t rho, int32_t c0, int32_t tc, float* sm) {
  const int32_t n = tc * (int32_t)a.dr;
  const int64_t base = (rho * a.de + c0) * a.dr;
  if (rho >= a.rel_rows) {
    for (int32_t i = threadIdx.x; i < n; i += blockDim.x) sm[i] = 0.f;
  } else if (a.mat_dt == kF32) {
    const float* src = static_cast<const float*>(a.matrix) + base;
    int32_t done = 0;
    if (((uintptr_t)src & 15) == 0) {
      const int32_t n4 = n >> 2;
#pragma unroll 4
      for (int32_t i = threadIdx.x; i < n4; i += blockDim.x)
        reinterpret_cast<float4*>(sm)[i] = reinterpret_cast<const float4*>(src)[i];
      done = n4 << 2;
    }
#pragma unroll 4
    for (int32_t i = done + threadIdx.x; i < n; i += blockDim.x) sm[i] = src[i];
  } else {
    const uint16_t* src = static_cast<const uint16_t*>(a.matrix) + base;
    const bool bf = a.mat_dt == kBF16;
#pragma unroll 4
    for (int32_t i = threadIdx.x; i < n; i += blockDim.x)
      sm[i] = bf ? HalfCvt<kBF16>::Widen(src[i]) : HalfCvt<kF16>::Widen(src[i]);
  }
}

// The same rows with `stride` floats a row in LDS (the gx kernel: tc <= 16 rows, 16 threads a row)
__device__ __forceinline__ void KgmLoadTilePadded(const KgmArgs& a, int64_t rho, int32_t c0, int32_t tc,
                                                  int32_t stride, float* sm) {
  const int32_t dr = (int32_t)a.dr;
  const int32_t c = threadIdx.x >> 4;
  if (c >= tc) return;
  const bool ok = rho < a.rel_rows;
  const int64_t base = (rho * a.de + c0 + c) * a.dr;
#pragma unroll 4
  for (int32_t j = threadIdx.x & 15; j < dr; j += 16) sm[c * stride + j] = ok ? KgmLoad(a.matrix, a.mat_dt, base + j) : 0.f;
}

constexpr int kKgmRows = 4;                       // entity rows projected in one pass over M
constexpr int kKgmAhead = 4;                      // steps of c whose x are loaded ahead of their use

// z of nr <= kKgmRows entity rows of every task of the share: for each run of equal relation the
// tiles of M_rho pass through LDS once and serve the rows of all the run's tasks.
template <int V>
__device__ __forceinline__ void KgmProject(const KgmArgs& a, int32_t n, int32_t task, const int64_t* s_key, float* sm,
                                           const int64_t ids[kKgmRows], int32_t nr, const int32_t* col,
                                           KgmRegs<V> z[kKgmRows]) {
  const int32_t de = (int32_t)a.de, dr = (int32_t)a.dr;
  const int32_t lanes = 1 << a.log_l, l = threadIdx.x & (lanes - 1);
  const int32_t tc_max = kKgmTileFloats / dr;
  bool ok[kKgmRows];
  int64_t at[kKgmRows];
#pragma unroll
  for (int r = 0; r < kKgmRows; ++r) {
    ok[r] = r < nr && KgInRange(ids[r], a.ent_rows);
    at[r] = ok[r] ? ids[r] * a.de : 0;
  }
  for (int32_t p = 0; p < n;) {
    const int32_t q = KgmRunEnd(s_key, p, n);
    const int64_t rho = s_key[p];
    const bool mine = task >= p && task < q;
    for (int32_t c0 = 0; c0 < de; c0 += tc_max) {
      const int32_t tc = de - c0 < tc_max ? de - c0 : tc_max;
      __syncthreads();
      KgmLoadTile(a, rho, c0, tc, sm);
      __syncthreads();
      if (mine && lanes >= 8) {
        // lane l loads x_{cb + l} of every row - one load serves `lanes` steps, the next group is
        // in flight while this one is used - and the task's lanes pass the value round
        float cur[kKgmRows], nxt[kKgmRows];
#pragma unroll
        for (int r = 0; r < kKgmRows; ++r) cur[r] = ok[r] && l < tc ? KgmLoad(a.ent, a.ent_dt, at[r] + c0 + l) : 0.f;
        for (int32_t cb = 0; cb < tc; cb += lanes) {
#pragma unroll
          for (int r = 0; r < kKgmRows; ++r)
            nxt[r] = ok[r] && cb + lanes + l < tc ? KgmLoad(a.ent, a.ent_dt, at[r] + c0 + cb + lanes + l) : 0.f;
          const int32_t steps = tc - cb < lanes ? tc - cb : lanes;
          for (int32_t u = 0; u < steps; ++u) {
#pragma unroll
            for (int r = 0; r < kKgmRows; ++r) {
              const float x = __shfl(cur[r], u, lanes);
              if (r < nr) KgmStep<V>(z[r], x, sm + (cb + u) * dr, col, c0 + cb + u == 0);
            }
          }
#pragma unroll
          for (int r = 0; r < kKgmRows; ++r) cur[r] = nxt[r];
        }
      } else if (mine) {
        for (int32_t cb = 0; cb < tc; cb += kKgmAhead) {
          float x[kKgmRows][kKgmAhead];
#pragma unroll
          for (int r = 0; r < kKgmRows; ++r) {
#pragma unroll
            for (int u = 0; u < kKgmAhead; ++u)
              x[r][u] = ok[r] && cb + u < tc ? KgmLoad(a.ent, a.ent_dt, at[r] + c0 + cb + u) : 0.f;
          }
#pragma unroll
          for (int u = 0; u < kKgmAhead; ++u) {
            if (cb + u < tc) {
#pragma unroll
              for (int r = 0; r < kKgmRows; ++r) {
                if (r < nr) KgmStep<V>(z[r], x[r][u], sm + (cb + u) * dr, col, c0 + cb + u == 0);
              }
            }
          }
        }
      }
    }
    p = q;
  }
}

// What the two per-triple kernels share of a task: its place, its rel row and z of h and t.  The
// entity rows of a task are numbered h, t, n_0 .. n_{K-1} and projected kKgmRows at a time, so
// h and t share their pass over M with the first two negatives.
template <int V>
struct KgmTask {
  int32_t lanes, l, task, chunks, t;
  bool live;
  int32_t col[kKgmCols / V];
  KgmRelRow<V> R;
  float ssr, ir, ssh, ih, sst, it;
  KgmRegs<V> zh, zt;
  __device__ __forceinline__ void Open(const KgmArgs& a, int32_t n, const int32_t* s_idx) {
    lanes = 1 << a.log_l;
    l = threadIdx.x & (lanes - 1);
    task = threadIdx.x >> a.log_l;
    chunks = (int32_t)(a.dr / V);
    KgmSlots<V>(l, lanes, chunks, col);
    t = task < n ? s_idx[task] : -1;
    live = t >= 0;
    const int64_t rid = live ? a.rel_id[t] : -1;
    R.base = a.rel;
    R.dt = a.rel_dt;
    R.ok = KgInRange(rid, a.rel_rows);
    R.at = R.ok ? rid * a.dr : 0;
    KgLaneNorm<V>(R, true, l, lanes, chunks, &ssr, &ir);
  }
  // z of the entity rows r0 .. r0 + kKgmRows - 1 (those below 2 + K)
  __device__ __forceinline__ void Rows(const KgmArgs& a, int32_t n, const int64_t* s_key, float* sm, int64_t r0,
                                       KgmRegs<V> z[kKgmRows]) const {
    int64_t ids[kKgmRows];
    const int64_t left = a.k + 2 - r0;
    const int32_t nr = left < kKgmRows ? (int32_t)left : kKgmRows;
#pragma unroll
    for (int i = 0; i < kKgmRows; ++i) {
      const int64_t r = r0 + i;
      ids[i] = !live || i >= nr ? -1 : r == 0 ? a.src[t] : r == 1 ? a.dst[t] : a.neg[(int64_t)t * a.k + r - 2];
      z[i].Clear(a.log_l);
    }
    KgmProject<V>(a, n, task, s_key, sm, ids, nr, col, z);
  }
  // h and t from the first pass
  __device__ __forceinline__ void Keep(const KgmRegs<V> z[kKgmRows]) {
    zh = z[0];
    zt = z[1];
    KgLaneNorm<V>(zh, true, l, lanes, chunks, &ssh, &ih);
    KgLaneNorm<V>(zt, true, l, lanes, chunks, &sst, &it);
  }
  template <typename RowA, typename RowC>
  __device__ __forceinline__ float Terms(int32_t kind, const RowA& x, float ix, const RowC& c, float ic) const {
    return KgCombine(KgLaneScore<V>(kind, x, ix, R, ir, c, ic, l, lanes, chunks), lanes);
  }
};

template <int V>
__global__ __launch_bounds__(256) void TripleScoreMatrixKernel(const KgmArgs a) {
  __shared__ __align__(16) float sm[kKgmTileFloats];
  __shared__ int32_t s_idx[kKgmMaxShare];
  __shared__ int64_t s_key[kKgmMaxShare];
  const int32_t share = (int32_t)blockDim.x >> a.log_l;
  for (int64_t p0 = (int64_t)blockIdx.x * share; p0 < a.b; p0 += (int64_t)gridDim.x * share) {
    const int32_t n = a.b - p0 < share ? (int32_t)(a.b - p0) : share;
    __syncthreads();
    KgmLoadShare(a, p0, n, s_idx, s_key);
    __syncthreads();
    KgmTask<V> T;
    T.Open(a, n, s_idx);
    const bool put = T.live && T.l == 0;
    for (int64_t r0 = 0; r0 < a.k + 2; r0 += kKgmRows) {
      KgmRegs<V> z[kKgmRows];
      T.Rows(a, n, s_key, sm, r0, z);
      if (r0 == 0) {
        T.Keep(z);
        const float pos = KgFinish(a.kind, T.Terms(a.kind, T.zh, T.ih, T.zt, T.it));
        if (put) a.pos_out[T.t] = pos;
      }
#pragma unroll
      for (int i = 0; i < kKgmRows; ++i) {
        const int64_t k = r0 + i - 2;
        if (k >= 0 && k < a.k) {
          float ssn, in;
          KgLaneNorm<V>(z[i], true, T.l, T.lanes, T.chunks, &ssn, &in);
          KgLaneCorrupt<V>(a.kind, a.corrupt, T.zh, T.ih, T.R, T.ir, T.zt, T.it, z[i], in, T.l, T.lanes, T.chunks,
                           [&](bool tail, float s) {
                             if (put) a.neg_out[KgNegSlot(a.corrupt, a.k, T.t, k, tail)] = s;
                           });
        }
      }
    }
  }
}

// A projected row whose gy is complete goes through its normalisation: gz -> its output row
template <int V>
__device__ __forceinline__ void KgmThrough(const KgmTask<V>& T, const KgmRegs<V>& z, float ss, float inv,
                                           const KgmRegs<V>& gy, LaneOut<V> out) {
  const float dot = KgCombine(KgLaneDot<V>(z, inv, gy, T.l, T.lanes, T.chunks), T.lanes);
  KgLaneRowGrad<V>(true, true, z, ss, inv, dot, gy, out, T.l, T.lanes, T.chunks);
}

template <int V>
__global__ __launch_bounds__(256) void TripleScoreMatrixGradKernel(const KgmArgs a) {
  __shared__ __align__(16) float sm[kKgmTileFloats];
  __shared__ int32_t s_idx[kKgmMaxShare];
  __shared__ int64_t s_key[kKgmMaxShare];
  const int32_t share = (int32_t)blockDim.x >> a.log_l;
  const bool vec = a.out_vec != 0, l2 = a.kind == kKgTransL2;
  for (int64_t p0 = (int64_t)blockIdx.x * share; p0 < a.b; p0 += (int64_t)gridDim.x * share) {
    const int32_t n = a.b - p0 < share ? (int32_t)(a.b - p0) : share;
    __syncthreads();
    KgmLoadShare(a, p0, n, s_idx, s_key);
    __syncthreads();
    KgmTask<V> T;
    T.Open(a, n, s_idx);
    const bool live = T.live;
    const int64_t tt = live ? T.t : 0;
    KgmRegs<V> gh, gt, gr;
    gh.Clear(a.log_l);
    gt.Clear(a.log_l);
    gr.Clear(a.log_l);
    for (int64_t r0 = 0; r0 < a.k + 2; r0 += kKgmRows) {
      KgmRegs<V> z[kKgmRows];
      T.Rows(a, n, s_key, sm, r0, z);
      if (r0 == 0) {
        T.Keep(z);
        const float s = l2 ? T.Terms(a.kind, T.zh, T.ih, T.zt, T.it) : 0.f;
        const float gs = KgScale(a.kind, live ? a.g_pos[tt] : 0.f, s);
        KgLaneScoreGrad<V>(a.kind, gs, T.zh, T.ih, T.R, T.ir, T.zt, T.it, gh, gr, gt, T.l, T.lanes, T.chunks);
      }
#pragma unroll
      for (int i = 0; i < kKgmRows; ++i) {
        const int64_t k = r0 + i - 2;
        if (k >= 0 && k < a.k) {
          float ssn, in;
          KgLaneNorm<V>(z[i], true, T.l, T.lanes, T.chunks, &ssn, &in);
          KgmRegs<V> gn;
          gn.Clear(a.log_l);
          const auto g = [&](bool tail) { return live ? a.g_neg[KgNegSlot(a.corrupt, a.k, tt, k, tail)] : 0.f; };
          KgLaneCorruptGrad<V>(a.kind, a.corrupt, g, T.zh, T.ih, T.R, T.ir, T.zt, T.it, z[i], in, gh, gr, gt, gn, T.l,
                               T.lanes, T.chunks);
          KgmThrough<V>(T, z[i], ssn, in, gn, LaneOut<V>{a.gz_neg_rows + (tt * a.k + k) * a.dr, live, vec});
        }
      }
    }
    KgmThrough<V>(T, T.zh, T.ssh, T.ih, gh, LaneOut<V>{a.gz_src + tt * a.dr, live, vec});
    KgmThrough<V>(T, T.zt, T.sst, T.it, gt, LaneOut<V>{a.gz_dst + tt * a.dr, live, vec});
    const float dot = KgCombine(KgLaneDot<V>(T.R, T.ir, gr, T.l, T.lanes, T.chunks), T.lanes);
    LaneOut<V> orl{a.g_rel + tt * a.dr, live, vec};
    KgLaneRowGrad<V>(T.R.ok, true, T.R, T.ssr, T.ir, dot, gr, orl, T.l, T.lanes, T.chunks);
  }
}

// The entity id, the gz row and the gx row of occurrence `role` of triple t: the negatives
// 0 .. k - 1, then h (k) and t (k + 1) - the row order of kg_matrix.h
struct KgmOcc {
  int64_t id;
  const float* gz;
  float* gx;
};
__device__ __forceinline__ KgmOcc KgmOccurrence(const KgmArgs& a, int64_t t, int32_t role) {
  if (role < a.k) {
    const int64_t at = t * a.k + role;
    return KgmOcc{a.neg[at], a.gz_neg_rows + at * a.dr, a.g_neg_rows + at * a.de};
  }
  if (role == a.k) return KgmOcc{a.src[t], a.gz_src + t * a.dr, a.g_src + t * a.de};
  return KgmOcc{a.dst[t], a.gz_dst + t * a.dr, a.g_dst + t * a.de};
}

__global__ __launch_bounds__(256) void TripleScoreMatrixRowGradKernel(const KgmArgs a) {
  __shared__ float sm[kKgmGxRows * (kKgMatrixMaxDim + 1)];
  __shared__ int32_t s_idx[kKgmGxShare];
  __shared__ int64_t s_key[kKgmGxShare];
  const int32_t cl = threadIdx.x & (kKgmGxRows - 1), slot = threadIdx.x / kKgmGxRows;
  const int32_t slots = 256 / kKgmGxRows;
  const int32_t de = (int32_t)a.de, dr = (int32_t)a.dr, stride = dr + 1;
  const int32_t per = (int32_t)a.k + 2;
  const int32_t share = a.gx_share;
  for (int64_t p0 = (int64_t)blockIdx.x * share; p0 < a.b; p0 += (int64_t)gridDim.x * share) {
    const int32_t n = a.b - p0 < share ? (int32_t)(a.b - p0) : share;
    __syncthreads();
    KgmLoadShare(a, p0, n, s_idx, s_key);
    __syncthreads();
    for (int32_t p = 0; p < n;) {
      const int32_t q = KgmRunEnd(s_key, p, n);
      const int64_t rho = s_key[p];
      const int64_t rows = (int64_t)(q - p) * per;
      for (int32_t c0 = 0; c0 < de; c0 += kKgmGxRows) {
        const int32_t tc = de - c0 < kKgmGxRows ? de - c0 : kKgmGxRows;
        __syncthreads();
        KgmLoadTilePadded(a, rho, c0, tc, stride, sm);
        __syncthreads();
        {
          // the 16 lanes of a slot walk the same gz row: lane cl loads column jb + cl, one load
          // serves 16 steps, the next group is in flight while this one is used (KgmRowDot's order)
          const float* m = sm + (cl < tc ? cl : 0) * stride;
          for (int64_t row = slot; row < rows; row += slots) {
            const int32_t t = s_idx[p + (int32_t)(row / per)];
            if (t < 0) continue;
            const KgmOcc o = KgmOccurrence(a, t, (int32_t)(row % per));
            float s = 0.f;
            if (KgInRange(o.id, a.ent_rows)) {
              bool first = true;
              float cur = cl < dr ? o.gz[cl] : 0.f;
              for (int32_t jb = 0; jb < dr; jb += kKgmGxRows) {
                const float nxt = jb + kKgmGxRows + cl < dr ? o.gz[jb + kKgmGxRows + cl] : 0.f;
                const int32_t steps = dr - jb < kKgmGxRows ? dr - jb : kKgmGxRows;
                for (int32_t u = 0; u < steps; ++u)
                  KgAcc(__fmul_rn(__shfl(cur, u, kKgmGxRows), m[jb + u]), &s, &first);
                cur = nxt;
              }
            }
            if (cl < tc) o.gx[c0 + cl] = s;
          }
        }
      }
      p = q;
    }
  }
}

__global__ __launch_bounds__(256) void TripleScoreMatrixTableGradKernel(const KgmArgs a) {
  __shared__ __align__(16) float sx[kKgmGmBatch][kKgmGmC];
  __shared__ __align__(16) float sg[kKgmGmBatch][kKgmGmJ];
  __shared__ int64_t s_x[kKgmGmBatch];            // where the occurrence's entity row starts, -1: no term
  __shared__ const float* s_gz[kKgmGmBatch];
  const int32_t de = (int32_t)a.de, dr = (int32_t)a.dr;
  const int32_t tiles_j = (dr + kKgmGmJ - 1) / kKgmGmJ;
  const int32_t c0 = (int32_t)(blockIdx.x / tiles_j) * kKgmGmC, j0 = (int32_t)(blockIdx.x % tiles_j) * kKgmGmJ;
  const int32_t jl = threadIdx.x & (kKgmGmJ - 1), cg = (threadIdx.x / kKgmGmJ) * 4;
  const int32_t per = (int32_t)a.k + 2;
  constexpr int kStage = kKgmGmC + kKgmGmJ;
  // 16-byte loads: fp32 entity rows that start on 16 bytes; gz rows do when the buffers do
  const bool xvec = a.ent_dt == kF32 && de % 4 == 0 && (uintptr_t)a.ent % 16 == 0;
  const bool gvec = a.out_vec != 0 && dr % 4 == 0;
  for (int64_t seg = blockIdx.y; seg < a.nseg; seg += gridDim.y) {
    int64_t s0 = a.seg_ptr[seg], s1 = a.seg_ptr[seg + 1];
    s0 = s0 < 0 ? 0 : (s0 > a.b ? a.b : s0);
    s1 = s1 < s0 ? s0 : (s1 > a.b ? a.b : s1);
    const int64_t rho = a.seg_rel[seg];
    if (!KgInRange(rho, a.rel_rows)) s1 = s0;
    const int64_t total = (s1 - s0) * per;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    bool first = true;
    for (int64_t r0 = 0; r0 < total; r0 += kKgmGmBatch) {
      const int32_t nb = total - r0 < kKgmGmBatch ? (int32_t)(total - r0) : kKgmGmBatch;
      __syncthreads();
      // the batch's occurrences, one thread each: the chain order -> triple -> id is walked once a row
      for (int32_t row = threadIdx.x; row < nb; row += 256) {
        const int64_t at = r0 + row;
        const int64_t t = a.order[s0 + at / per];
        int64_t x = -1;
        const float* gz = nullptr;
        if (t >= 0 && t < a.b && a.rel_id[t] == rho) {
          const KgmOcc o = KgmOccurrence(a, t, (int32_t)(at % per));
          if (KgInRange(o.id, a.ent_rows)) x = o.id * a.de;
          gz = o.gz;
        }
        s_x[row] = x;
        s_gz[row] = gz;
      }
      __syncthreads();
      // their x and gz columns of this tile, four a slot (one 16-byte load where the table allows):
      // independent loads, all of a thread's in flight at once
#pragma unroll 5
      for (int32_t e = threadIdx.x; e < nb * (kStage / 4); e += 256) {
        const int32_t row = e / (kStage / 4), w = (e - row * (kStage / 4)) * 4;
        const int64_t x = s_x[row];
        float f[4] = {0.f, 0.f, 0.f, 0.f};
        if (w < kKgmGmC) {
          if (x >= 0 && xvec && c0 + w < de) {
            const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(a.ent) + x + c0 + w);
            f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
          } else if (x >= 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) f[u] = c0 + w + u < de ? KgmLoad(a.ent, a.ent_dt, x + c0 + w + u) : 0.f;
          }
          *reinterpret_cast<float4*>(&sx[row][w]) = make_float4(f[0], f[1], f[2], f[3]);
        } else {
          const int32_t j = j0 + w - kKgmGmC;
          if (x >= 0 && gvec && j < dr) {
            const float4 v = *reinterpret_cast<const float4*>(s_gz[row] + j);
            f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
          } else if (x >= 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) f[u] = j + u < dr ? s_gz[row][j + u] : 0.f;
          }
          *reinterpret_cast<float4*>(&sg[row][w - kKgmGmC]) = make_float4(f[0], f[1], f[2], f[3]);
        }
      }
      __syncthreads();
      for (int32_t row = 0; row < nb; ++row) {
        if (s_x[row] < 0) continue;
        const float g = sg[row][jl];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float m = __fmul_rn(sx[row][cg + i], g);
          acc[i] = first ? m : __fadd_rn(acc[i], m);
        }
        first = false;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int32_t c = c0 + cg + i, j = j0 + jl;
      if (c < de && j < dr) KgmStore(a.g_matrix, a.mat_dt, (seg * a.de + c) * a.dr + j, acc[i]);
    }
  }
}

template <int V>
void LaunchPerTriple(hipStream_t st, const KgmArgs& a, bool grad, dim3 grid, dim3 block) {
  if (grad) hipLaunchKernelGGL((TripleScoreMatrixGradKernel<V>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((TripleScoreMatrixKernel<V>), grid, block, 0, st, a);
}

unsigned Blocks(int64_t b, int64_t share) {
  const int64_t blocks = (b + share - 1) / share;
  return (unsigned)(blocks > kKgmMaxBlocks ? kKgmMaxBlocks : blocks);
}

// The runs of a workgroup's share are worked on one after the other.  Where a relation has few
// triples (b / rel_rows below a quarter of the large share) a share of many triples is many runs
// of one task each: such batches take one wave a workgroup, and 2 triples a share in the gx
// kernel, so that the runs spread over the CUs.  The choice depends on b and rel_rows only and
// changes no bit.
int Launch(hipStream_t st, KgmArgs a, bool grad) {
  const int32_t v = KgMatrixChunkWidth(a.dr, (uintptr_t)a.rel, a.rel_dt == kF32);
  a.log_l = KgTaskLaunch(a.b, a.dr / v).log_l;
  const bool few = a.b * 4 < a.rel_rows * (256 >> a.log_l);
  const int threads = few ? 64 : 256;
  a.gx_share = few ? 2 : kKgmGxShare;
  const dim3 grid(Blocks(a.b, threads >> a.log_l)), block(threads);
  if (v == 8) LaunchPerTriple<8>(st, a, grad, grid, block);
  else if (v == 4) LaunchPerTriple<4>(st, a, grad, grid, block);
  else LaunchPerTriple<1>(st, a, grad, grid, block);
  EG_HIP(hipGetLastError());
  if (!grad) return EULER_GPU_OK;
  hipLaunchKernelGGL(TripleScoreMatrixRowGradKernel, dim3(Blocks(a.b, a.gx_share)), dim3(256), 0, st, a);
  EG_HIP(hipGetLastError());
  if (a.nseg > 0) {
    const int64_t tiles = ((a.de + kKgmGmC - 1) / kKgmGmC) * ((a.dr + kKgmGmJ - 1) / kKgmGmJ);
    const dim3 cells((unsigned)tiles, (unsigned)(a.nseg > 16384 ? 16384 : a.nseg));
    hipLaunchKernelGGL(TripleScoreMatrixTableGradKernel, cells, dim3(256), 0, st, a);
    EG_HIP(hipGetLastError());
  }
  return EULER_GPU_OK;
}

// what the matrix family adds to the shared ladder
KgCall MatrixCall(const char* what, const KgmArgs& a) {
  KgCall c{what, kKgMatrixFamily, a.ent_dt, a.rel_dt, a.de};
  c.dr = a.dr;
  c.matrix = a.matrix;
  c.matrix_dtype = a.mat_dt;
  c.order = a.order;
  return c;
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_triple_score_matrix(void* stream, int32_t kind, int32_t corrupt, const void* ent_dev, int32_t ent_dtype,
                                  int64_t ent_rows, int64_t de, const void* rel_dev, int32_t rel_dtype,
                                  int64_t rel_rows, int64_t dr, const void* matrix_dev, int32_t matrix_dtype,
                                  const int64_t* src_dev, const int64_t* rel_id_dev, const int64_t* dst_dev,
                                  const int64_t* neg_dev, int64_t b, int64_t k, const int64_t* order_dev,
                                  float* pos_out_dev, float* neg_out_dev) {
  KgmArgs a{KgShared(kind, corrupt, ent_dev, ent_rows, rel_dev, rel_rows, src_dev, rel_id_dev, dst_dev, neg_dev, b, k,
                     pos_out_dev, neg_out_dev),
            ent_dtype, rel_dtype, matrix_dtype, de, dr, matrix_dev, order_dev};
  bool run;
  const int rc = CheckKgCall(MatrixCall("triple_score_matrix", a), a, &run);
  if (rc != EULER_GPU_OK || !run) return rc;
  if (!pos_out_dev || (k > 0 && !neg_out_dev)) return Fail(EULER_GPU_EINVAL, "triple_score_matrix: null output buffer");
  return Launch((hipStream_t)stream, a, false);
}

int euler_gpu_triple_score_matrix_grad(void* stream, int32_t kind, int32_t corrupt, const void* ent_dev,
                                       int32_t ent_dtype, int64_t ent_rows, int64_t de, const void* rel_dev,
                                       int32_t rel_dtype, int64_t rel_rows, int64_t dr, const void* matrix_dev,
                                       int32_t matrix_dtype, const int64_t* src_dev, const int64_t* rel_id_dev,
                                       const int64_t* dst_dev, const int64_t* neg_dev, int64_t b, int64_t k,
                                       const int64_t* order_dev, const int64_t* seg_ptr_dev,
                                       const int64_t* seg_rel_dev, int64_t nseg, const float* g_pos_dev,
                                       const float* g_neg_dev, float* g_src_dev, float* g_rel_dev, float* g_dst_dev,
                                       float* g_neg_rows_dev, float* gz_src_dev, float* gz_dst_dev,
                                       float* gz_neg_rows_dev, void* g_matrix_dev) {
  KgmArgs a{KgShared(kind, corrupt, ent_dev, ent_rows, rel_dev, rel_rows, src_dev, rel_id_dev, dst_dev, neg_dev, b, k,
                     nullptr, nullptr, g_pos_dev, g_neg_dev, g_src_dev, g_rel_dev, g_dst_dev, g_neg_rows_dev),
            ent_dtype, rel_dtype, matrix_dtype, de, dr, matrix_dev, order_dev, seg_ptr_dev, seg_rel_dev, nseg,
            gz_src_dev, gz_dst_dev, gz_neg_rows_dev, g_matrix_dev};
  bool run;
  const int rc = CheckKgCall(MatrixCall("triple_score_matrix_grad", a), a, &run);
  if (rc == EULER_GPU_OK && (nseg < 0 || nseg >= (1LL << 31)))
    return Fail(EULER_GPU_EINVAL, "triple_score_matrix_grad: nseg outside 0 .. 2^31 - 1");
  if (rc != EULER_GPU_OK || !run) return rc;
  if (!g_pos_dev || !g_src_dev || !g_rel_dev || !g_dst_dev || !gz_src_dev || !gz_dst_dev ||
      (k > 0 && (!g_neg_dev || !g_neg_rows_dev || !gz_neg_rows_dev)))
    return Fail(EULER_GPU_EINVAL, "triple_score_matrix_grad: null gradient buffer");
  if (nseg > 0 && (!seg_ptr_dev || !seg_rel_dev || !g_matrix_dev))
    return Fail(EULER_GPU_EINVAL, "triple_score_matrix_grad: nseg > 0 without seg_ptr, seg_rel or g_matrix");
  const uintptr_t rows = (uintptr_t)g_src_dev | (uintptr_t)g_dst_dev | (uintptr_t)g_neg_rows_dev;
  const uintptr_t lane = (uintptr_t)g_rel_dev | (uintptr_t)gz_src_dev | (uintptr_t)gz_dst_dev | (uintptr_t)gz_neg_rows_dev;
  if ((rows | lane) % 4 != 0 || (uintptr_t)g_matrix_dev % (matrix_dtype == EULER_GPU_F32 ? 4 : 2) != 0)
    return Fail(EULER_GPU_EINVAL, "triple_score_matrix_grad: a gradient buffer is not aligned to its type");
  a.out_vec = lane % 16 == 0;
  return Launch((hipStream_t)stream, a, true);
}

}  // extern "C"
