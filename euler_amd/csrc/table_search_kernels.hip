// Exact top-k search and full-table rank over an embedding table on gfx950, with their C-ABI
// entry points (the step of the reference's knn/knn.py:35-77, and utils/metrics.py:51-83 taken
// from sampled negatives to every row).  The scores, the order of the rows and the outputs are
// stated in table_search.h, which the host check compiles too; this file is the tiling.
//
// An ITEM is (query tile, slab of rows); a block of 4 waves takes items blockIdx.x,
// blockIdx.x + gridDim.x, ...  The tile's queries are widened to fp32 into LDS once per item; a
// wave owns up to 8 of them and scores every row of the slab against its own queries.  A row is
// spread over the L lanes the summation order prescribes (64 / L rows side by side in a wave, 4
// rows per group of lanes in registers), its chunk is loaded once and used for every query of
// the wave, and its inv_x (cos) is formed once per row; the four waves of a block walk the slab
// together, so a row comes from HBM once per tile and from L1 for the other waves.  The partial
// sums stay in registers and are combined inside the wave (__shfl_xor): no atomics, and no
// synchronisation between waves after the staging.
//   top-k: lane j of a wave holds entry j of the list of the k best of each of the wave's queries
//          (k <= 64).  A score that the list's last entry does not precede is inserted by the whole
//          wave: position = the number of entries that precede it (a ballot), the entries behind
//          it move one lane up (__shfl_up).  The order is total, so the list does not depend on
//          the order rows arrive in.  The lists go to scratch [slabs][Q][k]; a second launch, a
//          wave per query, merges the slabs the same way and writes both outputs.
//   rank:  the target's score is formed first (the same lane steps), then every row is compared
//          with it; integer partials [slabs][Q], summed by a second launch.
// Scratch is O(Q * k * slabs) from StreamBuf; the outputs are written by the last launch alone, so
// a call that fails leaves both untouched.  Items are ordered tile-fastest: the blocks that walk
// the same slab for different tiles run together and share it in L2.
#include <hip/hip_runtime.h>

#include "device_fns.h"
#include "device_mem.h"
#include "half_cvt.h"
#include "kg_lanes.h"
#include "table_search.h"

namespace euler_gpu {
namespace {

constexpr int QW = kTsWaveQueries, R = kTsRows;

struct TsArgs {
  int32_t log_l, k, qw, staged;                   // qw: queries per wave (tile = kTsWaves * qw)
  const void* table; int64_t n, d;
  const void* queries; int32_t q_dtype; int64_t q;
  const int64_t* exclude; const int64_t* target;
  int64_t tiles, slabs, slab_rows;
  uint2* part;                                    // top-k: [slabs][q][k] {score bits, row}
  int32_t* count;                                 // rank: [slabs][q]
};

// V widened columns of chunk j of a query: from the staged tile (tq: its place there) or from memory
template <int V>
__device__ __forceinline__ void TsQueryChunk(const TsArgs& a, const float* qs, int32_t tq, int64_t q, int32_t j,
                                             float f[V]) {
  if (a.staged) {
    const float* p = qs + (int64_t)tq * a.d + (int64_t)j * V;
    if constexpr (V == 1) {
      f[0] = *p;
    } else {
#pragma unroll
      for (int i = 0; i < V / 4; ++i) {
        const float4 v = reinterpret_cast<const float4*>(p)[i];
        f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
      }
    }
  } else {
    const int64_t at = q * a.d + (int64_t)j * V;
    if (a.q_dtype == EULER_GPU_F32) KgLoadChunk<kF32, V>(a.queries, at, f);
    else if (a.q_dtype == EULER_GPU_BF16) KgLoadChunk<kBF16, V>(a.queries, at, f);
    else KgLoadChunk<kF16, V>(a.queries, at, f);
  }
}

// The scores of the rows row[0 .. R) of this lane's group (-1: no row, scored as zeros and dropped
// by the caller) against the wave's `mine` queries (tile places tq0 .., global q0 ..).
template <int M, int DT, int V>
__device__ __forceinline__ void TsScoreStep(const TsArgs& a, const float* qs, int32_t tq0, int64_t q0, int32_t mine,
                                            const int32_t row[R], const float inv_q[QW], int32_t l, int32_t lanes,
                                            int32_t chunks, float sc[R][QW]) {
  float acc[R][QW], ss[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ss[r] = 0.f;
#pragma unroll
    for (int qi = 0; qi < QW; ++qi) acc[r][qi] = 0.f;
  }
  for (int32_t j = l; j < chunks; j += lanes) {         // (no shuffle inside: lanes may differ in trips)
    const bool first = j == l;
    float x[R][V];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (row[r] >= 0) {
        KgLoadChunk<DT, V>(a.table, (int64_t)row[r] * a.d + (int64_t)j * V, x[r]);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) x[r][k] = 0.f;
      }
    }
    if constexpr (M == kTsCos) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float m = MpwMul(x[r][k], x[r][k]);
          ss[r] = (first && k == 0) ? m : MpwAdd(ss[r], m);
        }
      }
    }
#pragma unroll
    for (int qi = 0; qi < QW; ++qi) {
      if (qi < mine) {
        float qv[V];
        TsQueryChunk<V>(a, qs, tq0 + qi, q0 + qi, j, qv);
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const float m = TsTerm<M>(qv[k], x[r][k]);
            acc[r][qi] = (first && k == 0) ? m : MpwAdd(acc[r][qi], m);
          }
        }
      }
    }
  }
  // The butterfly of KgCombine over all the partial sums at once: the shuffles of one stage are
  // independent, so they are in flight together (one stage = one round trip, not R * QW).
  for (int32_t off = lanes >> 1; off > 0; off >>= 1) {
    float other[R][QW], other_ss[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if constexpr (M == kTsCos) other_ss[r] = __shfl_xor(ss[r], off);
#pragma unroll
      for (int qi = 0; qi < QW; ++qi) other[r][qi] = __shfl_xor(acc[r][qi], off);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if constexpr (M == kTsCos) ss[r] = __fadd_rn(ss[r], other_ss[r]);
#pragma unroll
      for (int qi = 0; qi < QW; ++qi) acc[r][qi] = __fadd_rn(acc[r][qi], other[r][qi]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float inv_x = M == kTsCos ? KgInv(ss[r], true) : 1.f;
#pragma unroll
    for (int qi = 0; qi < QW; ++qi) sc[r][qi] = TsFinish(M, acc[r][qi], inv_q[qi], inv_x);
  }
}

// One candidate into the list whose entry j lane j holds (entries j >= k are never read)
__device__ __forceinline__ void TsWaveInsert(bool larger, int32_t k, int32_t lane, float cs, int32_t cr, float* es,
                                             int32_t* er) {
  const bool before = lane < k && TsEntryPrecedes(larger, *es, *er, cs, cr);
  const int32_t pos = __popcll(__ballot(before));       // the list is sorted: a prefix precedes
  if (pos >= k) return;
  const float us = __shfl_up(*es, 1);
  const int32_t ur = __shfl_up(*er, 1);
  if (lane == pos) { *es = cs; *er = cr; }
  else if (lane > pos) { *es = us; *er = ur; }
}

// The candidates (s, row) of the lanes with `pass` into the list; thr: the list's entry k - 1
__device__ __forceinline__ void TsWaveOffer(bool larger, int32_t k, int32_t lane, bool pass, float s, int32_t row,
                                            float* es, int32_t* er, float* thr_s, int32_t* thr_r) {
  uint64_t any = __ballot(pass);
  if (any == 0) return;
  while (any != 0) {
    const int32_t src = __ffsll((unsigned long long)any) - 1;
    any &= any - 1;
    TsWaveInsert(larger, k, lane, __shfl(s, src), __shfl(row, src), es, er);
  }
  *thr_s = __shfl(*es, k - 1);
  *thr_r = __shfl(*er, k - 1);
}

template <int M, int DT, int V, bool RANK>
__global__ __launch_bounds__(kTsWaves * 64, kTsMinWaves) void TableSearchKernel(const TsArgs a) {
  extern __shared__ float4 ts_lds[];
  float* qs = reinterpret_cast<float*>(ts_lds);
  constexpr bool larger = M == kTsIp || M == kTsCos;
  const int32_t lanes = 1 << a.log_l;
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t sub = lane >> a.log_l, l = lane & (lanes - 1);
  const int32_t groups = 64 >> a.log_l;
  const int32_t chunks = (int32_t)(a.d / V);
  const int32_t tile_q = kTsWaves * a.qw;
  const int64_t items = a.tiles * a.slabs;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t tile = item % a.tiles, slab = item / a.tiles;
    const int64_t tile_q0 = tile * tile_q;
    const int32_t qn = (int32_t)(a.q - tile_q0 < tile_q ? a.q - tile_q0 : tile_q);
    if (a.staged) {
      __syncthreads();                                  // the previous item's readers are done
      const int64_t total = (int64_t)qn * a.d, from = tile_q0 * a.d;
      for (int64_t i = threadIdx.x; i < total; i += blockDim.x) {
        float f;
        if (a.q_dtype == EULER_GPU_F32) f = static_cast<const float*>(a.queries)[from + i];
        else if (a.q_dtype == EULER_GPU_BF16) f = HalfCvt<kBF16>::Widen(static_cast<const uint16_t*>(a.queries)[from + i]);
        else f = HalfCvt<kF16>::Widen(static_cast<const uint16_t*>(a.queries)[from + i]);
        qs[i] = f;
      }
      __syncthreads();
    }
    // this wave's queries: the tile's qn dealt evenly over the waves
    const int32_t per = (qn + kTsWaves - 1) / kTsWaves;
    const int32_t tq0 = wave * per;
    const int32_t mine = tq0 >= qn ? 0 : (qn - tq0 < per ? qn - tq0 : per);
    const int64_t q0 = tile_q0 + tq0;
    if (mine == 0) continue;                            // (no block-wide barrier below)
    float inv_q[QW];
    int32_t exc[QW];
#pragma unroll
    for (int qi = 0; qi < QW; ++qi) {
      inv_q[qi] = 1.f;
      exc[qi] = qi < mine ? TsRowOrNone(a.exclude, q0 + qi, a.n) : -1;
    }
    if constexpr (M == kTsCos) {
#pragma unroll
      for (int qi = 0; qi < QW; ++qi) {
        if (qi < mine) {
          float s = 0.f;
          for (int32_t j = l; j < chunks; j += lanes) {
            float qv[V];
            TsQueryChunk<V>(a, qs, tq0 + qi, q0 + qi, j, qv);
#pragma unroll
            for (int k = 0; k < V; ++k) {
              const float m = MpwMul(qv[k], qv[k]);
              s = (j == l && k == 0) ? m : MpwAdd(s, m);
            }
          }
          inv_q[qi] = KgInv(KgCombine(s, lanes), true);
        }
      }
    }
    // top-k: the lists; rank: the target, its score and the counts
    float es[QW], thr_s[QW], st[QW];
    int32_t er[QW], thr_r[QW], tgt[QW], cnt[QW];
#pragma unroll
    for (int qi = 0; qi < QW; ++qi) {
      es[qi] = thr_s[qi] = TsFill(M);
      er[qi] = thr_r[qi] = -1;
      st[qi] = 0.f;
      cnt[qi] = 0;
      tgt[qi] = RANK && qi < mine ? TsRowOrNone(a.target, q0 + qi, a.n) : -1;
    }
    if constexpr (RANK) {
      for (int32_t t = 0; t < mine; ++t) {
        int32_t row[R];
        float sc[R][QW];
        int32_t tt = -1;
#pragma unroll
        for (int qi = 0; qi < QW; ++qi) tt = qi == t ? tgt[qi] : tt;
#pragma unroll
        for (int r = 0; r < R; ++r) row[r] = (r == 0 && sub == 0) ? tt : -1;
        TsScoreStep<M, DT, V>(a, qs, tq0, q0, mine, row, inv_q, l, lanes, chunks, sc);
#pragma unroll
        for (int qi = 0; qi < QW; ++qi) {
          if (qi == t) st[qi] = __shfl(sc[0][qi], 0);
        }
      }
    }
    const int64_t r_begin = slab * a.slab_rows;
    const int64_t r_end = r_begin + a.slab_rows < a.n ? r_begin + a.slab_rows : a.n;
    for (int64_t base = r_begin; base < r_end; base += (int64_t)groups * R) {   // the same trips for every lane
      int32_t row[R];
      float sc[R][QW];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t rr = base + (int64_t)r * groups + sub;
        row[r] = rr < r_end ? (int32_t)rr : -1;
      }
      TsScoreStep<M, DT, V>(a, qs, tq0, q0, mine, row, inv_q, l, lanes, chunks, sc);
      if constexpr (RANK) {
#pragma unroll
        for (int qi = 0; qi < QW; ++qi) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const bool cand = l == 0 && qi < mine && row[r] >= 0 && row[r] != exc[qi] && row[r] != tgt[qi];
            cnt[qi] += (cand && TsCounts(larger, sc[r][qi], st[qi])) ? 1 : 0;
          }
        }
      } else {
        // One branch a step: once the lists are full, a step rarely holds a score that enters one.
        // The test is the cheap side of the order - "the list's last score is not strictly better"
        // (true with a NaN on either side, and for an empty entry, whose score is the fill) - and
        // only lets too much through; the order itself decides below.
        bool some = false;
#pragma unroll
        for (int qi = 0; qi < QW; ++qi) {
#pragma unroll
          for (int r = 0; r < R; ++r)
            some |= qi < mine && row[r] >= 0 && !(larger ? thr_s[qi] > sc[r][qi] : thr_s[qi] < sc[r][qi]);
        }
        if (__ballot(some && l == 0) != 0) {
#pragma unroll
          for (int qi = 0; qi < QW; ++qi) {
            if (qi < mine) {
#pragma unroll
              for (int r = 0; r < R; ++r) {
                const bool pass = l == 0 && row[r] >= 0 && row[r] != exc[qi] &&
                                  !TsEntryPrecedes(larger, thr_s[qi], thr_r[qi], sc[r][qi], row[r]);
                TsWaveOffer(larger, a.k, lane, pass, sc[r][qi], row[r], &es[qi], &er[qi], &thr_s[qi], &thr_r[qi]);
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int qi = 0; qi < QW; ++qi) {
      if (qi < mine) {
        const int64_t at = slab * a.q + q0 + qi;
        if constexpr (RANK) {
          int32_t c = cnt[qi];
          for (int32_t off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
          if (lane == 0) a.count[at] = c;
        } else {
          if (lane < a.k) a.part[at * a.k + lane] = make_uint2(F32Bits(es[qi]), (uint32_t)er[qi]);
        }
      }
    }
  }
}

// A wave per query: the slabs' lists into one, then both outputs.  Grid-stride over the queries.
__global__ __launch_bounds__(256) void TableTopkMergeKernel(int32_t metric, const uint2* part, int64_t q, int64_t slabs,
                                                            int32_t k, float* scores, int64_t* rows) {
  const bool larger = TsLargerIsBetter(metric);
  const int32_t lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t total = slabs * k;
  for (int64_t qq = wave; qq < q; qq += waves) {
    float es = TsFill(metric), thr_s = es;
    int32_t er = -1, thr_r = -1;
    for (int64_t base = 0; base < total; base += 64) {
      const int64_t i = base + lane;
      float s = 0.f;
      int32_t row = -1;
      if (i < total) {
        const uint2 e = part[((i / k) * q + qq) * k + i % k];
        s = BitsF32(e.x);
        row = (int32_t)e.y;
      }
      const bool pass = row >= 0 && !TsEntryPrecedes(larger, thr_s, thr_r, s, row);
      TsWaveOffer(larger, k, lane, pass, s, row, &es, &er, &thr_s, &thr_r);
    }
    if (lane < k) {
      scores[qq * k + lane] = es;
      rows[qq * k + lane] = er;
    }
  }
}

// rank[q] = the sum of the slabs' counts, or -1 for a target that names no row
__global__ __launch_bounds__(256) void TableRankSumKernel(const int32_t* count, const int64_t* target, int64_t q,
                                                          int64_t slabs, int64_t n, int32_t* rank) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t qq = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; qq < q; qq += stride) {
    int32_t c = 0;
    for (int64_t s = 0; s < slabs; ++s) c += count[s * q + qq];
    rank[qq] = KgInRange(target[qq], n) ? c : -1;
  }
}

template <int M, int DT, int V>
void LaunchOne(hipStream_t st, const TsArgs& a, bool rank, dim3 grid, size_t lds) {
  if (rank) hipLaunchKernelGGL((TableSearchKernel<M, DT, V, true>), grid, dim3(kTsWaves * 64), lds, st, a);
  else hipLaunchKernelGGL((TableSearchKernel<M, DT, V, false>), grid, dim3(kTsWaves * 64), lds, st, a);
}

template <int M, int DT>
void LaunchWidth(hipStream_t st, const TsArgs& a, int32_t v, bool rank, dim3 grid, size_t lds) {
  if (v == 8) LaunchOne<M, DT, 8>(st, a, rank, grid, lds);
  else if (v == 4) LaunchOne<M, DT, 4>(st, a, rank, grid, lds);
  else LaunchOne<M, DT, 1>(st, a, rank, grid, lds);
}

template <int M>
void LaunchDtype(hipStream_t st, const TsArgs& a, int32_t table_dtype, int32_t v, bool rank, dim3 grid, size_t lds) {
  if (table_dtype == EULER_GPU_F32) LaunchWidth<M, kF32>(st, a, v, rank, grid, lds);
  else if (table_dtype == EULER_GPU_BF16) LaunchWidth<M, kBF16>(st, a, v, rank, grid, lds);
  else LaunchWidth<M, kF16>(st, a, v, rank, grid, lds);
}

// The search launch.  Items = tiles * slabs, tiles = ceil(q / (kTsWaves * qw)) with qw of
// TsWaveQueriesFor(d) (8 up to d = 384), slabs = TsSlabs(n, tiles); one item a block per trip,
// the grid capped at kTsBlockCap = 8192 blocks, a block looping over the items past it.
int LaunchSearch(hipStream_t st, TsArgs a, int32_t metric, int32_t table_dtype, bool rank) {
  const int32_t v = KgChunkWidth(a.d, (uintptr_t)a.table, table_dtype == EULER_GPU_F32, (uintptr_t)a.queries,
                                 a.q_dtype == EULER_GPU_F32);
  a.log_l = KgLogLanes(a.d / v);
  const int64_t items = a.tiles * a.slabs;
  const dim3 grid((unsigned)(items > kTsBlockCap ? kTsBlockCap : items));
  const size_t lds = a.staged ? (size_t)kTsWaves * a.qw * a.d * sizeof(float) : 0;
  if (metric == kTsIp) LaunchDtype<kTsIp>(st, a, table_dtype, v, rank, grid, lds);
  else if (metric == kTsCos) LaunchDtype<kTsCos>(st, a, table_dtype, v, rank, grid, lds);
  else if (metric == kTsL2) LaunchDtype<kTsL2>(st, a, table_dtype, v, rank, grid, lds);
  else LaunchDtype<kTsL1>(st, a, table_dtype, v, rank, grid, lds);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

// The argument ladder in front of both entries (k: 1 for the rank; `extra`: the entry's own
// required pointers, all set?).  -> EULER_GPU_OK with *run = false when q == 0.
int CheckTableSearch(const char* what, int32_t metric, const void* table, int32_t table_dtype, int64_t n, int64_t d,
                     const void* queries, int32_t q_dtype, int64_t q, int64_t k, bool extra, bool* run) {
  *run = false;
  const std::string w(what);
  if (metric < kTsIp || metric > kTsL1) return Fail(EULER_GPU_EINVAL, w + ": metric outside 0..3 (0 ip, 1 cos, 2 l2, 3 l1)");
  if (!KnownDtype(table_dtype) || !KnownDtype(q_dtype)) return Fail(EULER_GPU_EINVAL, w + ": unknown dtype" + kDtypeCodes);
  if (d < 1) return Fail(EULER_GPU_EINVAL, w + ": d < 1");
  if (d >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, w + ": d >= 2^31");
  if (n < 0 || n >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, w + ": n outside 0 .. 2^31 - 1");
  if (q < 0 || q >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, w + ": q outside 0 .. 2^31 - 1");
  if (k < 1 || k > kTsMaxK) return Fail(EULER_GPU_EINVAL, w + ": k outside 1..64");
  if (q == 0) return EULER_GPU_OK;
  if ((n > 0 && !table) || !queries || !extra) return Fail(EULER_GPU_EINVAL, w + ": null buffer");
  if ((uintptr_t)table % (table_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)queries % (q_dtype == EULER_GPU_F32 ? 4 : 2) != 0)
    return Fail(EULER_GPU_EINVAL, w + ": a table is not aligned to its type");
  *run = true;
  return EULER_GPU_OK;
}

TsArgs MakeArgs(const void* table, int64_t n, int64_t d, const void* queries, int32_t q_dtype, int64_t q, int64_t k,
                const int64_t* exclude, const int64_t* target) {
  TsArgs a{};
  bool staged;
  a.qw = TsWaveQueriesFor(d, &staged);
  a.staged = staged;
  a.k = (int32_t)k;
  a.table = table; a.n = n; a.d = d;
  a.queries = queries; a.q_dtype = q_dtype; a.q = q;
  a.exclude = exclude; a.target = target;
  const int64_t tile_q = (int64_t)kTsWaves * a.qw;
  a.tiles = (q + tile_q - 1) / tile_q;
  a.slabs = TsSlabs(n, a.tiles);
  a.slab_rows = (n + a.slabs - 1) / a.slabs;
  return a;
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_table_topk(void* stream, int32_t metric, const void* table_dev, int32_t table_dtype, int64_t n,
                         int64_t d, const void* queries_dev, int32_t q_dtype, int64_t q, int64_t k,
                         const int64_t* exclude_dev, float* scores_out, int64_t* rows_out) {
  bool run;
  const int rc = CheckTableSearch("table_topk", metric, table_dev, table_dtype, n, d, queries_dev, q_dtype, q, k,
                                  scores_out && rows_out, &run);
  if (rc != EULER_GPU_OK || !run) return rc;
  if ((uintptr_t)scores_out % 4 != 0 || (uintptr_t)rows_out % 8 != 0 || (uintptr_t)exclude_dev % 8 != 0)
    return Fail(EULER_GPU_EINVAL, "table_topk: an index or output buffer is not aligned to its type");
  hipStream_t st = (hipStream_t)stream;
  TsArgs a = MakeArgs(table_dev, n, d, queries_dev, q_dtype, q, k, exclude_dev, nullptr);
  StreamBuf part(st);
  if (part.alloc((size_t)a.slabs * q * k * sizeof(uint2)) != hipSuccess)
    return Fail(EULER_GPU_ENOMEM, "table_topk: no memory for the slabs' lists");
  a.part = part.as<uint2>();
  const int rl = LaunchSearch(st, a, metric, table_dtype, false);
  if (rl != EULER_GPU_OK) return rl;
  int64_t blocks = (q + 3) / 4;                          // a wave per query, 4 a block; capped, the waves loop
  if (blocks > kTsBlockCap) blocks = kTsBlockCap;
  hipLaunchKernelGGL(TableTopkMergeKernel, dim3((unsigned)blocks), dim3(256), 0, st, metric, a.part, q, a.slabs,
                     (int32_t)k, scores_out, rows_out);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_table_rank(void* stream, int32_t metric, const void* table_dev, int32_t table_dtype, int64_t n,
                         int64_t d, const void* queries_dev, int32_t q_dtype, int64_t q, const int64_t* target_dev,
                         const int64_t* exclude_dev, int32_t* rank_out) {
  bool run;
  const int rc = CheckTableSearch("table_rank", metric, table_dev, table_dtype, n, d, queries_dev, q_dtype, q, 1,
                                  target_dev && rank_out, &run);
  if (rc != EULER_GPU_OK || !run) return rc;
  if ((uintptr_t)rank_out % 4 != 0 || (uintptr_t)target_dev % 8 != 0 || (uintptr_t)exclude_dev % 8 != 0)
    return Fail(EULER_GPU_EINVAL, "table_rank: an index or output buffer is not aligned to its type");
  hipStream_t st = (hipStream_t)stream;
  TsArgs a = MakeArgs(table_dev, n, d, queries_dev, q_dtype, q, 1, exclude_dev, target_dev);
  StreamBuf count(st);
  if (count.alloc((size_t)a.slabs * q * sizeof(int32_t)) != hipSuccess)
    return Fail(EULER_GPU_ENOMEM, "table_rank: no memory for the slabs' counts");
  a.count = count.as<int32_t>();
  const int rl = LaunchSearch(st, a, metric, table_dtype, true);
  if (rl != EULER_GPU_OK) return rl;
  hipLaunchKernelGGL(TableRankSumKernel, dim3((unsigned)GridFor(q, 256)), dim3(256), 0, st, a.count, target_dev, q,
                     a.slabs, n, rank_out);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

}  // extern "C"
