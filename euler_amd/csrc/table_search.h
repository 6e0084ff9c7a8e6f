// Exact search over a whole embedding table: the k best rows of a [N, d] table for each of Q
// queries (the reference's knn/knn.py:35-77, which returns (distance, idx) through faiss) and the
// rank of a given row among ALL rows (utils/metrics.py:51-83 ranks it among sampled negatives
// only): the arithmetic of ONE LANE for one (query, row) pair and the ordering rules, shared by
// the kernels of table_search_kernels.hip and by tests/csrc/table_search_check.cc, which compiles
// this file with the host compiler.  Every operation is a correctly rounded fp32 multiply, add,
// divide or square root (MpwMul / MpwAdd / MpwDiv / SeSqrt: on the device the __f*_rn forms, on
// the host plain operators in a translation unit built with -ffp-contract=off), a comparison or an
// integer operation: host and device return the same bits by construction.
//
// INPUTS: table [N, d] and queries [Q, d], fp32 / bf16 / fp16, each its own type, widened exactly
// to fp32; exclude [Q] int64 (optional): a row the query must neither return nor count - its own
// row when the queries come from the table; target [Q] int64 (the rank only).  Row offsets are
// int64: N * d may pass 2^31 elements; N < 2^31.
// SCORE s(q, x) of query row q and table row x, by metric:
//   0 ip   sum q_c * x_c                                   larger is better
//   1 cos  (ip * inv_q) * inv_x, inv = KgInv(ss, true)     larger is better
//          of kg_score.h with ss = sum x_c * x_c (1 / sqrt(max(ss, 1e-12)))
//   2 l2   sum e_c * e_c, e_c = q_c - x_c                  smaller is better
//          (the squared distance, as faiss METRIC_L2 returns it)
//   3 l1   sum |e_c| (KgAbs)                               smaller is better
//          (TransE's energy with q = h + r)
// SUMMATION ORDER - every sum over columns (the scores, ss of a table row and of a query) - is the
// one kg_score.h states with V = KgChunkWidth(d, table, queries): chunks of V adjacent columns,
// L = min(64, the power of two >= d / V) lanes; lane l takes the chunks l, l + L, ... and adds
// their terms one by one in increasing column order, starting FROM its first term (KgAcc); a lane
// without a chunk holds +0; then for off = L / 2, ..., 1: s = s + s[lane ^ off].  A score is a
// function of the two rows, their types and V alone - never of Q, N, k, the tiling or the grid.
// A NaN score is returned as a NaN; its sign and payload are the hardware's and no part of the contract.
// ORDER of the rows for one query: a precedes b iff s_a is better than s_b, or s_b is NaN and s_a
// is not, or the two compare equal (+0 == -0; any two NaNs) and a < b.  A total order: the result
// is a pure function of the scores, whatever order the rows are visited in.
// TOP-K: rows[q][j] (int64) = the j-th row in that order among [0, N) without exclude[q], for
// j < min(k, candidates); scores[q][j] (fp32) its score; past the candidates rows = -1 and
// scores = -inf (ip, cos) / +inf (l2, l1).  1 <= k <= 64.
// RANK: s_t = s(q, table[target[q]]) by the same lane arithmetic; rank[q] (int32) = the number of
// rows r in [0, N), r != target[q], r != exclude[q], whose score is better than or EQUAL to s_t:
// a tie goes against the target (the rule skipgram.h states for the sampled rank).  A NaN score is
// never counted (and nothing is counted against a NaN s_t).  A target outside [0, N) gives
// rank = -1; an exclude outside [0, N) excludes nothing.
// EMPTY SHAPES: Q == 0 touches nothing; N == 0 writes the fills (top-k) or -1 (rank).
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "half_cvt.h"
#include "kg_score.h"
#include "mp_weighted.h"
#include "sparse_embed.h"

namespace euler_gpu {

constexpr int kTsIp = 0, kTsCos = 1, kTsL2 = 2, kTsL1 = 3;
constexpr int kTsMaxK = 64;

// THE LAUNCH SHAPE (nothing of it enters a score or the order).  A block is kTsWaves waves; a wave
// owns up to kTsWaveQueries queries of the block's query tile and scores every row of the block's
// slab of rows against them, kTsRows rows per group of L lanes at a time.
constexpr int kTsWaves = 4, kTsWaveQueries = 8, kTsRows = 4;
#if defined(EULER_GPU_TS_MIN_WAVES)
constexpr int kTsMinWaves = EULER_GPU_TS_MIN_WAVES;   // an experiment's build (make EXTRA=-D...)
#else
constexpr int kTsMinWaves = 2;              // waves a SIMD the search kernel's register budget is declared for
#endif
constexpr int kTsLdsFloats = 12288;         // 48 KiB: the staged (widened) queries of a tile
constexpr int kTsMinSlabRows = 1024;        // a table up to this many rows is one slab
constexpr int kTsMaxSlabs = 512;
constexpr int kTsTargetBlocks = 2048;       // tiles * slabs aims at this many (tile, slab) items
constexpr int kTsBlockCap = 256 * 32;       // the grid's cap: a block loops over the items past it

// queries per wave: as many as keep the tile's widened queries inside kTsLdsFloats; rows wider
// than kTsLdsFloats / kTsWaves are not staged (*staged = false): the lanes read them from memory
inline int32_t TsWaveQueriesFor(int64_t d, bool* staged) {
  const int64_t fit = kTsLdsFloats / (kTsWaves * d);
  *staged = fit >= 1;
  return (int32_t)(fit < 1 || fit > kTsWaveQueries ? kTsWaveQueries : fit);
}

// S, the slabs of rows: a function of N and of the number of query tiles alone
inline int64_t TsSlabs(int64_t n, int64_t tiles) {
  int64_t s = (kTsTargetBlocks + tiles - 1) / (tiles < 1 ? 1 : tiles);
  const int64_t by_rows = (n + kTsMinSlabRows - 1) / kTsMinSlabRows;
  if (s > by_rows) s = by_rows;
  if (s > kTsMaxSlabs) s = kTsMaxSlabs;
  return s < 1 ? 1 : s;
}

EG_MPW_HD bool TsLargerIsBetter(int32_t metric) { return metric == kTsIp || metric == kTsCos; }

// the score of an entry past the candidates
EG_MPW_HD float TsFill(int32_t metric) {
  return BitsF32(TsLargerIsBetter(metric) ? 0xff800000u : 0x7f800000u);
}

// the term of one column
template <int M>
EG_MPW_HD float TsTerm(float q, float x) {
  if constexpr (M == kTsIp || M == kTsCos) {
    return MpwMul(q, x);
  } else {
    const float e = MpwAdd(q, -x);
    return M == kTsL2 ? MpwMul(e, e) : KgAbs(e);
  }
}

// a lane's part of the terms of s(q, x): Q and X are Rows of kg_score.h (Chunk(j, f) gives the V
// widened columns of chunk j).  The kernels run these steps for several rows and queries at once.
template <int M, int V, typename RowQ, typename RowX>
EG_MPW_HD float TsLaneScore(const RowQ& q, const RowX& x, int32_t l, int32_t lanes, int32_t chunks) {
  float s = 0.f;
  bool first = true;
  for (int32_t j = l; j < chunks; j += lanes) {
    float fq[V], fx[V];
    q.Chunk(j, fq);
    x.Chunk(j, fx);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) KgAcc(TsTerm<M>(fq[k], fx[k]), &s, &first);
  }
  return s;
}

// the score from the combined sum of its terms; inv_q / inv_x: KgInv of the two rows (cos only)
EG_MPW_HD float TsFinish(int32_t metric, float s, float inv_q, float inv_x) {
  return metric == kTsCos ? MpwMul(MpwMul(s, inv_q), inv_x) : s;
}

// ORDER: does row ra with score sa precede row rb with score sb?  (ra != rb)
EG_MPW_HD bool TsPrecedes(bool larger, float sa, int64_t ra, float sb, int64_t rb) {
  const bool an = sa != sa, bn = sb != sb;
  if (an | bn) return an == bn ? ra < rb : bn;
  if (sa == sb) return ra < rb;
  return larger ? sa > sb : sa < sb;
}

// The same over the entries of a list of the k best, where row -1 marks an empty entry: every
// row precedes an empty entry and an empty entry precedes nothing.
EG_MPW_HD bool TsEntryPrecedes(bool larger, float sa, int32_t ra, float sb, int32_t rb) {
  if (ra < 0) return false;
  if (rb < 0) return true;
  return TsPrecedes(larger, sa, ra, sb, rb);
}

// RANK: is a row with score s counted against a target with score st?  (never with a NaN)
EG_MPW_HD bool TsCounts(bool larger, float s, float st) { return larger ? s >= st : s <= st; }

// exclude[q] / target[q] as the row it names, or -1 (which equals no row) outside [0, n)
EG_MPW_HD int32_t TsRowOrNone(const int64_t* ids, int64_t q, int64_t n) {
  if (!ids) return -1;
  const int64_t id = ids[q];
  return KgInRange(id, n) ? (int32_t)id : -1;
}

}  // namespace euler_gpu
