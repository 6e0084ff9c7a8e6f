// Fused RelationConv (RGCN, tf_euler/python/convolution/relation_conv.py:53-70) - the typed reduce
// of relation_reduce and the per-relation matmul in ONE pass on the matrix units:
//
//     out[r] = sum_t  bucket(r, t) @ weight[t]^T,     bucket(r, t) = aggr over the valid updates
//                                                     of destination r with relation t of x[g(p)]
//
// The [size, R, F] block that relation_reduce writes and a GEMM reads back never exists: the R
// bucket aggregates of a destination stay in registers and are the A operands of the matrix
// instructions.  This file states the contract and holds the plan; the host entry, the kernel
// (relation_dense_kernels.hip) and a host-only program can all include it.
//
// ARGUMENTS.  x [rows, F] and weight [R, dim, F] (the reference's `matrix`), contiguous, one dtype
// of fp32 / bf16 / fp16.  mode: 0 add, 2 mean over the destination, 3 mean over the bucket (the
// codes of relation_reduce; 1, max, does not commute with the matrices).  out [size, dim], fp32 or
// x's dtype.
// VALIDITY, SEGMENTS AND INDICES are those of relation_reduce (mp_relation.h), so that the fused
// and the composed route agree.  Update p has the relation edge_type[p] and is valid iff
// 0 <= edge_type[p] < R; an invalid update belongs to no bucket and its row is never read.
// g(p) is p itself (no gather array; rows >= e), an int32 index or the low word of an int64 id,
// CLAMPED to rows - 1 as relation_reduce clamps it (MpwIndex::Row) - not the range rule of
// mp_dense.h.  Destination r owns the positions seg_ptr[r] .. seg_ptr[r + 1] (int64 [size + 1])
// or r * count .. (r + 1) * count with e == size * count, exactly one of the two; boundaries are
// kept inside [0, e] and an end at or after its begin (TkSegment).
// BUCKET FOLD, as RelationReduceDest folds it: from +0, the widened rows added in input order in
// fp32, one rounding per add; mode 2 then divides by fl(n_valid(r) + 1e-7f), mode 3 by
// fl(cnt(r, t) + 1e-7f), a true (correctly rounded) division; the bucket is then rounded ONCE to
// x's dtype (fp32: kept).  That is the value the composed route stores in its [size, R, F] block.
// ACCUMULATION.  The matrix instructions accumulate out[r] in fp32 in a fixed order: relations in
// increasing t, and within a relation the chunks of 32 k in increasing k; zero-filled tails (k >=
// F, columns >= dim) add +0.  One rounding to out_dtype at the store.
// EMPTY BUCKETS contribute nothing.  The kernel skips a relation that no destination of a wave's
// run has: with finite weights this cannot change a bit, because a bucket of +0 adds +0 products
// to a fp32 accumulator that starts at +0 and is therefore never -0.  With a NON-FINITE weight[t]
// the composed route's 0 x inf = NaN of an empty bucket is NOT reproduced for a skipped relation.
// DETERMINISM.  The same bits on every run, on every stream, for count or the equivalent seg_ptr,
// and wherever the destination sits in a run, a workgroup or the grid: a lane sees only its own
// destination's [begin, end), and a relation the lane's destination lacks adds +0 only.
// LIMITS.  1 <= F <= kRelDenseMaxF, 1 <= dim <= kRelDenseMaxDim, 1 <= R <= kRelDenseMaxR (a lane
// keeps the set of relations of its segment in one 64-bit word), e, size < 2^31, a mean with e or
// count below 2^24 (exact fp32 counts).  size == 0 touches nothing.
//
// THE KERNEL (RelDensePlan below is the one statement of its choices).
// A workgroup is 4 waves; a wave owns `m` RUNS of 16 consecutive destinations at a time.  Lane l
// owns destination l % 16 and, per chunk of 32 k, the 8 slots from 8 * (l / 16): the A operand of
// v_mfma_f32_16x16x32_{bf16,f16} (fp32: the eight v_mfma_f32_16x16x4_f32 and the k permutation of
// mp_pool.h).  ceil(dim / 16) accumulator fragments of 4 registers per run are kept across all
// relations and stored once.
// THE TYPE COLUMN is read in a pre-pass, once per run: the four lanes of a destination take every
// fourth position, build the 64-bit set of its relations and n_valid, and combine; an OR over the
// wave is the set of relations the run has.  A relation outside it is skipped: no fold, no MFMA.
// THE WALK of a present relation t, per fold tile of 128 k: the lanes walk their segments in
// lockstep - trip count the run's longest segment, or the scalar count - predicated on edge_type
// == t; the row loads of a batch of positions (4 for 16-bit rows, 2 for fp32: DenseBatch) are
// issued before the first add; 16-byte loads where x is aligned and F % 8 == 0 (fp32: % 4),
// element loads otherwise, nothing read past a row.  After the division and the narrowing the
// 32 fold registers ARE the A fragments of 4 chunks.
// WEIGHTS IN LDS.  weight[t] is [dim, F]: Wt[c][k] already.  It is copied in 16-byte units into
// the DenseWtByte layout of mp_dense.h (packed and XOR-swizzled where a column's staged K extent is
// a multiple of 256 bytes, else + 16 bytes a column); columns >= dim and k >= F are +0.
//  - RESIDENT: all R matrices fit the window.  They are staged once per workgroup, the waves then
//    run free over the groups of runs (grid capped at kRelDenseMaxBlocks, a loop beyond it).
//  - PHASED: otherwise a W tile - tile_cols columns x the 128 k of a fold tile of one relation -
//    is staged per (relation, fold tile, column tile) for the waves x m x 16 destinations of a
//    group; the waves move in lockstep, two barriers a tile.  A relation that no wave of the
//    workgroup has is not staged: the waves exchange their 64-bit sets through the first 32 bytes
//    of the window, between the last read of one group's tiles and the first copy of the next.
//    The copy of the next tile does not overlap the fold of this one: one tile at a time.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "mp_dense.h"
#include "mp_relation.h"

namespace euler_gpu {

constexpr int kRelDenseMaxF = 256;
constexpr int kRelDenseMaxDim = 256;
constexpr int kRelDenseMaxR = 64;
constexpr int kRelDenseWaves = 4;            // per workgroup
constexpr int kRelDenseLdsBytes = 65536;     // the window of W, all of a workgroup's LDS: 2 workgroups a CU
constexpr int kRelDenseMaxBlocks = 512;      // 2 resident workgroups x 256 CUs

struct RelDensePlan {
  int32_t nt;         // accumulator fragments of a run: the least of 1, 2, 4, 8, 16 with 16 nt >= dim
  int32_t m;          // runs a wave holds at a time: 2 up to nt = 8 (64 accumulator registers)
  int32_t resident;   // 1: all R matrices are staged once per workgroup
  int32_t stride;     // bytes between the columns of a staged Wt
  int32_t tile_cols;  // columns of a staged W tile (phased), a multiple of 16
  int32_t col_tiles;  // W tiles per (relation, fold tile)
  int32_t lds_bytes;  // dynamic LDS of a workgroup
};

inline RelDensePlan RelDenseMakePlan(int64_t f, int64_t dim, int64_t num_relations, bool f32) {
  const int32_t esz = f32 ? 4 : 2;
  const int32_t f32k = (int32_t)((f + kPoolChunk - 1) / kPoolChunk) * kPoolChunk;
  RelDensePlan p{};
  p.nt = 1;
  while (16 * p.nt < dim) p.nt *= 2;
  p.m = p.nt <= 8 ? 2 : 1;
  const int32_t cols = 16 * p.nt;
  const int32_t full = DenseColumnBytes(f32k, esz);
  if ((int64_t)num_relations * cols * full <= kRelDenseLdsBytes) {
    p.resident = 1;
    p.stride = full;
    p.tile_cols = cols;
    p.col_tiles = 1;
    p.lds_bytes = (int32_t)num_relations * cols * full;
    return p;
  }
  p.stride = DenseColumnBytes(f32k < kDenseFoldTile ? f32k : kDenseFoldTile, esz);
  p.tile_cols = kRelDenseLdsBytes / p.stride / 16 * 16;
  if (p.tile_cols > cols) p.tile_cols = cols;
  p.col_tiles = (cols + p.tile_cols - 1) / p.tile_cols;
  p.lds_bytes = p.tile_cols * p.stride;
  return p;
}

}  // namespace euler_gpu
