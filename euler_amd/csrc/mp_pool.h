// Fused pooling aggregation - the `meanpool` / `maxpool` aggregators of the reference's SageEncoder
// (tf_euler/python/utils/aggregators.py:75-114): every gathered neighbour row goes through a dense
// layer and an activation BEFORE it is reduced over the neighbours,
//
//     out[r] = reduce_{p in segment(r)}  act( table[g[p]] @ W + b )          reduce = max | mean | add
//
// in one pass, on the matrix units, without the [e, d] gathered block or the [e, F] activation
// block.  This file states the contract and holds the tile plan, which the host entry, the kernel
// (pool_aggregate_kernels.hip) and a host-only program can all include.
//
// ARGUMENTS.  table [rows, d] fp32 / bf16 / fp16, contiguous.  weight [d, F] (the layout of a TF
// Dense kernel), contiguous, the table's dtype.  bias [F], fp32 or the table's dtype, widened
// exactly; none = +0.  op: max, mean or add.  act: relu (the reference's) or none.
// SEGMENTS AND INDICES (those of mp_topk.h).  Destination r owns the positions seg_ptr[r] ..
// seg_ptr[r + 1] (int64 [size + 1]), or r * count .. (r + 1) * count with e == size * count;
// exactly one of the two forms.  g[p] is an int32 index, a signed int64 id compared in 64 bits, or
// p itself when no gather array is given.  RANGE RULE: an index outside [0, rows) names no row; it
// is never dereferenced and reads as a row of +0.  It DOES take part in the reduce, with the term
// act(b) - what the reference computes for a default_node fill, whose feature row is zeros.  Its
// table gradient is dropped.  A well-formed seg_ptr is non-decreasing.  For a malformed one the
// values are kept inside [0, e] and made non-decreasing within each run of 16 destinations (a
// value below its predecessor counts as the predecessor), so nothing is read or written out of
// bounds; what the destinations then reduce is unspecified.
// ARITHMETIC.  Products are taken from the stored values and accumulated in fp32 over k by the
// matrix instructions, in an order that depends only on d (the K chunks of 32 in increasing k; the
// zero-filled tail of the last chunk adds +0) - never on where the row sits in a tile, a wave, a
// workgroup or the grid.  Then the bias is added in fp32 and the activation applied (relu: x > 0
// ? x : +0, a NaN stays a NaN).  The terms of a segment are folded in increasing p in fp32, the
// first term taken as it is: max with NaN greatest (as scatter_max), add / mean with one rounding
// per add and, for mean, one multiply by 1 / len computed in fp32.  The result is rounded once to
// the output dtype (fp32 or the table's).  An empty segment gives +0 for every op.
// DETERMINISM.  The same call gives the same bits on every run, on every stream, and whether the
// segmentation is written with count or with the equivalent seg_ptr: both forms become the same
// boundary values before anything else looks at them.
// LIMITS.  e < 2^31, size < 2^31, 1 <= d, F <= 4096, rows >= 1.  size == 0 touches nothing.
//
// THE TILING (PoolPlan below is its one statement).
// A workgroup is 4 waves.  A wave owns RUNS of 16 consecutive destinations, whole, and walks the
// positions of a run in tiles of 16: the M of the matrix instruction is 16 gathered rows.  The N
// is 16 output columns; a wave keeps NT = F_tile / 16 accumulator fragments (NT in 1, 2, 4, 8, so
// F_tile <= 128 and 32 accumulator registers at most).  The K chunk is 32 for every dtype.
// FRAGMENTS.  In a chunk, lane l holds row l % 16 and the 8 consecutive k starting at 8 * (l / 16)
// of A, and the same 8 k of column l % 16 of B.  For bf16 / fp16 this is the operand layout of
// v_mfma_f32_16x16x32_{bf16,f16}: one instruction per chunk and fragment.  For fp32 the same 8
// elements feed 8 v_mfma_f32_16x16x4_f32: instruction j takes element j of every lane, i.e. the
// four k values 8 * g + j (g = 0..3) - a fixed permutation of k inside the chunk that A and B
// share, so no LDS staging of A is needed for fp32 either.  The accumulator of lane l holds rows
// 4 * (l / 16) + i, i = 0..3, of column l % 16.
// A goes from global memory straight into registers: 16 contiguous bytes of a table row per lane
// and chunk when d % 8 == 0 (fp32: two 16-byte loads, d % 4 == 0) and the table starts on a
// 16-byte boundary; otherwise element loads.  A K tail is zero-filled, never read past the row.
// W IN LDS.  W^T is staged k-contiguous per output column: Wt[c][k], column stride K_tile + 16
// bytes, so a B fragment is one 16-byte LDS read (fp32: two) and the 16 columns of a quarter wave
// fall on distinct banks.  Columns >= F and k >= d are +0.
// LDS BUDGET: 64 KB per workgroup - 17 408 bytes of fold staging (4 waves x 16 rows x 68 floats)
// and kPoolWBytes = 47 104 bytes of W^T.  gfx950 has 160 KB per CU, so 2 workgroups (8 waves) are
// resident per CU at the full budget, 3 at d = F = 128 in 16 bits (52 KB).
// F TILING: F_tile is the largest of 128 / 64 / 32 / 16 (not above F rounded up to 16) whose
// F_tile x (d32 + pad) elements fit kPoolWBytes, d32 = d rounded up to 32.  There are
// ceil(F / F_tile) F-tile passes; a gathered row is read once per pass.  16-bit tables: F_tile 128
// up to d = 160, 64 up to 352, 32 up to 704, 16 beyond; fp32: 128 / 64 / 32 / 16 up to d = 64 /
// 160 / 352 / 704.  d = F = 128 in 16 bits is ONE pass.
// K TILING: where even F_tile = 16 does not fit (16-bit d > 1440, fp32 d > 704), K is cut into
// K tiles of 1440 (fp32 704) and W^T is re-staged per K tile for the four row tiles the
// workgroup's waves hold at that moment; the waves then move in lockstep.  Below that boundary W
// is staged once per F-tile pass and workgroup residency, and the waves run free.
// THE FOLD.  A wave writes 64 columns of its 16 x F_tile tile to its staging rows, then lane l
// walks column l down the 16 rows - increasing p - adding the bias, applying the activation and
// folding into a running value it keeps in a register across tiles; at a segment boundary it
// stores the finished destination.  Tile boundaries therefore never show in the bits, and a hub
// segment is simply many tiles of its owner.
// The grid is capped (kPoolMaxBlocks); a workgroup loops over groups of 4 runs beyond it.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "half_cvt.h"
#include "mp_topk.h"

namespace euler_gpu {

constexpr int kPoolMax = 0, kPoolMean = 1, kPoolAdd = 2;
constexpr int kPoolRelu = 0, kPoolNone = 1;
constexpr int kPoolMaxDim = 4096;
constexpr int kPoolWaves = 4;             // per workgroup
constexpr int kPoolTile = 16;             // gathered rows of a tile; destinations of a run
constexpr int kPoolChunk = 32;            // k per chunk
constexpr int kPoolStageStride = 68;      // floats per staging row: 64 columns + 4 against bank conflicts
constexpr int kPoolStageBytes = kPoolWaves * kPoolTile * kPoolStageStride * 4;
constexpr int kPoolWBytes = 47104;
constexpr int kPoolMaxBlocks = 1024;

struct PoolPlan {
  int32_t nt;         // accumulator fragments of a wave: F_tile = 16 * nt
  int32_t f_passes;   // F-tile passes over the gathered rows
  int32_t k_tile;     // k per staged K tile, a multiple of 32
  int32_t k_tiles;    // 1: W^T of an F tile is staged once per pass
  int32_t k_stride;   // elements between the columns of Wt
  int32_t lds_bytes;  // dynamic LDS of a workgroup
};

inline PoolPlan PoolMakePlan(int64_t d, int64_t f, bool f32) {
  const int32_t esz = f32 ? 4 : 2, pad = 16 / esz;
  const int32_t d32 = (int32_t)((d + kPoolChunk - 1) / kPoolChunk) * kPoolChunk;
  const int32_t f16 = (int32_t)((f + 15) / 16);
  PoolPlan p{};
  p.nt = 8;
  while (p.nt > 1 && (p.nt / 2 >= f16 || (int64_t)16 * p.nt * (d32 + pad) * esz > kPoolWBytes)) p.nt /= 2;
  p.k_tile = d32;
  if ((int64_t)16 * p.nt * (d32 + pad) * esz > kPoolWBytes)
    p.k_tile = (kPoolWBytes / (16 * esz) - pad) / kPoolChunk * kPoolChunk;
  p.k_tiles = (d32 + p.k_tile - 1) / p.k_tile;
  p.k_stride = p.k_tile + pad;
  p.f_passes = (int32_t)((f + 16 * p.nt - 1) / (16 * p.nt));
  p.lds_bytes = kPoolStageBytes + 16 * p.nt * p.k_stride * esz;
  return p;
}

// May A go from global memory in 16-byte loads?
inline bool PoolVectorLoads(int64_t d, uintptr_t table, bool f32) { return table % 16 == 0 && d % (f32 ? 4 : 8) == 0; }

// Boundary value i of a run that starts at destination r0: the begin of destination r0 + i, kept
// inside [0, e] (the caller makes the values of a run non-decreasing)
EG_MPW_HD int64_t PoolBoundary(const int64_t* seg_ptr, int64_t count, int64_t e, int64_t r) {
  const int64_t v = seg_ptr ? seg_ptr[r] : r * count;
  return v < 0 ? 0 : (v > e ? e : v);
}

EG_MPW_HD float PoolAct(int32_t act, float x) { return act == kPoolRelu ? (x <= 0.f ? 0.f : x) : x; }

// term v of a segment into the running value m; first: v is the segment's first term
EG_MPW_HD float PoolFold(int32_t op, float m, float v, bool first) {
  if (first) return v;
  if (op == kPoolMax) return ((v > m) | (v != v)) ? v : m;
  return m + v;
}

// the finished value of a segment of `len` terms
EG_MPW_HD float PoolFinish(int32_t op, float m, int64_t len) {
  if (len == 0) return 0.f;
  return op == kPoolMean ? m * (1.f / (float)len) : m;
}

}  // namespace euler_gpu
