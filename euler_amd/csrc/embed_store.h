// In-place embedding stores - the three operations ScalableSage / ScalableGCN apply to their
// per-layer [max_id + 1, d] stores (tf_euler/python/utils/embedding.py:24-68, encoders.py:713-748):
// update (tf.scatter_update), add (tf.scatter_add) and take (embedding_lookup, optionally followed
// by the clearing embedding_update(..., zeros) of encoders.py:738-743).  THE CONTRACT is stated
// here once; the pieces below are shared by the kernels of embed_store_kernels.hip and by
// tests/csrc/embed_store_check.cc, which compiles this file with the host compiler.
//
// table  [rows, d], contiguous, fp32 / bf16 / fp16, rows >= 1; MODIFIED IN PLACE.
// ids    signed int64 [e], as the samplers return them; the row index is the id itself.
// RANGE RULE (that of kg_score.h): an id outside [0, rows) names no row.  It is never
// dereferenced; it is left out of update / add and reads as a row of +0 in take.
// An OCCURRENCE is a position p in ids.  Its source row is values[p], or values[row_index[p]]
// (int32 [e], values [m, d]; an entry outside [0, m) removes the occurrence - range rule), or
// values[p / count] (count > 0, e % count == 0, m = e / count: the gradient of a mean / sum over
// `count` sampled neighbours, broadcast from its [m, d] row - the [e, d] block never exists).
// values is fp32 or the table's dtype: widening is exact, narrowing is ONE round to nearest even
// (half_cvt.h).
//
//   update  for every distinct in-range id: table[id] = round(source row of its LAST occurrence)
//           (tf.scatter_update on the CPU: a sequential loop over p).  Same dtype: the bits are
//           copied, -0 and NaN payloads included.
//   add     for every distinct in-range id: acc = widen(table[id]); for its occurrences in
//           increasing p: acc = fl32(acc + widen(source row)) - one correctly rounded fp32 add per
//           occurrence and column; then table[id] = round(acc), one rounding.  No float atomics.
//   take    out[p] = table[ids[p]] as it was BEFORE the call, for every occurrence, duplicates
//           included; out is [e, d] in the table's dtype (bits copied) or fp32 (widened).  With
//           clear != 0 every row named by an in-range id is +0 afterwards.
// e == 0 or d == 0: nothing is touched.  Rows not named by any id keep their bits.
//
// HOW: the occurrences are grouped by a STABLE sort of (key, position) with key = the id of a live
// occurrence and `rows` for one the range rule removed (those sort last); only the bits `rows`
// needs take part.  In the sorted array a run of equal keys is a SEGMENT with its positions in
// increasing order: its first element is the HEAD, its last the TAIL - the last occurrence.  One
// owner (L lanes of a wave) per segment reads the table row once, walks the segment in position
// order and writes the row once; no other lane touches that row, which makes "before the call" of
// take and the order of add structural.  Lanes run over chunks of V adjacent columns, V = 8 / 4 /
// 1 by d % V and the alignment of table, values and out.  There is NO sum across columns here:
// every column is a chain of its own, so V, L and the launch geometry cannot change any bit.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "half_cvt.h"
#include "mp_weighted.h"

namespace euler_gpu {

constexpr int kEsUpdate = 0, kEsAdd = 1, kEsTakeClear = 2, kEsTake = 3;

EG_MPW_HD bool EsInRange(int64_t id, int64_t rows) { return id >= 0 && id < rows; }

// Is occurrence p live under its row_index entry (the other two forms always are)?
EG_MPW_HD bool EsSourceLive(int64_t p, const int32_t* row_index, int64_t m) {
  return !row_index || (row_index[p] >= 0 && (int64_t)row_index[p] < m);
}

// The row of `values` a live occurrence p reads.
EG_MPW_HD int64_t EsSourceRow(int64_t p, const int32_t* row_index, int64_t count) {
  if (row_index) return row_index[p];
  return count > 0 ? p / count : p;
}

// The sort key of occurrence p: its id, or `rows` when the range rule removed it.
EG_MPW_HD uint64_t EsKey(int64_t id, int64_t rows, bool source_live) {
  return EsInRange(id, rows) && source_live ? (uint64_t)id : (uint64_t)rows;
}

// The number of low bits in which the keys 0 .. rows differ
inline int32_t EsKeyBits(int64_t rows) {
  int32_t b = 1;
  while (b < 63 && ((int64_t)1 << b) <= rows) ++b;
  return b;
}

// Over the stably sorted keys [e]: sorted index i starts / ends a run of equal keys.  The tail of
// a run holds the LAST occurrence of its id (positions increase inside a run).
EG_MPW_HD bool EsIsHead(const uint64_t* keys, int64_t i) { return i == 0 || keys[i - 1] != keys[i]; }
EG_MPW_HD bool EsIsTail(const uint64_t* keys, int64_t i, int64_t e) { return i + 1 == e || keys[i + 1] != keys[i]; }

// An element is carried as its bits in a uint32 (fp32: all 32, 16-bit types: the low 16).
template <int DT>
EG_MPW_HD float EsWiden(uint32_t raw) {
  if constexpr (DT == kF32) return BitsF32(raw);
  else return HalfCvt<DT>::Widen((uint16_t)raw);
}
template <int DT>
EG_MPW_HD uint32_t EsNarrow(float f) {
  if constexpr (DT == kF32) return F32Bits(f);
  else return HalfCvt<DT>::Narrow(f);
}
// An element of type FROM stored as type TO (FROM == TO: the bits; else through fp32, where
// widening is exact and narrowing rounds once)
template <int FROM, int TO>
EG_MPW_HD uint32_t EsConvert(uint32_t raw) {
  if constexpr (FROM == TO) return raw;
  else return EsNarrow<TO>(EsWiden<FROM>(raw));
}

// The add step: one correctly rounded fp32 add of the widened source element
template <int DV>
EG_MPW_HD float EsAddStep(float acc, uint32_t raw) { return MpwAdd(acc, EsWiden<DV>(raw)); }

// V, given d and the addresses and element sizes of the buffers a call touches (0: not used)
inline int32_t EsChunkWidth(int64_t d, uintptr_t table, int table_bytes, uintptr_t other, int other_bytes) {
  const bool a16 = table % 16 == 0 && other % 16 == 0;
  const bool a4 = table % (table_bytes == 4 ? 16 : 8) == 0 && other % (other_bytes == 4 ? 16 : 8) == 0;
  return (d % 8 == 0 && a16) ? 8 : (d % 4 == 0 && a4) ? 4 : 1;
}

// log2 L, given the number of chunks of a row
inline int32_t EsLogLanes(int64_t chunks) {
  int32_t log_l = 0;
  while (log_l < 6 && ((int64_t)1 << log_l) < chunks) ++log_l;
  return log_l;
}

}  // namespace euler_gpu
