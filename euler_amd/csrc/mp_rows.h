// Full-neighbour aggregation read straight from the graph's rows: the contract and the arithmetic
// of ONE queried node, shared by neighbor_reduce_kernels.hip and by
// tests/csrc/neighbor_reduce_check.cc, which compiles it with the host compiler.
//
// THE UPDATES OF ONE QUERIED NODE.  For queried node i with id nodes[i], the updates are the
// entries of its row's listed edge-type groups, enumerated exactly as euler_gpu_get_full_neighbor
// enumerates them (core/graph/node.cc:175-197): groups in the order the types are listed; a type
// listed twice is read twice; a type outside [0, T) is skipped; a node without a row gives an
// empty segment.
//
// WHAT UPDATE p READS.  Table row min((uint32) low word of nbr[p], table_rows - 1) - the rule of
// euler_gpu_gather_segment_reduce_ids.  Tables are id-indexed, like every table op here;
// row-indexed tables for hashed-id graphs are out of scope.
//
// WEIGHT KINDS.
//   0 none: the plain reduce (the weight is 1.0f, and x * 1.0f is exact).
//   1 edge: w = fl(prefix_w[p] - (p == 0 ? 0 : prefix_w[p - 1])), p the position in the WHOLE row
//           (not in its group): the bit pattern get_full_neighbor returns.
//   2 norm: w = fl(norm_dst[i] * norm_src[g]) for the neighbour's index g = (uint32) low word of
//           nbr[p], norm_src an fp32 table of table_rows entries; 0 when g >= table_rows
//           (GcnNormOps's rule, mp_gcn.h).
//
// ARITHMETIC (the rules of mp_weighted.h).  Message fl(x * w); the sum a separate rounded add, in
// the enumerated order, starting at +0; max starts from -1e9; mean divides by (length + 1e-7f).
//
// self_loop != 0 appends one more update after the listed ones: the table row of nodes[i] itself,
// under the same clamp rule, with weight 1.0f for kinds 0 and 1 and fl(norm_dst[i] *
// norm_src[nodes[i]]) for kind 2 (0 past the table, as every update of that kind).  It counts in
// the mean's length, and it is appended whether or not the node has a row - where
// full_blocks(add_self_loops=True) puts it.
//
// ROOT EPILOGUE.  GcnRootEpilogue unchanged: fl(fl(agg * a) + fl(root[i] * b)).
//
// BIT EQUALITY WITH THE COMPOSITION.  The result is, bit for bit, what get_full_neighbor, then the
// ids / weights (with the self id appended per segment), then gather_segment_reduce(...,
// seg_ptr=..., edge_weight=...) or gcn_aggregate(...) give, on any input that composition accepts;
// totals of 2^31 listed entries and more, which it refuses, are served too.
//
// LIMITS.  n < 2^31 queried nodes, table_rows in [1, 2^31), k <= kMaxListedTypes.
//
// The loads of a group are issued eight (then four, then one) updates at a time (MpwBatch), and
// the fold stays in the enumerated order.  A batch never spans two groups; where a batch ends is
// no part of the bits.  No HIP header is needed: a host-only program may include this file on its
// own.
#pragma once

#include <stdint.h>

#include "mp_gcn.h"
#include "mp_weighted.h"

namespace euler_gpu {

EG_MPW_HD float MpwSub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fsub_rn(a, b);
#else
  return a - b;
#endif
}

constexpr int kRowWeightNone = 0, kRowWeightEdge = 1, kRowWeightNorm = 2;
constexpr int64_t kRowSelfPos = -1;      // the position that names the appended self update

// Ops of MpwBatch whose segment is a graph row.  nbr_lo / prefix_w point at the ROW's first entry
// (nbr_lo at the 32-bit words of its uint64 ids: word 2 p is the low word of entry p, little
// endian); a position is row-absolute, kRowSelfPos the self update.
template <int KIND, typename Loader>
struct RowOps {
  using Raw = typename Loader::Raw;
  Loader ld;
  const uint32_t* nbr_lo;
  const float* prefix_w;
  const float* norm_src;     // kind 2: [rows]
  uint32_t rows;
  float nd;                  // kind 2: norm_dst[i]
  uint32_t self_lo;          // low word of nodes[i]
  EG_MPW_HD uint32_t Index(int64_t pos) const { return pos == kRowSelfPos ? self_lo : nbr_lo[2 * pos]; }
  EG_MPW_HD int64_t Pos(int64_t p) const { return p; }
  EG_MPW_HD int64_t Row(int64_t pos) const {
    const uint32_t g = Index(pos);
    return (int64_t)(g < rows - 1 ? g : rows - 1);
  }
  EG_MPW_HD float Weight(int64_t pos) const {
    if (KIND == kRowWeightEdge) {
      if (pos == kRowSelfPos) return 1.0f;
      return MpwSub(prefix_w[pos], pos == 0 ? 0.f : prefix_w[pos - 1]);
    }
    if (KIND == kRowWeightNorm) {
      const uint32_t g = Index(pos);
      return g < rows ? MpwMul(nd, norm_src[g]) : 0.f;
    }
    return 1.0f;
  }
  EG_MPW_HD Raw Load(int64_t row) const { return ld.Load(row); }
  EG_MPW_HD void Widen(const Raw& v, float* f) const { ld.Widen(v, f); }
};

// The listed edge types of a call, as the kernels take them by value.
struct RowTypeList {
  int32_t k;
  int32_t T;                 // edge-type groups of a row
  int32_t et[32];            // (kMaxListedTypes)
};

// The listed degree of a row whose cumulative group ends are type_end[T] (nullptr: no row):
// FullNbCount's sum, plus the self update.
EG_MPW_HD int64_t RowListedDegree(const RowTypeList& L, const int32_t* type_end, bool self_loop) {
  int64_t c = self_loop ? 1 : 0;
  if (type_end == nullptr) return c;
  for (int32_t x = 0; x < L.k; ++x) {
    const int32_t t = L.et[x];
    if (t >= 0 && t < L.T) c += type_end[t] - (t == 0 ? 0 : type_end[t - 1]);
  }
  return c;
}

// acc[0..N) = the reduce (MODE 0 add, 1 max, 2 mean) of N adjacent columns of queried node i over
// its listed groups and, with self_loop, its own row.  type_end == nullptr: the node has no row.
template <int MODE, int N, typename Ops>
EG_MPW_HD void RowReduce(const Ops& o, const RowTypeList& L, const int32_t* type_end, bool self_loop,
                         float acc[N]) {
  const float init = MODE == 1 ? (float)-1e9 : 0.f;
  for (int k = 0; k < N; ++k) acc[k] = init;
  int64_t len = 0;
  if (type_end != nullptr) {
    for (int32_t x = 0; x < L.k; ++x) {
      const int32_t t = L.et[x];
      if (t < 0 || t >= L.T) continue;
      const int64_t b = t == 0 ? 0 : type_end[t - 1], en = type_end[t];
      int64_t p = b;
      for (; p + 8 <= en; p += 8) MpwBatch<MODE, N, 8>(o, p, acc);
      for (; p + 4 <= en; p += 4) MpwBatch<MODE, N, 4>(o, p, acc);
      for (; p < en; ++p) MpwBatch<MODE, N, 1>(o, p, acc);
      len += en - b;
    }
  }
  if (self_loop) {
    MpwBatch<MODE, N, 1>(o, kRowSelfPos, acc);
    ++len;
  }
  if (MODE == 2) {
    const float denom = MpwAdd((float)len, 1e-7f);
    for (int k = 0; k < N; ++k) acc[k] = MpwDiv(acc[k], denom);
  }
}

}  // namespace euler_gpu
