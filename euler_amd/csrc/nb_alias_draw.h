// The alias neighbour draw of one output slot (root, sample j), shared by SampleNeighborAliasKernel
// (nb_alias_kernels.hip) and tests/csrc/nb_alias_check.cc, which runs it on the host.
//
// Row lookup, type modes and validity are the exact mode's (device_fns.h: FindRow, TypeModeOf,
// InitRowSampler - Node::__SampleNeighbor, core/graph/node.cc:98-161): one listed type; a
// sub-collection in the listed order; all groups when k == 0 or k >= T; an invalid type or an empty
// listed group gives a row without samples.  The TYPE of a sample is drawn exactly as the exact mode
// draws it, RandomSelect over the type sums of the row record.  Only the neighbour draw differs:
// AliasMethod::Next (alias_method.cc:66-78) over the group's table (nb_alias.h: NbAliasPick).
//
// RNG: domain 0, stream = the root's node id.  Sample j uses draw indices 4 j (type, only
// when a type is drawn), 4 j + 2 (column) and 4 j + 3 (coin): column and coin are the two halves of
// Philox block 2 j + 1, the type is the first half of block 2 j.  A single-type call computes one
// block per sample.
#pragma once

#include "device_fns.h"
#include "nb_alias.h"

namespace euler_gpu {

// What the samples of one root share, found once per root: `valid`, and
//   one listed type: base = the flat index of the group's first edge, d = its length;
//   a type draw:     base = the root's row (the draw reads the type sums of its record), d unused.
struct NbAliasRoot {
  int64_t base;      // -1: the row has no samples
  int32_t d;
};

EG_HD NbAliasRoot NbAliasRootOf(const GraphView& g, uint64_t node, const int32_t* edge_types, int32_t k) {
  NbAliasRoot r{-1, 0};
  const int64_t row = FindRow(g, node);
  RowSampler rs;
  InitRowSampler(rs, g, row, edge_types, k);
  if (!rs.valid) return r;
  if (rs.mode == kTypeSingle) {
    const int32_t t = rs.single_type;
    const int32_t b = t == 0 ? 0 : rs.type_end[t - 1];
    r.base = (int64_t)(rs.nbr - g.nbr) + b;
    r.d = rs.type_end[t] - b;
  } else {
    r.base = row;
  }
  return r;
}

// Sample j of a valid root: (id, weight, type).  A type draw that lands on a group without a table
// (an empty one through RandomSelect's fall-through, Q3, or one whose weights are all 0 although its
// type sum is not) gives the sentinel (0, 0.0, 0), as SampleAt does in its unreachable branch; so
// does a single listed type whose group's weights are all 0.
EG_HD void NbAliasSampleAt(const GraphView& g, const NbAliasEntry* tab, const NbAliasRoot& root,
                           const int32_t* edge_types, int32_t k, uint64_t seed, uint32_t call_id,
                           uint64_t node, int32_t j, uint64_t* out_id, float* out_w, int32_t* out_t) {
  const int32_t mode = TypeModeOf(k, g.T);
  int32_t t, d = root.d;
  int64_t first = root.base;
  if (mode == kTypeSingle) {
    t = edge_types[0];
  } else {
    const Philox4 tb = RngBlock(seed, call_id, kDomainNeighbor, node, 2u * (uint32_t)j);
    const double u_type = UnitFromWords(tb.w[0], tb.w[1]);
    const RowMeta m = LoadRowMeta(g, root.base);
    if (mode == kTypeSub) {
      const SubTypeSum sub{m.type_prefix, edge_types};
      t = edge_types[RandomSelectT(sub, 0, (uint64_t)(k - 1), u_type)];
    } else {
      t = (int32_t)RandomSelect(m.type_prefix, 0, (uint64_t)(g.T - 1), u_type);
    }
    const int32_t b = t == 0 ? 0 : m.type_end[t - 1];
    d = m.type_end[t] - b;
    first = m.row_ptr + b;
  }
  uint64_t id = 0;
  float w = 0.f;
  if (d > 0) {
    const Philox4 nb = RngBlock(seed, call_id, kDomainNeighbor, node, 2u * (uint32_t)j + 1u);
    NbAliasPick(tab + first, d, UnitFromWords(nb.w[0], nb.w[1]), UnitFromWords(nb.w[2], nb.w[3]), &id, &w);
  }
  // a table never yields weight 0 (nb_alias.h: the fix-up): weight 0 = the group has none
  if (w == 0.f) { id = 0; t = 0; }
  *out_id = id; *out_w = w; *out_t = t;
}

// The output slot (root, j) under the conventions of euler_gpu_sample_neighbor: LAYOUT_CORE fills a
// row without samples with (0, 0.0, 0), LAYOUT_TF with (default_node, 0.0, -1) - and drops a row
// whose FIRST id is the sentinel 0 (tf_euler/kernels/sample_neighbor_op.cc:114-122, Q1), which only
// graphs with a neighbour id 0 can have on a live row.  *masked: the row is a default row.
EG_HD void NbAliasSlot(const GraphView& g, const NbAliasEntry* tab, const NbAliasRoot& root,
                       const int32_t* edge_types, int32_t k, uint64_t seed, uint32_t call_id, uint64_t node,
                       int32_t j, bool tf, int64_t default_node, uint64_t* out_id, float* out_w,
                       int32_t* out_t, bool* masked) {
  uint64_t id = 0;
  float w = 0.f;
  int32_t t = 0;
  bool drop = root.base < 0;
  if (!drop) {
    NbAliasSampleAt(g, tab, root, edge_types, k, seed, call_id, node, j, &id, &w, &t);
    if (tf) {
      if (j == 0) {
        drop = id == 0;
      } else if (g.has_zero_nbr || w == 0.f) {
        // (w == 0: a group without a table gives id 0 in every slot, the first one included)
        uint64_t id0; float w0; int32_t t0;
        NbAliasSampleAt(g, tab, root, edge_types, k, seed, call_id, node, 0, &id0, &w0, &t0);
        drop = id0 == 0;
      }
    }
  }
  if (drop) { id = tf ? (uint64_t)default_node : 0; w = 0.f; t = tf ? -1 : 0; }
  *out_id = id; *out_w = w; *out_t = t; *masked = drop;
}

}  // namespace euler_gpu
