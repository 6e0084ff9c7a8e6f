// Graph::from_edges: an edge list on the device -> the rows of a graph, on the device, with the
// bits BuildGraphFromHost produces from the same edges laid out by the reference's rules
// (GraphBuilder::Build + Node::Init, core/graph/node.cc:46-66; restated in oracle/euler_oracle.c:
// eo_build_prefix).  edge_build_kernels.hip holds the passes; graph_build.hip puts the graph
// together around them (search index, node sampler, commit).
//
// The edge list the passes see has `total` entries: the E given ones and, when undirected, all of
// them reversed behind those (entry E + e = edge e with src and dst exchanged, its type and weight
// copied).  The reversed half is never written anywhere: every pass reads entry p of the list
// through the four input arrays.
//
// Passes, in order, and what each moves per entry of the list (k = 4-byte keys while N * T <=
// 2^32, else 8; every pass runs on the caller's stream):
//   rows, nodes NULL   src and dst -> one array of 2 E ids, radix sort (64 bits), unique: the rows
//                      are the distinct ids ascending as unsigned numbers.  16 + 16 bytes per given
//                      edge, returned before anything below is taken.
//   rows, nodes given  a copy of the ids; the caller's order is the row order.
//   id map             identity when row r has the id base + r * stride (stride > 0), checked on
//                      the device; else the open-addressing table of common.h (Mix64, linear
//                      probes, at most half full).  A slot is claimed through its ROW word, so an
//                      id of 0 - which the synthetic path's claim through the key word excludes -
//                      is a key like any other; a second row with an id already in the table is
//                      found by probing every row's id back (FindRow must answer the row itself).
//   keys               key = row(src) * T + type and the entry's position: k + 4 bytes written.  A
//                      type outside [0, T) and a src that is no row are counted here.
//   sort               stable LSD radix sort of (key, position) over exactly the bits N * T - 1
//                      has, in double buffers: 2 (k + 4) bytes held.
//   segments           seg[q] = first sorted entry with key >= q, q = 0 .. N * T: 8 (N T + 1) bytes;
//                      row_ptr and type_end are differences of it.  By bisection: (N T + 1) * log2(total)
//                      dependent reads of the sorted keys, against one pass over them for counts +
//                      ExclusiveScanI64 - measured at T = 2 only, not at T = 32.
//   gather             nbr and the raw weight of sorted entry j through its position: 12 bytes
//                      written - these two arrays are the graph's own.
//   prefix             Node::Init per row, in place over the raw weights, and the row's record.
//   flags              has_zero_nbr (gather), monotone and uniform_w (prefix) as
//                      BuildGraphFromHost computes them: plain stores of the value that ends the
//                      property, no scalar path.
//   features           slot f of row r -> feat_val[r * stride + begin(f) ...], one kernel per slot.
//
// Peak temporaries: max(32 E [nodes NULL only], 2 (k + 4) total + 8 (N T + 1) + 8 (total / 65 + 1))
// bytes plus hipcub's scratch (a few MB: the double buffers are the sort's own alternates) - 16
// bytes per entry of the list while N * T <= 2^32.  All of it is returned before BuildSearchIndex
// runs.
//
// Why the prefix is no scan: prefix_w[j] is the f32 sum ((w0 + w1) + w2) + ... in entry order, and
// a tree or a segmented scan adds the same numbers in another order - other floats (2^24 + 1 + 1
// is 2^24, 1 + 1 + 2^24 is 2^24 + 2).  So the adds of a row stay one chain.  A row of up to
// kEbLaneRow entries is one lane's; a longer row is one wave's: the wave loads kEbChunk weights
// into LDS with coalesced loads, lane 0 walks them in order (its loads are LDS reads, not one
// dependent HBM load per add), and all lanes store the sums and test the flags.
//
// Limits: total (E, or 2 E when undirected) < 2^31 - a position is a uint32 and type_end an int32;
// no row can then reach 2^31 entries.  hipcub's item counts are 64-bit here, so the sort itself
// sets no limit below that.
#pragma once

#include "common.h"
#include "device_mem.h"

namespace euler_gpu {
#pragma GCC visibility push(hidden)

constexpr int kEbLaneRow = 64;       // rows up to this many entries: one lane each
constexpr int kEbChunk = 1024;       // weights a wave stages per step of a longer row

// The passes a build is timed by (euler_gpu_graph_from_edges_pass_ms): the stream is drained after
// each, which a build - that returns a finished graph - can afford.
enum EbPass {
  kEbRows = 0, kEbIdMap, kEbKeys, kEbSort, kEbSegments, kEbGather, kEbPrefixLane, kEbPrefixWave,
  kEbFeatures, kEbSearchIndex, kEbNodeSampler, kEbPasses
};

// What a build from edges knows beyond the view
struct EdgeBuildFacts {
  uint64_t max_id = 0;
  bool feat_slot_aligned = false;
  const int32_t* node_type_dev = nullptr;
  float pass_ms[kEbPasses] = {};
};

// The argument ladder of euler_gpu_graph_create_from_edges: host arithmetic, before any HIP call.
int CheckDevEdges(const euler_gpu_dev_edges* e, euler_gpu_graph** out);

// graph_build.hip: its HashInitKernel (every slot {key 0, row ~0}) over `cap` slots, enqueued on `st`
void LaunchHashInit(hipStream_t st, uint64_t* slots, uint64_t cap);

// Every pass above on `st`.  The view's row, id-map, flag and feature fields are filled; the
// arrays they point to are blocks of `blocks`.  Returns after the stream has run them all, with
// every temporary returned.
int BuildRowsFromEdges(const euler_gpu_dev_edges* e, hipStream_t st, AllocList* blocks, GraphView* v,
                       EdgeBuildFacts* facts);

#pragma GCC visibility pop
}  // namespace euler_gpu
