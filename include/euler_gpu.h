/*
 * euler_gpu.h - C ABI of the MI355X-native sampling / aggregation backend for
 * Euler's minibatch-construction hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch
 * types.  Each entry point names the reference interface it replaces
 * (paths relative to the alibaba/euler tree).  INTEGRATION.md shows the
 * binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - Every function returns 0 on success or a negative EULER_GPU_E* code; the
 *     message is available from euler_gpu_last_error() (thread-local).  This
 *     mirrors the reference's "log and produce no output" error behaviour
 *     (core/kernels/sample_node_op.cc:118-122) with a code the caller can test.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 *     device work is enqueued on it; nothing synchronises unless documented.
 *   - Pointers named *_dev are device (HBM) pointers, *_host are host
 *     pointers.  Outputs are caller-allocated; their sizes are static
 *     (n * count ...), exactly the shapes of the reference ops.
 *   - Node ids are uint64 (euler::common::NodeID); the TF-level ops read and
 *     write them as int64 bit patterns (tf_euler/kernels/sample_neighbor_op.cc:110).
 *   - Random numbers: counter-based Philox4x32-10 keyed by (seed, call_id,
 *     node id | sample index, draw index) - see DESIGN.md "RNG contract".  The
 *     same (seed, call_id) always reproduces the same ids, independent of batch
 *     order, duplication, launch geometry or sharding.
 */
#ifndef EULER_GPU_H_
#define EULER_GPU_H_

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EULER_GPU_OK 0
#define EULER_GPU_EINVAL (-1)   /* bad argument                                */
#define EULER_GPU_ENOMEM (-2)   /* device or host allocation failed            */
#define EULER_GPU_EHIP (-3)     /* HIP runtime error (message has the detail)  */
#define EULER_GPU_ENOGRAPH (-4) /* no graph initialised / bad handle           */
#define EULER_GPU_EIO (-5)      /* data_path unreadable / malformed .dat       */
#define EULER_GPU_EEMPTY (-6)   /* sampler has zero total weight: no output    */

typedef struct euler_gpu_graph euler_gpu_graph;

/* Result layouts of the neighbour sampler. */
#define EULER_GPU_LAYOUT_CORE 0 /* API_SAMPLE_NB / GQL layout: empty rows are
                                   count x (0, 0.0f, 0)
                                   (core/kernels/sample_neighbor_op.cc:134-143) */
#define EULER_GPU_LAYOUT_TF 1   /* tf_euler dense layout: rows whose first id
                                   is the sentinel 0 are default_node/0.0/-1
                                   (tf_euler/kernels/sample_neighbor_op.cc:79-81,
                                   114-122)                                     */

/* Host description of a graph in the reference's own per-node storage
 * (euler/core/graph/node.h:49-57) concatenated over rows. */
typedef struct euler_gpu_host_csr {
  int64_t n_rows;
  int32_t n_edge_types;        /* edge-type groups per node                    */
  int32_t n_node_types;
  const uint64_t* row_id;      /* [n_rows] node id of each row                 */
  const int64_t* row_ptr;      /* [n_rows+1]                                   */
  const int32_t* type_end;     /* [n_rows*T] neighbor_groups_idx (row-relative)*/
  const uint64_t* nbr;         /* [E] neighbors                                */
  const float* prefix_w;       /* [E] neighbors_weight (running f32 sums)      */
  const float* type_prefix;    /* [n_rows*T] edge_group_collection running sums*/
  const int32_t* node_type;    /* [n_rows] or NULL (all type 0)                */
  const float* node_weight;    /* [n_rows] or NULL (all 1.0f)                  */
  const uint64_t* sampler_order; /* [n_rows] node ids in the order the global
                                  node sampler enumerates them
                                  (Graph::BuildGlobalSampler, graph.cc:349) or
                                  NULL = row order                             */
  /* dense float features, the reference's per-node float_features_idx_ /
   * float_features_ (core/graph/node.h): optional (n_float_features = 0) */
  int32_t n_float_features;    /* feature slots per node                       */
  int32_t pad0;
  const int64_t* feat_ptr;     /* [n_rows+1] offset of each row's values        */
  const int32_t* feat_idx;     /* [n_rows*F] cumulative ends per slot,
                                  row-relative; a missing slot repeats the
                                  previous end                                 */
  const float* feat_val;       /* [feat_ptr[n_rows]]                            */
  /* sparse (uint64) features, the reference's uint64_features_idx_ /
   * uint64_features_ (core/graph/node.h), same layout: optional */
  int32_t n_u64_features;
  int32_t pad1;
  const int64_t* ufeat_ptr;    /* [n_rows+1]                                    */
  const int32_t* ufeat_idx;    /* [n_rows*U] cumulative ends per slot           */
  const uint64_t* ufeat_val;   /* [ufeat_ptr[n_rows]]                           */
} euler_gpu_host_csr;

/* Host description of Edge records (core/graph/edge.h: id_ = (src, dst, type), weight_ and the
 * uint64 / float / binary feature idx + value lists) in ORDINAL order: a record's ordinal is its
 * position here, the order every edge entry point below uses.  Feature tables have the layout of
 * euler_gpu_host_csr's (ptr [n+1], per-slot ends [n * slots] row-relative, values); binary
 * values are bytes.  A table with 0 slots may have NULL arrays. */
typedef struct euler_gpu_host_edges {
  int64_t n;
  int32_t n_edge_types;        /* euler.meta's edge type count (0 = not known)    */
  int32_t pad0;
  const uint64_t* src;         /* [n]                                             */
  const uint64_t* dst;         /* [n]                                             */
  const int32_t* type;         /* [n]                                             */
  const float* weight;         /* [n]                                             */
  int32_t n_float_features;
  int32_t n_u64_features;
  int32_t n_binary_features;
  int32_t pad1;
  const int64_t* feat_ptr;  const int32_t* feat_idx;  const float* feat_val;
  const int64_t* ufeat_ptr; const int32_t* ufeat_idx; const uint64_t* ufeat_val;
  const int64_t* bfeat_ptr; const int32_t* bfeat_idx; const uint8_t* bfeat_val;
} euler_gpu_host_edges;

/* Parameters of the deterministic synthetic power-law graph (benchmarks). */
typedef struct euler_gpu_synth_params {
  uint64_t seed;
  int64_t n_nodes;             /* ids 1..n_nodes                               */
  int64_t n_edges_target;
  int32_t scale;               /* RMAT scale (bits)                            */
  int32_t n_types;
  int32_t weighted;            /* 0: all weights 1.0f, 1: uniform [0.5, 8)     */
  int32_t hashed_ids;          /* 1: node x (1..n_nodes) carries the external id mix64(x), a
                                * bijection of u64 - arbitrary ids, hash id map - instead of x  */
  double deg_table[64];        /* expected extra degree by popcount(id-1)      */
} euler_gpu_synth_params;

/* ---- library / error ---------------------------------------------------- */
const char* euler_gpu_last_error(void);
const char* euler_gpu_version(void);
int euler_gpu_device_count(void);

/* ---- graph life cycle ---------------------------------------------------
 * Replaces QueryProxy::Init local branch -> Graph::Init -> GraphBuilder::Build
 * -> BuildGlobalSampler (client/query_proxy.cc:145-190, core/graph/graph.cc:
 * 72-120,333-370): the graph becomes an immutable CSR + alias tables in HBM. */
int euler_gpu_graph_create(const euler_gpu_host_csr* csr, int device,
                           euler_gpu_graph** out);
/* Only rows owned by `shard_index` under owner(id) = (id % partitions) % shards
 * (core/kernels/id_split_op.cc:46-49) are kept (Graph::Init file filter,
 * core/graph/graph.cc:90-98). */
int euler_gpu_graph_create_shard(const euler_gpu_host_csr* csr, int device,
                                 int32_t partitions, int32_t shard_index,
                                 int32_t shards, euler_gpu_graph** out);
/* Synthetic graph generated directly in HBM.  rows are [row_begin,row_end) of
 * the global graph when sharded by contiguous ranges is wanted; pass
 * partitions/shards = 1 for the whole graph.  With shards > 1 the shard keeps
 * the nodes with owner(id) == shard_index. */
int euler_gpu_graph_create_synthetic(const euler_gpu_synth_params* p,
                                     int device, int32_t partitions,
                                     int32_t shard_index, int32_t shards,
                                     euler_gpu_graph** out);
/* An edge list in device memory, as OGB, PyG and most pipelines hand a graph over.  Every array is
 * read only.  features / feature_dims are HOST arrays (of device pointers and of widths). */
typedef struct euler_gpu_dev_edges {
  int64_t n_edges;             /* E                                                       */
  int64_t n_nodes;             /* N, the length of nodes (not looked at when nodes NULL)  */
  int32_t n_edge_types;        /* T: 1 .. 32                                              */
  int32_t undirected;          /* != 0: the list is the E edges, then all of them reversed */
  const uint64_t* src;         /* [E] device                                              */
  const uint64_t* dst;         /* [E] device                                              */
  const int32_t* type;         /* [E] device, or NULL (all type 0)                        */
  const float* weight;         /* [E] device, or NULL (all 1.0f)                          */
  const uint64_t* nodes;       /* [N] device: the rows, in this order; or NULL            */
  const int32_t* node_type;    /* [N] device or NULL (all type 0); needs nodes            */
  const float* node_weight;    /* [N] device or NULL (all 1.0f); needs nodes              */
  int32_t n_node_types;        /* 0 .. 32; 0 = 1                                          */
  int32_t node_sampler;        /* != 0: build the global node sampler over the rows       */
  int32_t n_features;          /* dense feature slots; needs nodes                        */
  int32_t pad0;
  const float* const* features;  /* HOST [n_features]: device pointers to [N, dim] fp32   */
  const int32_t* feature_dims;   /* HOST [n_features]: the widths, each >= 1             */
} euler_gpu_dev_edges;
/* The graph of an edge list, built on the device: replaces GraphBuilder::Build + Node::Init
 * (core/graph/graph_builder.cc:57-158, core/graph/node.cc:46-66) over files the reference's
 * converters wrote, and the host pass of euler_gpu_graph_create.  The result is the graph
 * euler_gpu_graph_create makes from the same edges laid out by the reference's rules - the same
 * bytes in every row array, the same output of every seeded call:
 *   rows     nodes NULL: one per distinct id of src and dst, ascending as UNSIGNED 64-bit numbers;
 *            nodes given: exactly those, in that order - an id twice is refused, an edge whose
 *            src is not among them is refused, a dst that is not among them stays a neighbour
 *            without a row.  A node without out-edges is a row of degree 0.
 *   entries  of a row: grouped by type 0 .. T-1, within a (row, type) group in the order of the
 *            list (the sort is stable); repeated edges are all kept.
 *   weights  prefix_w is the sequential fp32 sum over the whole row, type_prefix the running sum
 *            of each group's own sequential fp32 sum (Node::Init); weights are not validated.
 *   id map   the strided identity when row r has the id base + r * stride, stride > 0; else the
 *            hash table.  has_zero_nbr / monotone / uniform_w as euler_gpu_graph_create sets them.
 *   features the uniform layout: a row's slots side by side, feat_stride = the sum of the widths.
 *   sampler  node_sampler != 0: Graph::BuildGlobalSampler over the rows in row order (the ids,
 *            types and weights are copied to the host for it); 0: none, as a synthetic graph, for
 *            a later euler_gpu_graph_set_node_sampler.  node_type is kept either way.
 * The work runs on `stream` (a hipStream_t; NULL = the null stream) and the call returns when the
 * graph is complete.  Temporaries peak at 16 bytes per entry of the list (24 when N * T > 2^32)
 * plus 8 (N * T + 1), or at 32 E while the rows of a nodes == NULL call are found, and are
 * returned before the search index is built (csrc/edge_build.h has the passes).
 * E = 0 and N = 0 are graphs.  EULER_GPU_EINVAL, checked in this order before the first HIP call:
 * a null argument; a negative size; T outside 1 .. 32; n_node_types outside 0 .. 32; a null src
 * or dst with E > 0; features, node_type or node_weight without nodes; a null features /
 * feature_dims array or entry, a width < 1, widths summing to 2^31 or more; a buffer not aligned
 * to its type; E (2 E when undirected) >= 2^31 - a position in the list is a uint32 and type_end an
 * int32, so no row can reach 2^31 entries either (hipcub's own item counts are 64-bit).  Found on
 * the device, with the count in the message: a type outside [0, T); a src that is no row; an id
 * twice in nodes.  On any failure *out is NULL and nothing stays allocated. */
int euler_gpu_graph_create_from_edges(const euler_gpu_dev_edges* edges, int device, void* stream,
                                      euler_gpu_graph** out);
/* Load a directory written by euler/tools (euler.meta + Node/<x>_<partition>.dat), the
 * input of the reference's Graph::Init (core/graph/graph_builder.cc:57-158,
 * core/graph/node.cc:414-526). */
int euler_gpu_graph_load(const char* data_path, int device,
                         int32_t shard_index, int32_t shards,
                         euler_gpu_graph** out);
/* Host-only view of the same reader (no GPU needed): parses the directory
 * into malloc'ed arrays described by *csr; free with euler_gpu_dat_close().
 * *partitions receives euler.meta's partitions_num. */
int euler_gpu_dat_open(const char* data_path, int32_t shard_index,
                       int32_t shards, euler_gpu_host_csr* csr,
                       int32_t* partitions, void** owner);
void euler_gpu_dat_close(void* owner);
/* Host-only check of a dataset (no GPU needed): every record of the Edge partition files (the
 * (src, dst, type) the reference's EdgeExist consults, core/api/api.cc:46-48,
 * core/graph/edge.cc:136-153) against the node rows this backend answers
 * SparseGetAdj from.  The two agree exactly when *not_in_rows == 0 and
 * *edge_records == *row_triples (distinct (src, dst, type) entries of the rows). */
int euler_gpu_dat_verify_edges(const char* data_path, int32_t shard_index, int32_t shards,
                               int64_t* edge_records, int64_t* not_in_rows,
                               int64_t* row_triples);
/* Host-only Edge reader (no GPU needed): Edge/<x>_<partition>.dat records (Edge::DeSerialize,
 * core/graph/edge.cc:136-200) of the files the shard keeps (Graph::Init's filter,
 * core/graph/graph.cc:90-98) in sorted file order; a repeated (src, dst, type) keeps its first
 * record (Graph::AddEdgeFrom(vector) inserts, core/graph/graph.cc:197-203).  *edges describes
 * malloc'ed arrays owned by *owner; free with euler_gpu_dat_close().  A truncated or malformed
 * record: EULER_GPU_EIO. */
int euler_gpu_dat_open_edges(const char* data_path, int32_t shard_index, int32_t shards,
                             euler_gpu_host_edges* edges, void** owner);
/* The binary node features of a euler_gpu_dat_open owner (Node::DeSerialize keeps them,
 * core/graph/node.cc:515-523): ragged layout (ptr [n_rows+1], ends [n_rows * slots], bytes). */
int euler_gpu_dat_node_binary(const void* owner, int32_t* n_slots, const int64_t** ptr,
                              const int32_t** idx, const uint8_t** val);
/* euler.meta's feature tables (GraphMeta::GetFeatureInfo / GetEdgeFeatureInfo,
 * core/graph/graph_meta.h:97-105): `name` exactly as written there ("dense_f3"); edge = 0 the
 * node table, 1 the edge table.  *type: 0 sparse (uint64), 1 dense (float), 2 binary;
 * *slot: the feature's index among its type; *dim.  An unknown name: EULER_GPU_EINVAL. */
int euler_gpu_dat_feature_info(const char* data_path, int32_t edge, const char* name,
                               int32_t* type, int32_t* slot, int64_t* dim);
void euler_gpu_graph_destroy(euler_gpu_graph* g);

int64_t euler_gpu_graph_num_nodes(const euler_gpu_graph* g);
int64_t euler_gpu_graph_num_edges(const euler_gpu_graph* g);
int32_t euler_gpu_graph_num_edge_types(const euler_gpu_graph* g);
int32_t euler_gpu_graph_num_node_types(const euler_gpu_graph* g);
int euler_gpu_graph_device(const euler_gpu_graph* g);
/* Total device bytes held by the graph. */
int64_t euler_gpu_graph_bytes(const euler_gpu_graph* g);
/* euler.meta's partitions_num of a graph loaded with euler_gpu_graph_load (0 for a
 * graph built from arrays): a multi-GPU sampler must route ids with
 * owner(id) = (id % partitions) % shards using THIS value, because the loader kept
 * the partition files with file_idx % shards == shard_index
 * (core/graph/graph.cc:90-98). */
int32_t euler_gpu_graph_partitions(const euler_gpu_graph* g);
/* Per node type weight sums (Graph::GetNodeWeightSums, used by
 * SAMPLE_NODE_SPLIT); out_host has n_node_types floats. */
int euler_gpu_graph_node_weight_sums(const euler_gpu_graph* g, float* out_host);
/* Graph::BuildGlobalSampler (core/graph/graph.cc:333-370) as a call of its own: the global
 * node sampler (per node type an alias table over weight / type sum, FastWeightedCollection;
 * a type table over the type sums) of a graph that has none - a synthetic one - or in place
 * of the one it has.  The n nodes are taken in the order given, which is the order the
 * reference enumerates node_map_: ids_host NULL = the graph's rows in row order
 * (strided-identity id maps only), types_host NULL = all type 0, weights_host NULL = all
 * 1.0f.  Host work, O(n); not to be called while SampleNode calls are in flight. */
int euler_gpu_graph_set_node_sampler(euler_gpu_graph* g, int64_t n, const uint64_t* ids_host,
                                     const int32_t* types_host, const float* weights_host,
                                     int32_t n_node_types);
/* Copy rows of the device CSR back to the host for the listed ids, in the
 * euler_gpu_host_csr layout (spot checks at sizes no CPU structure can hold).
 * Call with nbr_host == NULL to obtain row_ptr_host (n+1) first. */
int euler_gpu_graph_export_rows(const euler_gpu_graph* g, const uint64_t* ids_host,
                                int64_t n, int64_t* row_ptr_host,
                                int32_t* type_end_host, uint64_t* nbr_host,
                                float* prefix_w_host, float* type_prefix_host);

/* The reference's one process-level C entry (tf_euler/utils/
 * init_query_proxy.cc:19-37, loaded by euler_ops/base.py:33-67).  Accepts the
 * same "k=v;k=v" string (mode=local; data_path; sampler_type; data_type) plus
 * `device`, `shard_idx`, `shard_num` and `verify_edges` (1: refuse a dataset whose
 * Edge records are not exactly the entries of its node rows, see
 * euler_gpu_dat_verify_edges).  Installs the process-wide default graph returned
 * by euler_gpu_default_graph(). */
bool InitQueryProxy(const char* conf);
euler_gpu_graph* euler_gpu_default_graph(void);

/* Largest node id of the graph (shard) and whether its id -> row map is the
 * strided identity (ids = base + stride * row).  A multi-GPU sampler reduces
 * max_id over the shards to size euler_gpu_dedup_split's dense table. */
int euler_gpu_graph_id_range(const euler_gpu_graph* g, uint64_t* max_id_host,
                             int32_t* identity_host);

/* ---- SampleNeighbor ------------------------------------------------------
 * Replaces euler::SampleNeighbor (core/api/api.cc:223-236) ->
 * Node::SampleNeighbor (core/graph/node.cc:98-167) -> RandomSelect
 * (common/compact_weighted_collection.h:30-52), the empty-row fill of
 * API_SAMPLE_NB, FillNeighbor (core/kernels/common.cc:275-334) and, with
 * LAYOUT_TF, the dense repack of the TF SampleNeighbor kernel.
 *   roots_dev      [n] node ids
 *   root_mask_dev  optional [ceil(n / root_group)] bytes; a non-zero byte means
 *                  "this group of roots came from a missing row": they sample
 *                  as node id 0, the id the reference's core tensors carry
 *                  (used to chain hops, tf_euler/kernels/sample_fanout_op.cc)
 *   edge_types_host[k] (k may be 0 = all types)
 *   out_*_dev      [n*count]; out_row_mask_dev optional [n] (1 = default row)
 */
int euler_gpu_sample_neighbor(const euler_gpu_graph* g, void* stream,
                              uint64_t seed, uint32_t call_id,
                              const uint64_t* roots_dev, int64_t n,
                              const uint8_t* root_mask_dev, int32_t root_group,
                              const int32_t* edge_types_host, int32_t k,
                              int32_t count, int32_t layout,
                              int64_t default_node, uint64_t* out_id_dev,
                              float* out_w_dev, int32_t* out_t_dev,
                              uint8_t* out_row_mask_dev);

/* Same call for roots the caller knows to be (mostly) distinct - e.g. the ids a
 * shard receives after euler_gpu_dedup_split: skips the on-device duplicate
 * detection of euler_gpu_sample_neighbor.  Results are identical. */
int euler_gpu_sample_neighbor_distinct(const euler_gpu_graph* g, void* stream,
                                       uint64_t seed, uint32_t call_id,
                                       const uint64_t* roots_dev, int64_t n,
                                       const int32_t* edge_types_host, int32_t k,
                                       int32_t count, int32_t layout,
                                       int64_t default_node, uint64_t* out_id_dev,
                                       float* out_w_dev, int32_t* out_t_dev,
                                       uint8_t* out_row_mask_dev);
/* Several edge-type SETS of one batch of roots in ONE launch - what a heterogeneous
 * (RGCN-style) model issues per minibatch as n_sets SampleNeighbor ops over the same nodes
 * (tf_euler/kernels/sample_neighbor_op.cc:29-132 once per relation set).  Set s lists
 * set_k_host[s] types, taken in order from edge_types_host, and draws with call_id + s; TF
 * layout; out_*_dev hold [n_sets][n][count] elements.  The result equals n_sets calls of
 * euler_gpu_sample_neighbor bit for bit (Node::__SampleNeighbor's type modes,
 * core/graph/node.cc:98-161: one listed type, a sub-collection in the listed order, all
 * groups).  Graphs the one-launch kernel does not serve (running sums that decrease, the
 * id-0 sentinel rule) get the separate calls. */
int euler_gpu_sample_neighbor_sets(const euler_gpu_graph* g, void* stream, uint64_t seed,
                                   uint32_t call_id, const uint64_t* roots_dev, int64_t n,
                                   const int32_t* edge_types_host, const int32_t* set_k_host,
                                   int32_t n_sets, int32_t count, int64_t default_node,
                                   uint64_t* out_id_dev, float* out_w_dev, int32_t* out_t_dev);
/* ... followed, in the same enqueue, by the aggregation of the sampled neighbours' feature
 * rows per (set, root): out_agg_dev [n_sets][n][d] = add / max / mean (mode 0 / 1 / 2) over
 * the `count` rows feat_dev[id] of every root, in sample order - the bits of
 * scatter_(aggr, gather(feat, ids)) (tf_euler/kernels/gather_op.cc, scatter_op.cc;
 * euler_gpu_gather_segment_reduce_ids).  feat_dev is a [feat_rows, d] f32 table indexed by
 * node id; default_node must be one of its rows. */
int euler_gpu_sample_aggregate_sets(const euler_gpu_graph* g, void* stream, uint64_t seed,
                                    uint32_t call_id, const uint64_t* roots_dev, int64_t n,
                                    const int32_t* edge_types_host, const int32_t* set_k_host,
                                    int32_t n_sets, int32_t count, int64_t default_node,
                                    int32_t mode, const float* feat_dev, int64_t feat_rows, int64_t d,
                                    uint64_t* out_id_dev, float* out_w_dev, int32_t* out_t_dev,
                                    float* out_agg_dev);
/* The shard side of a multi-GPU hop in one call: sample the (distinct) ids this
 * shard received, TF layout, and write the wire rows euler_gpu_expand_packed
 * consumes - euler_gpu_pack_rows' format: 4 * count + 2 int32 words per root
 * (ids | weights | types | row mask, pad), 3 * count + 2 (padded to even) without
 * the type column when k == 1.  Single-type calls on
 * graphs the pivot kernels serve write the rows straight from the sampling
 * kernel; every other call samples into scratch arrays and packs. */
int euler_gpu_sample_neighbor_packed(const euler_gpu_graph* g, void* stream,
                                     uint64_t seed, uint32_t call_id,
                                     const uint64_t* roots_dev, int64_t n,
                                     const int32_t* edge_types_host, int32_t k,
                                     int32_t count, int64_t default_node,
                                     int32_t* packed_dev);
/* ... for several edge-type SETS over the same ids in ONE launch (euler_gpu_sample_neighbor_sets'
 * kernel writing wire rows: the typed hops of a heterogeneous minibatch on a sharded graph).
 * Set s draws with call_id + s and its n rows begin sum over s' < s of n * words(s') int32 words into
 * packed_dev, words(s) = 4 * count + 2, or 3 * count + 2 padded to even for a set of ONE type (no
 * type column) - the rows of n_sets euler_gpu_sample_neighbor_packed calls, bit for bit in every
 * word euler_gpu_expand_packed reads.  Graphs the one-launch kernel does not serve take those calls. */
int euler_gpu_sample_neighbor_sets_packed(const euler_gpu_graph* g, void* stream, uint64_t seed,
                                          uint32_t call_id, const uint64_t* roots_dev, int64_t n,
                                          const int32_t* edge_types_host, const int32_t* set_k_host,
                                          int32_t n_sets, int32_t count, int64_t default_node,
                                          int32_t* packed_dev);

/* TF SampleFanout (tf_euler/kernels/sample_fanout_op.cc:32-148): `layers` hops
 * chained on device; hop h uses call_id + h, edge_types_host[h*k .. h*k+k) and
 * counts_host[h].  out_*_dev[h] has n * prod(counts[0..h]) elements.
 * workspace_dev must hold euler_gpu_sample_fanout_workspace() bytes. */
size_t euler_gpu_sample_fanout_workspace(int64_t n, const int32_t* counts_host,
                                         int32_t layers);
/* M minibatches of one SampleFanout in ONE enqueue - the regime of the reference's callers
 * (tf_euler/python/dataflow/sage_dataflow.py:35-50 issues one sample_fanout per minibatch of
 * a few hundred roots; its client keeps 8 such queries in flight, client/query_proxy.cc:
 * 205-210).  roots_dev holds m * n roots, minibatch b = roots [b n, (b + 1) n) draws with
 * call id call_ids_dev[b] (a DEVICE array, 2-hop single-type fanouts only) or, when that is
 * NULL, call_id + b * call_stride (hop h: + h).  out_*_dev[h] has m * n * prod(counts[0..h])
 * elements, minibatch-major.  Draws are keyed by (call id, node id), so the result equals
 * m calls of euler_gpu_sample_fanout bit for bit.  A 2-hop fanout of single listed types
 * is one launch (a workgroup per root below 8 192 roots in all, the wave-per-4-roots kernel
 * of fanout_local.h above); other shapes enqueue the minibatches one after the other.
 * workspace_dev: euler_gpu_sample_fanout_workspace(m * n, ...) bytes. */
int euler_gpu_sample_fanout_multi(const euler_gpu_graph* g, void* stream, uint64_t seed,
                                  uint32_t call_id, uint32_t call_stride,
                                  const uint32_t* call_ids_dev, int32_t m,
                                  const uint64_t* roots_dev, int64_t n,
                                  const int32_t* edge_types_host, int32_t k,
                                  const int32_t* counts_host, int32_t layers,
                                  int64_t default_node, uint64_t* const* out_id_dev,
                                  float* const* out_w_dev, int32_t* const* out_t_dev,
                                  void* workspace_dev);
int euler_gpu_sample_fanout(const euler_gpu_graph* g, void* stream,
                            uint64_t seed, uint32_t call_id,
                            const uint64_t* roots_dev, int64_t n,
                            const int32_t* edge_types_host, int32_t k,
                            const int32_t* counts_host, int32_t layers,
                            int64_t default_node, uint64_t* const* out_id_dev,
                            float* const* out_w_dev, int32_t* const* out_t_dev,
                            void* workspace_dev);

/* ---- SampleNeighbor, alias mode (opt-in) -----------------------------------
 * The calls above invert the row's running sums exactly as the reference does
 * (RandomSelect): that is the default and the only mode that reproduces the reference's
 * neighbours.  The calls below draw from the SAME distribution through one alias table per
 * (row, edge-type group) - AliasMethod (common/alias_method.cc:23-78) over the group's
 * normalised weights (FastWeightedCollection::Init, common/fast_weighted_collection.h:55-75),
 * the structure the reference itself uses for SampleNode: one 32-byte entry read per draw,
 * whatever the degree and the weight distribution.  For the same seed they pick DIFFERENT
 * neighbours than the exact mode; the mode is validated statistically.  One departure from
 * alias_method.cc:52-62: an edge of weight 0 is never drawn (csrc/nb_alias.h).
 *
 * The tables: 32 bytes per edge, counted in euler_gpu_graph_bytes; built by the call below or by
 * the first alias call, on `stream`, under a per-graph lock (concurrent callers wait; the call
 * returns when the build has finished).  Idempotent.  EULER_GPU_EINVAL for a graph with negative
 * or NaN weights; a failed build leaves the graph as it was and returns the HIP error.  Builds
 * none of the exact mode's indexes. */
int euler_gpu_graph_build_neighbor_alias(euler_gpu_graph* g, void* stream);
/* Bytes and entries of the tables; 0 / 0 when they are not built. */
int euler_gpu_graph_neighbor_alias_info(const euler_gpu_graph* g, int64_t* bytes_host,
                                        int64_t* entries_host);
/* The entries of the listed rows in the row order of euler_gpu_graph_export_rows (spot checks):
 * entry x of row i at row_ptr_host[i] + x holds AliasMethod's prob_ (alias_method.cc:43,55,61),
 * the ids of the edge itself and of its alias_ edge, and the weights the exact mode returns for
 * the two.  Call with id_self_host == NULL to obtain row_ptr_host (n + 1) first.
 * EULER_GPU_EINVAL when the tables are not built. */
int euler_gpu_graph_export_neighbor_alias(const euler_gpu_graph* g, const uint64_t* ids_host,
                                          int64_t n, int64_t* row_ptr_host,
                                          uint64_t* id_self_host, uint64_t* id_alias_host,
                                          float* prob_host, float* w_self_host,
                                          float* w_alias_host);
/* euler_gpu_sample_neighbor with the alias draw: the same parameters, row lookup, type modes
 * (Node::__SampleNeighbor, core/graph/node.cc:98-161; the type of a sample is drawn as the exact
 * mode draws it), layouts, fills, first-id-0 rule, root mask and row mask.  The neighbour is
 * AliasMethod::Next (alias_method.cc:66-78): column = floor(d * u), one entry, coin < prob ? the
 * edge : its alias.  Domain 0, stream = the root's node id; sample j uses draw indices 4 j (type,
 * when one is drawn), 4 j + 2 (column), 4 j + 3 (coin).  Duplicate roots get identical rows. */
int euler_gpu_sample_neighbor_alias(const euler_gpu_graph* g, void* stream,
                                    uint64_t seed, uint32_t call_id,
                                    const uint64_t* roots_dev, int64_t n,
                                    const uint8_t* root_mask_dev, int32_t root_group,
                                    const int32_t* edge_types_host, int32_t k,
                                    int32_t count, int32_t layout,
                                    int64_t default_node, uint64_t* out_id_dev,
                                    float* out_w_dev, int32_t* out_t_dev,
                                    uint8_t* out_row_mask_dev);
/* euler_gpu_sample_fanout with the alias draw (AliasMethod::Next per sample, alias_method.cc:
 * 66-78): `layers` launches in one enqueue, hop h with call_id + h on hop h - 1's TF-layout ids;
 * the rows under a default row of hop h - 1 sample as node id 0.  Same parameters and workspace
 * size as the exact calls. */
size_t euler_gpu_sample_fanout_alias_workspace(int64_t n, const int32_t* counts_host,
                                               int32_t layers);
int euler_gpu_sample_fanout_alias(const euler_gpu_graph* g, void* stream,
                                  uint64_t seed, uint32_t call_id,
                                  const uint64_t* roots_dev, int64_t n,
                                  const int32_t* edge_types_host, int32_t k,
                                  const int32_t* counts_host, int32_t layers,
                                  int64_t default_node, uint64_t* const* out_id_dev,
                                  float* const* out_w_dev, int32_t* const* out_t_dev,
                                  void* workspace_dev);

/* ---- SampleNode -----------------------------------------------------------
 * Replaces euler::SampleNode (core/api/api.cc:32-37) -> Graph::SampleNode
 * (core/graph/graph.cc:221-275) -> AliasMethod::Next (common/alias_method.cc:
 * 66-78).  node_types_host[k]: k == 1 && type == -1 samples over all types.
 * Returns EULER_GPU_EEMPTY (and writes nothing) when the weight sum is 0. */
int euler_gpu_sample_node(const euler_gpu_graph* g, void* stream, uint64_t seed,
                          uint32_t call_id, const int32_t* node_types_host,
                          int32_t k, int32_t count, uint64_t* out_dev);

/* API_GET_NODE_T / TF GetNodeType (core/kernels/get_node_type_op.cc:35-62,
 * tf_euler/kernels/get_node_type_op.cc:33-57): the node type of every id;
 * INT32_MIN (euler::common::DEFAULT_INT32) for an unknown node. */
int euler_gpu_get_node_type(const euler_gpu_graph* g, void* stream,
                            const uint64_t* ids_dev, int64_t n, int32_t* out_dev);

/* API_SAMPLE_N_WITH_TYPES / TF SampleNWithTypes (core/kernels/
 * sample_n_with_types_op.cc:33-75, tf_euler/kernels/sample_n_with_types_op.cc:
 * 38-84; euler_ops sample_node_with_src): row i of out_dev [n, count] = one
 * Graph::SampleNode(types_dev[i], count) call (type -1 = all types).  RNG:
 * domain 1, stream = i.  A type that is out of range or has zero weight makes
 * the reference's TF kernel abort ("samples size error, invalid node types!");
 * here the call returns EULER_GPU_EEMPTY.  Synchronises the stream. */
int euler_gpu_sample_n_with_types(const euler_gpu_graph* g, void* stream, uint64_t seed,
                                  uint32_t call_id, const int32_t* types_dev, int64_t n,
                                  int32_t count, uint64_t* out_dev);

/* ---- full neighbours ------------------------------------------------------
 * euler::GetFullNeighbor (core/api/api.cc:208-221) -> Node::GetFullNeighbor
 * (core/graph/node.cc:175-197) in the FillNeighbor layout.  Two calls: first
 * with out_id_dev == NULL fills idx_dev [n,2] (int32 offsets) and *total_host
 * (synchronises the stream); the second call writes the values (out_t_dev may be
 * NULL: the edge types are not written - the sharded node2vec walk does not read them).
 * A call that lists 2^31 entries or more does not fit the int32 offsets: the first call
 * returns EULER_GPU_EINVAL, leaves *total_host alone, and idx_dev is not to be used. */
int euler_gpu_get_full_neighbor(const euler_gpu_graph* g, void* stream,
                                const uint64_t* ids_dev, int64_t n,
                                const int32_t* edge_types_host, int32_t k,
                                int32_t* idx_dev, int64_t* total_host,
                                uint64_t* out_id_dev, float* out_w_dev,
                                int32_t* out_t_dev);

/* Post-process of API_GET_NB_NODE (core/kernels/get_neighbor_op.cc:117-168) on
 * the result of euler_gpu_get_full_neighbor, in place: order_by (0 none, 1 id,
 * 2 weight; desc != 0 = descending) then limit (< 0 = none).  Rows are
 * re-packed, idx_dev rewritten, *total_host receives the new total (stream
 * sync).  This is what the TF ops GetSortedFullNeighbor (`order_by(id, asc)`,
 * tf_euler/kernels/get_sorted_full_neighbor_op.cc:43-46) and GetTopKNeighbor
 * (`order_by(weight, desc).limit(k)`, get_top_k_neighbor_op.cc:36-44) run.
 * Equal keys keep storage order (undefined in the reference: std::sort with a
 * non-strict comparator). */
int euler_gpu_neighbor_post_process(void* stream, int64_t n, int32_t* idx_dev,
                                    int64_t total, uint64_t* id_dev, float* w_dev,
                                    int32_t* t_dev, int32_t order_by, int32_t desc,
                                    int64_t limit, int64_t* total_host);
/* tf_euler get_top_k_neighbor (tf_euler/kernels/get_top_k_neighbor_op.cc: GQL
 * `v(nodes).outV(edge_types).order_by(weight, desc).limit(k)`, dense fill) in
 * one kernel: out_*_dev [n, k] = the k heaviest neighbours of every node over
 * the listed edge types (ties keep the order of Node::GetFullNeighbor,
 * core/graph/node.cc:175-197), default_node / 0.0 / -1 where a node has fewer.
 * Same result as euler_gpu_get_full_neighbor + euler_gpu_neighbor_post_process
 * (weight, descending, limit k) + euler_gpu_neighbor_to_dense. */
int euler_gpu_get_top_k_neighbor(const euler_gpu_graph* g, void* stream,
                                 const uint64_t* ids_dev, int64_t n,
                                 const int32_t* edge_types_host, int32_t k_types,
                                 int32_t k, int64_t default_node, uint64_t* out_id_dev,
                                 float* out_w_dev, int32_t* out_t_dev);

/* Dense [n, k] fill of the TF GetTopKNeighbor kernel
 * (tf_euler/kernels/get_top_k_neighbor_op.cc:70-75,101-109): default_node /
 * 0.0 / -1 where a row has fewer than k entries. */
int euler_gpu_neighbor_to_dense(void* stream, int64_t n, const int32_t* idx_dev,
                                const uint64_t* id_dev, const float* w_dev,
                                const int32_t* t_dev, int32_t k, int64_t default_node,
                                int64_t* out_id_dev, float* out_w_dev,
                                int32_t* out_t_dev);

/* ---- layerwise sampling (GQL sampleLNB without a weight function) -----------
 * The DAG euler/parser/translator.cc:338-386,489-527 builds for
 * `v(nodes).sampleLNB(edge_types, n, m, default_node)`:
 * API_GET_EDGE_SUM_WEIGHT -> API_SAMPLE_ROOT -> API_SAMPLE_L ->
 * API_SPARSE_GEN_ADJ -> API_SPARSE_GET_ADJ -> API_GATHER_RESULT.
 * With a weight function the first three are API_GET_NB_NODE ->
 * API_LOCAL_SAMPLE_L (euler_gpu_local_sample_layer below). */

/* API_GET_EDGE_SUM_WEIGHT (core/kernels/get_edge_sum_weight_op.cc:33-66):
 * out_w_dev[i] = f32 sum, in Node::GetFullNeighbor order (core/graph/node.cc:
 * 175-197), of the weights of ids_dev[i]'s out-edges of the listed types; 0 for
 * an unknown node. */
int euler_gpu_get_edge_sum_weight(const euler_gpu_graph* g, void* stream,
                                  const uint64_t* ids_dev, int64_t n,
                                  const int32_t* edge_types_host, int32_t k,
                                  float* out_w_dev);

/* API_SAMPLE_ROOT (core/kernels/sample_root_op.cc:33-88): for every batch row b,
 * a FastWeightedCollection (common/fast_weighted_collection.h:55-75 over
 * AliasMethod::Init, common/alias_method.cc:23-63) of roots_dev[b*n .. b*n+n)
 * with weights_dev[b*n ..]; m draws per row -> out_dev [batch * m]; rows whose
 * f32 weight sum is 0 give default_node.  RNG: domain 4, stream = b, draws 2j
 * (column) and 2j+1 (coin) for draw j. */
int euler_gpu_sample_root(void* stream, uint64_t seed, uint32_t call_id,
                          const uint64_t* roots_dev, const float* weights_dev,
                          int64_t batch, int32_t n, int32_t m, int64_t default_node,
                          uint64_t* out_dev);

/* API_SAMPLE_L (core/kernels/sample_layer_op.cc:32-72): position i receives ONE
 * neighbour of roots_dev[i] (euler::SampleNeighbor({root}, edge_types, 1)) or
 * (default_node, 0.0, 0) when that yields nothing.  RNG: domain 5, stream = the
 * position i (a root listed twice is sampled twice, as in the reference).
 * out_w_dev / out_t_dev may be NULL. */
int euler_gpu_sample_layer(const euler_gpu_graph* g, void* stream, uint64_t seed,
                           uint32_t call_id, const uint64_t* roots_dev, int64_t n,
                           const int32_t* edge_types_host, int32_t k,
                           int64_t default_node, uint64_t* out_id_dev,
                           float* out_w_dev, int32_t* out_t_dev);

/* The same draw with explicit RNG streams: root i samples as position
 * pos_dev[i].  A shard of a multi-GPU hop answers the requester's positions, so
 * the sharded result equals the single-GPU one. */
int euler_gpu_sample_layer_at(const euler_gpu_graph* g, void* stream, uint64_t seed,
                              uint32_t call_id, const uint64_t* roots_dev,
                              const int64_t* pos_dev, int64_t n,
                              const int32_t* edge_types_host, int32_t k,
                              int64_t default_node, uint64_t* out_id_dev,
                              float* out_w_dev, int32_t* out_t_dev);

/* The three ops above chained on the stream = output 0 of the TF kernel
 * SampleNeighborLayerwiseWithAdj (tf_euler/kernels/
 * sample_neighbor_layerwise_with_adj_op.cc:56-150, weight_func == ""):
 * nodes_dev [batch, n] -> out_dev [batch, count].  Its sparse adjacency outputs
 * are euler_gpu_sparse_get_adj_tf(nodes_dev, out_dev, batch, n, count, ...). */
int euler_gpu_sample_neighbor_layerwise(const euler_gpu_graph* g, void* stream,
                                        uint64_t seed, uint32_t call_id,
                                        const uint64_t* nodes_dev, int64_t batch,
                                        int32_t n, const int32_t* edge_types_host,
                                        int32_t k, int32_t count,
                                        int64_t default_node, uint64_t* out_dev);

/* API_LOCAL_SAMPLE_L (core/kernels/local_sample_layer_op.cc:43-146), the
 * sampler of `sampleLNB(edge_types, n, m, weight_func, default_node)`: per batch
 * row the distinct (neighbour id, edge type) pairs among the full neighbours of
 * its n nodes (idx_dev [batch*n, 2] / ids_dev / w_dev / t_dev [total]: the
 * API_GET_NB_NODE result, e.g. euler_gpu_get_full_neighbor), weights of
 * duplicates added, then `sqrt` when weight_func is "sqrt" (any other string
 * leaves them as they are, :86-95), then m draws by CDF inversion -> out_*_dev
 * [batch * m].  The candidate ORDER is the iteration order of the op's
 * std::unordered_map<std::string, ...>; the tables are therefore built on the
 * host with that very container (a stream sync each way), the draws run on the
 * device.  Rows with no candidates or zero weight are memset like the op does:
 * every BYTE of the ids = default_node's low byte.  RNG: domain 6, stream = b. */
int euler_gpu_local_sample_layer(void* stream, uint64_t seed, uint32_t call_id,
                                 const int32_t* idx_dev, const uint64_t* ids_dev,
                                 const float* w_dev, const int32_t* t_dev, int64_t total,
                                 int64_t batch, int32_t n, int32_t m,
                                 const char* weight_func, int64_t default_node,
                                 uint64_t* out_id_dev, float* out_w_dev,
                                 int32_t* out_t_dev);

/* API_SPARSE_GET_ADJ (core/kernels/sparse_get_adj_op.cc:35-92) with the
 * root_batch tensor API_SPARSE_GEN_ADJ builds (sparse_gen_adj_op.cc:52-61:
 * root r belongs to batch row r / n): for every root the candidates
 * l_nb_dev[b*m .. b*m+m) it has an edge of a listed type to, in candidate
 * order.  FillNeighbor-style result: idx_dev [batch*n, 2] int32 offsets +
 * out_id_dev [total].  Two calls like euler_gpu_get_full_neighbor: with
 * out_id_dev == NULL it answers the query (one bit per (root, candidate) kept
 * in workspace_dev), fills idx_dev and *total_host (stream sync); the second
 * call writes the ids from the workspace.  workspace_dev:
 * euler_gpu_sparse_get_adj_workspace(batch, n, m) bytes, 8-byte aligned, kept
 * by the caller between the two calls.  EdgeExist (core/api/api.cc:46-48) is
 * answered from the adjacency rows: the Edge records the reference would
 * consult hold the same (src, dst, type) triples in data written by its
 * converter. */
size_t euler_gpu_sparse_get_adj_workspace(int64_t batch, int32_t n, int32_t m);
int euler_gpu_sparse_get_adj(const euler_gpu_graph* g, void* stream,
                             const uint64_t* roots_dev, const uint64_t* l_nb_dev,
                             int64_t batch, int32_t n, int32_t m,
                             const int32_t* edge_types_host, int32_t k,
                             void* workspace_dev, int32_t* idx_dev,
                             int64_t* total_host, uint64_t* out_id_dev);

/* TF SparseGetAdj (tf_euler/kernels/sparse_get_adj_op.cc:43-134) and the
 * adjacency outputs of SampleNeighborLayerwiseWithAdj: COO triples (b, j, c) in
 * row-major order with value 1 where nodes[b, j] has a listed-type edge to
 * nb_nodes[b, c], plus the kernel's explicit 0 at (b, n-1, m-1) when that pair
 * is no edge (so dense_shape = [batch, n, m]).  Two calls over the same
 * workspace (see above): indices_dev == NULL answers the query and returns
 * *nnz_host (stream sync); then indices_dev [nnz, 3] / values_dev [nnz] int64. */
int euler_gpu_sparse_get_adj_tf(const euler_gpu_graph* g, void* stream,
                                const uint64_t* nodes_dev, const uint64_t* nb_nodes_dev,
                                int64_t batch, int32_t n, int32_t m,
                                const int32_t* edge_types_host, int32_t k,
                                void* workspace_dev, int64_t* nnz_host,
                                int64_t* indices_dev, int64_t* values_dev);

/* SparseGetAdj on a SHARDED graph, owner side and requester side.  Every shard computes the
 * hit mask of the sources it owns - mask_dev [batch * n][(m + 63) / 64] uint64, bit c of a
 * source = candidate c of its batch row is in the source's row; sources without a row on
 * this shard give zeros - and the masks of all shards OR to the mask of the whole graph.  The
 * requester turns the combined mask into the TF triple (two calls as
 * euler_gpu_sparse_get_adj_tf; workspace 8 * (batch * n + 1) bytes).  Replaces shipping the
 * sources' whole rows (core/kernels/sparse_get_adj_op.cc:35-92 is the per-shard op). */
int euler_gpu_sparse_adj_mask(const euler_gpu_graph* g, void* stream, const uint64_t* nodes_dev,
                              const uint64_t* nb_nodes_dev, int64_t batch, int32_t n, int32_t m,
                              const int32_t* edge_types_host, int32_t k, uint64_t* mask_dev);
int euler_gpu_sparse_adj_from_mask_tf(void* stream, const uint64_t* mask_dev, int64_t batch,
                                      int32_t n, int32_t m, void* workspace_dev,
                                      int64_t* nnz_host, int64_t* indices_dev,
                                      int64_t* values_dev);

/* ---- dense features --------------------------------------------------------
 * TF GetDenseFeature (tf_euler/kernels/get_dense_feature_op.cc:63-125) over
 * Node::GetFloat32Feature (core/graph/node.cc:330-394): out_dev is [n, dim]
 * float32, zero filled; row j receives the stored values of feature slot `fid`
 * of node nodes_dev[j] (unknown node / slot: zeros).  A node that stores more
 * than `dim` values would overrun the reference's output row; here the row is
 * truncated to dim. */
int32_t euler_gpu_graph_num_float_features(const euler_gpu_graph* g);
int euler_gpu_get_dense_feature(const euler_gpu_graph* g, void* stream,
                                const uint64_t* nodes_dev, int64_t n, int32_t fid,
                                int32_t dim, float* out_dev);

/* The dense feature table in 16 bits.  euler_gpu_graph_set_dense_feature_dtype converts the
 * value array on the device, element by element (round to nearest even; every offset is in
 * elements and stays), frees the fp32 array and lowers euler_gpu_graph_bytes by the half it
 * saves.  The same dtype again is a no-op; a 16-bit table cannot go back to fp32 or to the
 * other 16-bit type (the bits are gone): EULER_GPU_EINVAL, as for an unknown dtype, a graph
 * without dense features and a shard of a sharded graph (shards > 1: the sharded feature
 * exchange moves fp32 rows).  It waits for the device: no other call may run on the graph
 * meanwhile.  Afterwards euler_gpu_get_dense_feature and euler_gpu_sample_fanout_with_feature
 * return fp32 rows of the rounded values.
 * euler_gpu_get_dense_feature_t writes rows of out_dtype: fp32, or the table's dtype (the stored
 * bits); an fp32 table serves all three (values rounded once at the store).  Anything else:
 * EULER_GPU_EINVAL. */
int euler_gpu_graph_set_dense_feature_dtype(euler_gpu_graph* g, void* stream, int32_t dtype);
int32_t euler_gpu_graph_dense_feature_dtype(const euler_gpu_graph* g);
int euler_gpu_get_dense_feature_t(const euler_gpu_graph* g, void* stream,
                                  const uint64_t* nodes_dev, int64_t n, int32_t fid,
                                  int32_t dim, void* out_dev, int32_t out_dtype);

/* ---- sparse (uint64) features ----------------------------------------------
 * TF GetSparseFeature (tf_euler/kernels/get_sparse_feature_op.cc:52-131) over
 * Node::GetUint64Feature (core/graph/node.cc:330-372), one feature slot per
 * call: the COO triple of the [n, max_len] SparseTensor - for node j the
 * entries (j, 0..len-1) = its stored values, or ONE entry (j, 0) =
 * default_value when it stores none (unknown node / slot included).
 * Two calls: with indices_dev == NULL it fills row_off_dev [n + 1] (int64
 * scratch the second call reads), *nnz_host and *max_len_host (dense_shape =
 * [n, max_len]; stream sync); then indices_dev [nnz, 2] / values_dev [nnz]. */
int32_t euler_gpu_graph_num_u64_features(const euler_gpu_graph* g);
int euler_gpu_get_sparse_feature(const euler_gpu_graph* g, void* stream,
                                 const uint64_t* nodes_dev, int64_t n, int32_t fid,
                                 int64_t default_value, int64_t* row_off_dev,
                                 int64_t* nnz_host, int64_t* max_len_host,
                                 int64_t* indices_dev, int64_t* values_dev);

/* The same feature slot in the GQL `values(...)` layout of API_GET_P
 * (core/kernels/get_feature_op.cc:34-70): idx_dev [n, 2] int32 offsets + the
 * packed values, no default entries - what a shard returns to the requester in
 * the multi-GPU path.  Two calls like euler_gpu_get_full_neighbor. */
int euler_gpu_get_sparse_feature_core(const euler_gpu_graph* g, void* stream,
                                      const uint64_t* nodes_dev, int64_t n, int32_t fid,
                                      int32_t* idx_dev, int64_t* total_host,
                                      uint64_t* values_dev);

/* The lookup ShallowEncoder makes of a sparse feature (tf_euler/python/utils/encoders.py:146-170:
 * get_sparse_feature, then tf.nn.embedding_lookup_sparse(table, sp, None, combiner)) in one
 * kernel: out_dev [n, dim] = the combined rows of table_dev [n_rows, dim] named by the values of
 * uint64 slot `fid` of each node.  No SparseTensor is written; the call only enqueues (no
 * allocation, no host wait: safe under stream capture).
 * Entry list of a node: its stored values; a node without any (unknown node, empty slot, fid
 * outside the table) has the one entry default_value when has_default != 0, else none.
 * An entry >= n_rows (compared UNSIGNED, so values at or above 2^63 too) names no row: it is left
 * out of the sum and of the count (the default value obeys the rule as well).
 * The counted rows are widened exactly to fp32 and added in stored order, one fp32 add per entry
 * starting from the first row; combiner 0 sum, 1 mean = sum / (float)cnt, 2 sqrtn =
 * sum / sqrtf((float)cnt) (IEEE fp32; what embedding_lookup_sparse with sp_weights = None divides
 * by); cnt == 0 gives a zero row.  counts_dev [n] (or NULL) receives cnt.
 * table_dtype: EULER_GPU_F32 / _BF16 / _F16; out_dtype: EULER_GPU_F32 or table_dtype (rounded once
 * at the store).  16-byte-aligned table and output with dim a multiple of 4 (fp32) / 8 (16-bit)
 * take 16-byte lanes, everything else one element per lane.
 * EULER_GPU_ENOGRAPH: null graph.  EULER_GPU_EINVAL: n < 0, dim < 1, n_rows < 1 or >= 2^31, an
 * unknown dtype or combiner, out_dtype neither fp32 nor table_dtype, a null buffer with n > 0.
 * n == 0 returns EULER_GPU_OK and touches nothing. */
int euler_gpu_sparse_feature_embedding(const euler_gpu_graph* g, void* stream,
                                       const uint64_t* nodes_dev, int64_t n, int32_t fid,
                                       int32_t has_default, int64_t default_value,
                                       const void* table_dev, int32_t table_dtype, int64_t n_rows,
                                       int32_t dim, int32_t combiner /* 0 sum, 1 mean, 2 sqrtn */,
                                       void* out_dev, int32_t out_dtype, int32_t* counts_dev);

/* ---- block construction (SageDataFlow) on the device ---------------------------
 * tf_euler/python/dataflow/sage_dataflow.py:35-50 + neighbor_dataflow.py:84-110
 * (UniqueDataFlow.produce_subgraph) for `layers` hops, enqueued on `stream` with NO
 * host round trip in between: hop h samples fanouts_host[h] neighbours
 * (edge_types_host[h*k .. h*k+k), call id call_id + h, default_node) of the layer's
 * nodes, takes the first-occurrence unique (tf.unique) of [neighbours | nodes] as
 * the next layer and emits the block.  Arrays are sized for the worst case
 * cap_0 = n, cap_{h+1} = cap_h * (fanouts[h] + 1); the true sizes are
 * counts_dev [layers + 1] (uint32: counts[0] = n, counts[h+1] = nodes of layer
 * h + 1), which the host may read after the call or never.  Block h:
 *   n_id_dev[h]      [cap_{h+1}]                 new_n_id (valid: counts[h+1])
 *   res_n_id_dev[h]  [cap_h]                     index of every node of layer h in
 *                                                new_n_id (valid: counts[h])
 *   edge_src_dev[h], edge_dst_dev[h]  [cap_h * (fanouts[h] + 1)]   edge_index rows;
 *                    valid: counts[h] * fanouts[h] (+ counts[h] self loops when
 *                    add_self_loops != 0)
 * workspace_dev: euler_gpu_sage_blocks_workspace(n, fanouts_host, layers) bytes. */
size_t euler_gpu_sage_blocks_workspace(int64_t n, const int32_t* fanouts_host, int32_t layers);
int euler_gpu_sage_blocks(const euler_gpu_graph* g, void* stream, uint64_t seed,
                          uint32_t call_id, const uint64_t* roots_dev, int64_t n,
                          const int32_t* edge_types_host, int32_t k,
                          const int32_t* fanouts_host, int32_t layers, int64_t default_node,
                          int32_t add_self_loops, void* workspace_dev,
                          uint64_t* const* n_id_dev, int64_t* const* res_n_id_dev,
                          int64_t* const* edge_src_dev, int64_t* const* edge_dst_dev,
                          uint32_t* counts_dev);

/* n_mb minibatches of n roots each as ONE enqueue - what n_mb consecutive euler_gpu_sage_blocks
 * calls produce, bit for bit: the reference's GraphSAGE callers build a flow per minibatch of a
 * few hundred roots (sage_dataflow.py:35-50; examples/graphsage/run_graphsage.py:35 defaults to
 * 32), which neither fills a GPU nor amortises the dozen launches of a flow.  roots_dev
 * [n_mb * n], minibatch-major; minibatch b draws hop h with call_id + b * call_stride + h (what
 * consecutive calls take from a counter with call_stride = layers).  Every output is n_mb copies
 * of the single call's array, each sized for the worst case and b * cap apart: n_id_dev[h]
 * [n_mb][cap_{h+1}], res_n_id_dev[h] [n_mb][cap_h], edge_src_dev[h] / edge_dst_dev[h]
 * [n_mb][cap_{h+1}], counts_dev [n_mb][layers + 1].  Hops that list ONE edge type on a graph
 * without the id-0 sentinel rule run as one launch per kernel of the flow (a minibatch per
 * blockIdx.y); other shapes are served by the separate calls, one after the other.
 * workspace_dev: euler_gpu_sage_blocks_multi_workspace(n_mb, n, fanouts_host, layers) bytes. */
size_t euler_gpu_sage_blocks_multi_workspace(int32_t n_mb, int64_t n, const int32_t* fanouts_host,
                                             int32_t layers);
int euler_gpu_sage_blocks_multi(const euler_gpu_graph* g, void* stream, uint64_t seed,
                                uint32_t call_id, uint32_t call_stride, int32_t n_mb,
                                const uint64_t* roots_dev, int64_t n,
                                const int32_t* edge_types_host, int32_t k,
                                const int32_t* fanouts_host, int32_t layers, int64_t default_node,
                                int32_t add_self_loops, void* workspace_dev,
                                uint64_t* const* n_id_dev, int64_t* const* res_n_id_dev,
                                int64_t* const* edge_src_dev, int64_t* const* edge_dst_dev,
                                uint32_t* counts_dev);

/* The full-neighbour dataflows (tf_euler/python/dataflow/gcn_dataflow.py:33-47 GCNDataFlow,
 * relation_dataflow.py:30-72 RelationDataFlow: every hop takes ALL neighbours of the listed
 * edge types of the nodes seen so far, then tf.unique of [neighbours | nodes], res_n_id and
 * edge_index) enqueued without a host round trip between the hops.  Row lengths are
 * data: the caller gives the capacity of every hop's edge list, edge_caps_host[h]; layer
 * h + 1 then holds at most cap_n[h] + edge_caps[h] nodes (cap_n[0] = n).  A hop whose rows
 * do not fit sets the overflow word and contributes no edges - the host sees it in its one
 * read of counts_dev and repeats the flow with larger capacities (or op by op).
 *   n_id_dev[h]      [cap_n[h + 1]]              nodes of layer h + 1 (first-occurrence order)
 *   res_n_id_dev[h]  [cap_n[h]]                  index of layer h's nodes in layer h + 1
 *   edge_src_dev[h], edge_dst_dev[h]  [edge_caps[h] + cap_n[h]]   edges, then (add_self_loops) one
 *                                                self loop per node of layer h
 *   e_type_dev[h]    [edge_caps[h]] or e_type_dev == NULL   the edge type of every edge (RGCN's e_id)
 *   counts_dev       uint32 [2 * layers + 2]: nodes per layer [layers + 1], edges per hop
 *                    [layers] (self loops not counted), overflow [1] */
size_t euler_gpu_full_blocks_workspace(int64_t n, const int64_t* edge_caps_host, int32_t layers);
int euler_gpu_full_blocks(const euler_gpu_graph* g, void* stream, const uint64_t* roots_dev,
                          int64_t n, const int32_t* edge_types_host, int32_t k, int32_t layers,
                          int32_t add_self_loops, const int64_t* edge_caps_host,
                          void* workspace_dev, uint64_t* const* n_id_dev,
                          int64_t* const* res_n_id_dev, int64_t* const* edge_src_dev,
                          int64_t* const* edge_dst_dev, int32_t* const* e_type_dev,
                          uint32_t* counts_dev);

/* ---- RandomWalk -------------------------------------------------------------
 * TF RandomWalk kernel (tf_euler/kernels/random_walk_op.cc:172-291):
 * |p-1|,|q-1| <= 1e-6 -> chain of count=1 SampleNeighbor hops (:207-247), else
 * node2vec with BuildWeights (:83-168).  edge_types_host is [walk_len, k];
 * out_dev is [n, walk_len+1] int64. */
int euler_gpu_random_walk(const euler_gpu_graph* g, void* stream, uint64_t seed,
                          uint32_t call_id, const int64_t* nodes_dev, int64_t n,
                          const int32_t* edge_types_host, int32_t k,
                          int32_t walk_len, float p, float q,
                          int64_t default_node, int64_t* out_dev);

/* One node2vec step over explicit neighbour lists, as the reference's client runs it
 * (tf_euler/kernels/random_walk_op.cc:83-168: RWCallback::operator(), BuildWeights,
 * CompactWeightedCollection::Sample) on the lists the `v(nodes).outV(edge_types)` query
 * returned - no graph: on a sharded graph the requester calls this on fetched rows.
 * Walker i's child list is row c_row[i] of the packed rows (c_idx [rows, 2] int32 offsets,
 * c_ids, c_w - c_entries ids / weights in all), its parent's list row p_row[i] of (p_idx,
 * p_ids) (p_row NULL on the first
 * step: no parent lists yet), parent_ids[i] its previous node (the start node on the first
 * step).  out[i] = the next node, default_node for an empty child list.  RNG: domain WALK,
 * stream = walker index i, draw 0 of call_id (the single-GPU random_walk uses call_id +
 * step).  One wave per walker runs the single-GPU walk's two-cursor merge with integer
 * running sums (csrc/n2v_kernels.h) over the fetched rows; tuning key 7 = 0 selects the
 * lane-per-walker reference loop. */
int euler_gpu_node2vec_step(void* stream, uint64_t seed, uint32_t call_id, int64_t n,
                            const int32_t* c_row_dev, const int32_t* c_idx_dev,
                            const uint64_t* c_ids_dev, const float* c_w_dev, int64_t c_entries,
                            const int32_t* p_row_dev, const int32_t* p_idx_dev,
                            const uint64_t* p_ids_dev, const int64_t* parent_ids_dev,
                            float p, float q, int64_t default_node, int64_t* out_dev);

/* GenPair (tf_euler/kernels/gen_pair_op.cc:42-95): paths [batch,path_len] ->
 * pairs [batch, pair_count, 2]. */
int64_t euler_gpu_gen_pair_count(int64_t path_len, int32_t left_win,
                                 int32_t right_win);
int euler_gpu_gen_pair(void* stream, const int64_t* paths_dev, int64_t batch,
                       int64_t path_len, int32_t left_win, int32_t right_win,
                       int64_t* out_dev);

/* ---- ID_UNIQUE / IDX_GATHER / DATA_GATHER ----------------------------------
 * core/kernels/id_unique_op.cc:35-64 (first-occurrence order),
 * idx_gather_op.cc:33-55, data_gather_op.cc:33-80.
 * euler_gpu_id_unique synchronises the stream to return *n_unique_host, euler_gpu_idx_gather
 * to return *total_host; gathered segments of 2^31 entries or more in all do not fit the int32
 * offsets: EULER_GPU_EINVAL, *total_host left alone, out_idx_dev not to be used. */
int euler_gpu_id_unique(void* stream, const uint64_t* ids_dev, int64_t n,
                        uint64_t* unique_dev, int32_t* gather_idx_dev,
                        int64_t* n_unique_host);
int euler_gpu_idx_gather(void* stream, const int32_t* idx_dev,
                         const int32_t* gather_idx_dev, int64_t n,
                         int32_t* out_idx_dev, int64_t* total_host);
int euler_gpu_data_gather(void* stream, const void* data_dev, int32_t elem_size,
                          const int32_t* idx_dev, const int32_t* gather_idx_dev,
                          const int32_t* out_idx_dev, int64_t n, void* out_dev);

/* ---- message passing -----------------------------------------------------
 * MPScatterAdd / MPScatterMax / MPGather (tf_euler/kernels/scatter_op.cc:27-105,
 * gather_op.cc:26-59).  fp32 data, int32 indices.  Scatter results are
 * order-faithful: each output element adds its updates in input order, so
 * they are bit-identical to the reference's sequential loop.
 * An update whose scatter index is < 0 or >= size belongs to no destination (undefined behaviour
 * in the reference): every entry with a key column - scatter_add / _max / _mean, gather_scatter and
 * their _w and _t forms - leaves it out, an empty destination is 0 (add, mean) or -1e9 (max), and
 * the gradients the Python layer builds from these entries give such an update exactly 0 (output
 * and gradient, as euler_gpu_edge_softmax below) without reading grad, out or a count by its key.
 * euler_gpu_gather trusts its indices. */
int euler_gpu_scatter_add(void* stream, const float* updates_dev,
                          const int32_t* indices_dev, int64_t e, int64_t d,
                          int32_t size, float* out_dev);
int euler_gpu_scatter_max(void* stream, const float* updates_dev,
                          const int32_t* indices_dev, int64_t e, int64_t d,
                          int32_t size, float* out_dev);
/* scatter_mean of euler_ops/mp_ops.py:65-69 - scatter_add(x) / (scatter_add(ones) +
 * 1e-7) - in ONE pass over the segments (a destination's count is its segment
 * length); same bits as the composition.  e < 2^24. */
int euler_gpu_scatter_mean(void* stream, const float* updates_dev,
                           const int32_t* indices_dev, int64_t e, int64_t d,
                           int32_t size, float* out_dev);
/* scatter_{add,max,mean}(gather(params, gather_indices), scatter_indices, size) of a
 * message-passing step (tf_euler/python/convolution: x_j = gather(x, edge_index[1]);
 * scatter_(aggr, x_j, edge_index[0])) in ONE pass: a destination's updates are read
 * straight from the rows of `params` they name, in input order - the bits of the
 * composition, without writing and re-reading the e x d block of gathered rows (a third
 * of the composition's HBM traffic).  mode: 0 add, 1 max, 2 mean.  Indices are int32,
 * gather indices must be valid rows of params. */
int euler_gpu_gather_scatter(void* stream, int32_t mode, const float* params_dev,
                             const int32_t* gather_indices_dev,
                             const int32_t* scatter_indices_dev, int64_t e, int64_t d,
                             int32_t size, float* out_dev);
/* The same reduction when the caller knows the segments (a sampled block: `count`
 * neighbours per destination, or CSR offsets): out[r] = reduce over p in
 * [seg_ptr[r], seg_ptr[r+1]) - or [r * count, (r+1) * count) when seg_ptr_dev is NULL -
 * of params[gather_indices[p]] (gather_indices_dev NULL: of params[p]), in that order.
 * No sortedness check of a key column, no host wait.  mean divides by (length + 1e-7)
 * as scatter_mean does. */
int euler_gpu_gather_segment_reduce(void* stream, int32_t mode, const float* params_dev,
                                    const int32_t* gather_indices_dev,
                                    const int64_t* seg_ptr_dev, int64_t count, int64_t d,
                                    int32_t size, float* out_dev);
/* ... with the gather indices given as the int64 ids a sampler returned (SampleNeighbor's
 * output feeding the aggregation of a block): index p is the low 32 bits of
 * gather_ids_dev[p] - the int32 MPGather would receive after a cast
 * (tf_euler/kernels/gather_op.cc:26-59 takes int32 indices) - read in place, without the
 * cast's pass over the ids.  params_rows = the rows of params_dev (< 2^31): an id at or past
 * it - a neighbour that is not a node of this graph - reads the LAST row, never memory outside
 * the table (0 = the caller vouches for the ids). */
int euler_gpu_gather_segment_reduce_ids(void* stream, int32_t mode, const float* params_dev,
                                        int64_t params_rows, const int64_t* gather_ids_dev,
                                        const int64_t* seg_ptr_dev, int64_t count, int64_t d,
                                        int32_t size, float* out_dev);
int euler_gpu_gather(void* stream, const float* params_dev,
                     const int32_t* indices_dev, int64_t e, int64_t d,
                     int64_t n_params, float* out_dev);

/* ---- message passing over 16-bit storage ---------------------------------------
 * The entries above with the storage type of the data as an argument: EULER_GPU_F32 (what the
 * untyped entries take; a typed call with it forwards to them), EULER_GPU_BF16 or
 * EULER_GPU_F16 (IEEE half).  out_dtype is EULER_GPU_F32 or in_dtype.  For 16-bit input x the
 * result has the bits of the fp32 entry on the widened x (widening is exact: the same fp32
 * adds in input order, max over the widened values, mean = sum / (length + 1e-7f), -1e9 for
 * an empty max row), stored as fp32 unchanged or rounded once, to nearest even, to in_dtype.
 * Nothing is summed in 16 bits.  16-bit buffers must be 2-byte aligned; 16-byte aligned
 * ones with d % 8 == 0, d <= 512, d / 8 a divisor of 64 take the 16-byte-lane kernels.
 * Unknown dtype, or out_dtype neither fp32 nor in_dtype: EULER_GPU_EINVAL.
 * euler_gpu_scatter_t: mode 0 add, 1 max, 2 mean (e < 2^24). */
enum { EULER_GPU_F32 = 0, EULER_GPU_BF16 = 1, EULER_GPU_F16 = 2 };
int euler_gpu_gather_t(void* stream, const void* params_dev, int32_t in_dtype,
                       const int32_t* indices_dev, int64_t e, int64_t d, int64_t n_params,
                       void* out_dev, int32_t out_dtype);
int euler_gpu_scatter_t(void* stream, int32_t mode, const void* updates_dev, int32_t in_dtype,
                        const int32_t* indices_dev, int64_t e, int64_t d, int32_t size,
                        void* out_dev, int32_t out_dtype);
int euler_gpu_gather_scatter_t(void* stream, int32_t mode, const void* params_dev, int32_t in_dtype,
                               const int32_t* gather_indices_dev,
                               const int32_t* scatter_indices_dev, int64_t e, int64_t d,
                               int32_t size, void* out_dev, int32_t out_dtype);
int euler_gpu_gather_segment_reduce_t(void* stream, int32_t mode, const void* params_dev,
                                      int32_t in_dtype, const int32_t* gather_indices_dev,
                                      const int64_t* seg_ptr_dev, int64_t count, int64_t d,
                                      int32_t size, void* out_dev, int32_t out_dtype);
int euler_gpu_gather_segment_reduce_ids_t(void* stream, int32_t mode, const void* params_dev,
                                          int32_t in_dtype, int64_t params_rows,
                                          const int64_t* gather_ids_dev,
                                          const int64_t* seg_ptr_dev, int64_t count, int64_t d,
                                          int32_t size, void* out_dev, int32_t out_dtype);

/* ---- edge-weighted message passing -----------------------------------------------
 * The fused reduces above with a per-edge multiplier folded in: update p contributes
 * fl(params[g(p)][c] * w[p][c / dh]), dh = d / heads - the message of GCN and APPNP
 * (tf_euler/python/convolution/gcn_conv.py:50-51, appnp_conv.py:54-55: norm_i * norm_j * x_j;
 * heads = 1) and of GAT and AGNN (gat_conv.py:71, agnn_conv.py:54: x_j * alpha, one alpha per
 * head), or a sampled neighbour's weight (sample_neighbor returns them next to the ids).
 * w_dev is [e, heads], indexed by the update's position in the INPUT.  The product and the add
 * are two correctly rounded fp32 operations, in input order: the bits of
 * scatter_(op, gather(params, g) * w, dst, size) with the multiply done elementwise in fp32,
 * without any [e, d] intermediate.  mean divides by (segment length + 1e-7f); the weights do not
 * enter the denominator.  Arguments as the unweighted sibling, then w_dev and heads (and, for the
 * _t forms, w_dtype: EULER_GPU_F32 or in_dtype - widened exactly, products and sums in fp32, one
 * rounding at the store).  gather_indices_dev of euler_gpu_gather_scatter_w may be NULL: update p
 * is row p.  16-byte-aligned buffers with the unweighted vector shapes and dh % 4 == 0 (fp32) /
 * dh % 8 == 0 (16-bit) take the 16-byte-lane kernels.  EULER_GPU_EINVAL: heads < 1, heads not
 * dividing d, a null buffer, e >= 2^31, mean with e (or count) >= 2^24.  size == 0 or d == 0
 * returns EULER_GPU_OK and touches nothing. */
int euler_gpu_gather_scatter_w(void* stream, int32_t mode, const float* params_dev,
                               const int32_t* gather_indices_dev,
                               const int32_t* scatter_indices_dev, int64_t e, int64_t d,
                               int32_t size, float* out_dev, const float* w_dev, int32_t heads);
int euler_gpu_gather_segment_reduce_w(void* stream, int32_t mode, const float* params_dev,
                                      const int32_t* gather_indices_dev,
                                      const int64_t* seg_ptr_dev, int64_t count, int64_t d,
                                      int32_t size, float* out_dev, const float* w_dev,
                                      int32_t heads);
int euler_gpu_gather_segment_reduce_ids_w(void* stream, int32_t mode, const float* params_dev,
                                          int64_t params_rows, const int64_t* gather_ids_dev,
                                          const int64_t* seg_ptr_dev, int64_t count, int64_t d,
                                          int32_t size, float* out_dev, const float* w_dev,
                                          int32_t heads);
int euler_gpu_gather_scatter_w_t(void* stream, int32_t mode, const void* params_dev, int32_t in_dtype,
                                 const int32_t* gather_indices_dev,
                                 const int32_t* scatter_indices_dev, int64_t e, int64_t d,
                                 int32_t size, void* out_dev, int32_t out_dtype, const void* w_dev,
                                 int32_t w_dtype, int32_t heads);
int euler_gpu_gather_segment_reduce_w_t(void* stream, int32_t mode, const void* params_dev,
                                        int32_t in_dtype, const int32_t* gather_indices_dev,
                                        const int64_t* seg_ptr_dev, int64_t count, int64_t d,
                                        int32_t size, void* out_dev, int32_t out_dtype,
                                        const void* w_dev, int32_t w_dtype, int32_t heads);
int euler_gpu_gather_segment_reduce_ids_w_t(void* stream, int32_t mode, const void* params_dev,
                                            int32_t in_dtype, int64_t params_rows,
                                            const int64_t* gather_ids_dev,
                                            const int64_t* seg_ptr_dev, int64_t count, int64_t d,
                                            int32_t size, void* out_dev, int32_t out_dtype,
                                            const void* w_dev, int32_t w_dtype, int32_t heads);
/* out[p][h] = sum over c < dh of a[a_index[p]][h * dh + c] * b[b_index[p]][h * dh + c], dh =
 * d / heads: the per-edge dot product of two gathered rows - the gradient of the entries above
 * with respect to w, and AGNN's attention logit (agnn_conv.py:43-47) - without either [e, d]
 * block of gathered rows.  An index array may be NULL (row p); indices must be valid rows.  fp32
 * products and fp32 sums in a fixed order that depends on dh, the types and the 16-byte alignment
 * of the tables, never on e or the launch (stated in euler_amd/csrc/edge_dot_kernels.hip): the
 * same call returns the same bits; dh = 1 returns the fp32 product.  out_dev is [e, heads].
 * The _t form: each table has its own storage type, out_dtype is any of the three (one
 * rounding).  EULER_GPU_EINVAL: heads < 1, heads not dividing d, a null buffer, e >= 2^31, an
 * unknown dtype.  e == 0 or d == 0 returns EULER_GPU_OK and touches nothing. */
int euler_gpu_edge_dot(void* stream, const float* a_dev, const int32_t* a_index_dev,
                       const float* b_dev, const int32_t* b_index_dev, int64_t e, int64_t d,
                       int32_t heads, float* out_dev);
int euler_gpu_edge_dot_t(void* stream, const void* a_dev, int32_t a_dtype,
                         const int32_t* a_index_dev, const void* b_dev, int32_t b_dtype,
                         const int32_t* b_index_dev, int64_t e, int64_t d, int32_t heads,
                         void* out_dev, int32_t out_dtype);

/* ---- quantised (FP8) feature row tables -------------------------------------------
 * A table is q_dev, [rows, d] uint8 codes of OCP e4m3fn (what torch.float8_e4m3fn and gfx950's
 * converts use: 0x7f / 0xff NaN, no inf, largest finite value 448, subnormals m * 2^-9), plus
 * scale_dev, [d] fp32 finite positive values, one per COLUMN.  Its value is
 *   x^[r][c] = fl(Dec(q[r][c]) * scale[c])          (one correctly rounded fp32 multiply)
 * and an entry below that reads a table is the fp32 entry above on x^: the same fp32 adds in
 * input order, the same compares for max and the -1e9 empty row, mean = sum / (length + 1e-7f),
 * the same min((uint32) low word, rows - 1) treatment of int64 ids, the weighted product formed
 * as the _w entries form it - stored as fp32 unchanged or rounded once, to nearest even, to
 * bf16 / fp16 (out_dtype: any of EULER_GPU_F32 / _BF16 / _F16).  Nothing is accumulated below
 * fp32, so the result has the bits of the fp32 entry on the dequantised table.  These are new
 * entries: no `_t` entry accepts a code for this storage.
 *
 * euler_gpu_column_absmax: absmax_dev[c] = max(absmax_dev[c], max |x[r][c]|) over the FINITE
 * values of column c of x_dev ([n, d] of `dtype`; NaN and +-inf are skipped) - in/out, so that a
 * table is scanned in chunks; the caller zeroes it first.  Exact (a max has no order).  The scale
 * of a column is absmax / 448.0f, or 1.0f where absmax is 0 (the caller's arithmetic).
 * euler_gpu_fp8_quantize_rows: q_dev[r][c] = Enc(x[r][c] / scale[c]) for the n rows of x_dev - an
 * IEEE fp32 division, then round to nearest even into e4m3fn with subnormals, after a clamp to
 * [-448, 448]: +-inf and everything past the scale saturate to +-448, NaN gives 0x7f | sign, -0
 * gives 0x80.  16-bit x is widened exactly first.  q_dev may point into a larger table.
 * euler_gpu_fp8_gather: out[i][:] = x^[indices[i]][:], e rows of out_dtype; indices are trusted.
 * euler_gpu_fp8_gather_segment_reduce / _ids: euler_gpu_gather_segment_reduce_t / _ids_t over x^
 * (mode 0 add, 1 max, 2 mean; seg_ptr_dev or `count`; gather_indices_dev NULL: update p is row p),
 * and with w_dev != NULL their _w_t forms: w_dev [e, heads] of w_dtype (any of the three), heads
 * dividing d.  w_dev == NULL: unweighted, w_dtype and heads are not looked at.
 * 16-byte aligned q_dev / out_dev with d % 16 == 0, d <= 1024, d / 16 a divisor of 64 (and
 * (d / heads) % 16 == 0) take the 16-byte-lane reduce kernels - a 128-d row is one 128-byte line -,
 * every other shape a column per lane; the gather reads four codes a lane into fp32 rows (d % 4 == 0,
 * q_dev 4-byte and out_dev 16-byte aligned) and sixteen into 16-bit rows (d % 16 == 0, both 16-byte
 * aligned), else one.  A table may be larger than 2^32 bytes.
 * EULER_GPU_EINVAL, checked in this order: an unknown dtype code, weights not aligned to their
 * type; mode, heads < 1, heads not dividing d; a negative shape; [size == 0 or d == 0 (e, n):
 * EULER_GPU_OK, nothing is touched]; a null buffer; e >= 2^31 (weighted); mean with count >= 2^24;
 * params_rows outside [0, 2^31); a buffer not aligned to its type. */
int euler_gpu_column_absmax(void* stream, const void* x_dev, int32_t dtype, int64_t n, int64_t d,
                            float* absmax_dev);
int euler_gpu_fp8_quantize_rows(void* stream, const void* x_dev, int32_t dtype, int64_t n, int64_t d,
                                const float* scale_dev, uint8_t* q_dev);
int euler_gpu_fp8_gather(void* stream, const uint8_t* q_dev, const float* scale_dev,
                         const int32_t* indices_dev, int64_t e, int64_t d, int64_t n_rows,
                         void* out_dev, int32_t out_dtype);
int euler_gpu_fp8_gather_segment_reduce(void* stream, int32_t mode, const uint8_t* q_dev,
                                        const float* scale_dev, const int32_t* gather_indices_dev,
                                        const int64_t* seg_ptr_dev, int64_t count, int64_t d,
                                        int32_t size, void* out_dev, int32_t out_dtype,
                                        const void* w_dev, int32_t w_dtype, int32_t heads);
int euler_gpu_fp8_gather_segment_reduce_ids(void* stream, int32_t mode, const uint8_t* q_dev,
                                            const float* scale_dev, int64_t params_rows,
                                            const int64_t* gather_ids_dev,
                                            const int64_t* seg_ptr_dev, int64_t count, int64_t d,
                                            int32_t size, void* out_dev, int32_t out_dtype,
                                            const void* w_dev, int32_t w_dtype, int32_t heads);
/* gcn_norm: the two tables of the symmetric degree normalisation of GCN / APPNP / SGCN / TAG /
 * ARMA / DNA (gcn_conv.py:33-51: norm = deg ** -0.5 on both sides of a block).  dst_keys_dev and
 * src_keys_dev are int32 [e]; an edge counts if and only if BOTH keys are in range (dst in
 * [0, size_dst), src in [0, size_src)): an edge the reduce below leaves out changes nobody's
 * degree.  norm_dst_out_dev [size_dst] and norm_src_out_dev [size_src] get
 * 1 / sqrt((float)deg) - a correctly rounded fp32 square root and a correctly rounded fp32 divide:
 * the bits of numpy's float32(1) / sqrt(float32(deg)) - and exactly 0 where deg == 0 (the
 * reference's inf there is never multiplied into anything; 0 keeps the tables finite).  The
 * degrees are counted with int32 atomics into stream-ordered scratch: no grouping of the keys, no
 * sort, no host wait, and the same bits on every call.  One kernel writes both tables: both or
 * neither.  EULER_GPU_EINVAL: a negative shape, a null buffer, e >= 2^31, a buffer that is not
 * 4-byte aligned.  size_dst == 0 and size_src == 0 returns EULER_GPU_OK and touches nothing. */
int euler_gpu_gcn_norm(void* stream, const int32_t* dst_keys_dev, const int32_t* src_keys_dev,
                       int64_t e, int32_t size_dst, int32_t size_src, float* norm_dst_out_dev,
                       float* norm_src_out_dev);
/* gather_reduce_norm: the weighted fused reduce above whose weight is formed from two node
 * tables instead of read from an [e] array:
 *   out[r][c] = reduce over the updates p of r, in input order, of
 *               fl(x[g(p)][c] * fl(norm_dst[r] * norm_src[g(p)])),   g = gather_indices_dev
 * - three separate fp32 roundings, in the order of norm_i * norm_j * x_j: the bits of
 * euler_gpu_gather_scatter_w_t with w[p] = norm_dst[dst[p]] * norm_src[g(p)] (fp32).  mode is 0
 * (add) or 2 (mean: divided by segment length + 1e-7f); max is refused.  x_dev is [rows, d] in
 * fp32 / bf16 / fp16, the norm tables are fp32 ([size] and [rows]), out_dtype is fp32 or in_dtype
 * (one rounding at the store).  The destinations come in exactly one of the three forms of
 * euler_gpu_edge_softmax (indices_dev, seg_ptr_dev, count > 0); e is the number of gather indices.
 * An update whose gather index lies outside [0, rows) contributes nothing: weight 0, row clamped
 * to the last one - for finite tables every bit of the result is that of the reduce without it
 * (euler_amd/csrc/mp_gcn.h).  A backward pass can therefore gather by a destination key that is
 * out of range, without an appended zero row.
 * root_dev (NULL: no epilogue, the scales are not read) is [size, d] in root_dtype (fp32 or
 * in_dtype): out = fl(fl(agg * agg_scale) + fl(root[r] * root_scale)), formed in fp32 before the
 * one rounding to out_dtype - APPNP's (1 - alpha, alpha), ARMA's (1, 1).
 * 16-byte-aligned x, root and out with the vector shapes of the weighted entries take the
 * 16-byte-lane kernels.  EULER_GPU_EINVAL, in this order: an unknown dtype, out_dtype / root_dtype
 * neither fp32 nor in_dtype; mode not 0 or 2; a negative shape, not exactly one segment form, count
 * with e != size * count; (size == 0 or d == 0 returns EULER_GPU_OK and touches nothing;) a null
 * buffer - out and norm_dst whenever there is a destination; x, the gather indices and norm_src when
 * e > 0 and rows > 0 (an empty table may be null: nothing of it is read); e or rows >= 2^31; mean
 * with e (keys, seg_ptr) or count >= 2^24; a buffer not aligned to its type.  A refused call writes
 * nothing. */
int euler_gpu_gather_reduce_norm_t(void* stream, int32_t mode, const void* x_dev, int32_t in_dtype,
                                   int64_t rows, const int32_t* gather_indices_dev,
                                   const int32_t* indices_dev, const int64_t* seg_ptr_dev,
                                   int64_t count, int64_t e, int64_t d, int32_t size,
                                   const float* norm_dst_dev, const float* norm_src_dev,
                                   const void* root_dev, int32_t root_dtype, float agg_scale,
                                   float root_scale, void* out_dev, int32_t out_dtype);
/* edge_softmax: the softmax of the [e, heads] logits over the updates of every destination -
 * what GATConv and AGNNConv run between the logit and the aggregate (gat_conv.py:66-72), the
 * reference's scatter_softmax (tf_euler/python/euler_ops/mp_ops.py:76-79) - in one read and one
 * write, and its gradient gx_p = y_p * (g_p - sum_q y_q g_q) on the forward's output y.
 * What differs from the composition scatter_max / gather / exp / scatter_add / gather / divide:
 * the exponential is the library's own (ExpNonPositive of euler_amd/csrc/mp_softmax.h: correctly
 * rounded fp32 operations only, +0 below -86, error bound in DESIGN 4.11), and the sum runs in the
 * order that header states - a function of the segment length and of heads, never of e, size or
 * the launch.  So the bits are NOT those of the composition; they are the same for the same
 * segment through every form, on every call, and on the host build of the header.
 * The destinations are given in exactly ONE of three forms: indices_dev (int32 scatter keys, e of
 * them, any order; grouped by one stable sort a call when they are not non-decreasing, values are
 * read and written at their input position), seg_ptr_dev (int64, size + 1 non-decreasing offsets
 * into the e updates; those outside [seg_ptr[0], seg_ptr[size]) have no destination), or count > 0
 * (destination r owns updates [r * count, (r + 1) * count); e == size * count).  An empty segment
 * writes nothing; updates that belong to no destination (a key outside [0, size), a position
 * outside the span of seg_ptr) get 0 (output and gradient); a -inf
 * logit beside a finite maximum gets exactly 0.  A segment whose maximum is not finite (all -inf,
 * a +inf) returns NaN for all of it; a NaN logit is left out of the maximum and gets 0.
 * Storage: logits fp32 / bf16 / fp16, out_dtype fp32 or in_dtype (one rounding); in the gradient
 * y, grad and the output are each any of the three; all arithmetic is fp32.
 * EULER_GPU_EINVAL: heads < 1, a null buffer, an unknown dtype, e >= 2^31, not exactly one
 * segment form, count with e != size * count.  e == 0 returns EULER_GPU_OK and touches nothing. */
int euler_gpu_edge_softmax(void* stream, const void* logits_dev, int32_t in_dtype,
                           const int32_t* indices_dev, const int64_t* seg_ptr_dev, int64_t count,
                           int64_t e, int32_t heads, int32_t size, void* out_dev,
                           int32_t out_dtype);
int euler_gpu_edge_softmax_grad(void* stream, const void* y_dev, int32_t y_dtype,
                                const void* grad_dev, int32_t grad_dtype,
                                const int32_t* indices_dev, const int64_t* seg_ptr_dev,
                                int64_t count, int64_t e, int32_t heads, int32_t size,
                                void* out_dev, int32_t out_dtype);
/* segment_attention: attention over the updates of every destination in one pass - a logit per
 * (update, head), the softmax of euler_gpu_edge_softmax over the destination's updates, and the
 * sum of the gathered rows weighted by it: GATConv (convolution/gat_conv.py:66-72), AGNNConv
 * (convolution/agnn_conv.py:36-54), AttentionPool (graph_pool/attention_pool.py:36-40) and
 * Set2SetPool (graph_pool/set2set_pool.py:45-49).  For destination r (qr = q_index_dev[r], or r),
 * update p gathering row g = gather_dev[p] and head h:
 *   kind 0 (dot):       logit = fl(scale * DOT_c q[qr][h dh + c] * k[g][h dh + c]), q and k [*, d],
 *                       dh = d / heads, in the order euler_amd/csrc/mp_attention.h states (a
 *                       function of dh alone);
 *   kind 1 (additive):  a = fl(q[qr][h] + k[g][h]), logit = a < 0 ? fl(a * negative_slope) : a,
 *                       q and k [*, heads] (d == heads), q_dev NULL: q = +0;
 *   alpha = the bits euler_gpu_edge_softmax returns for these logits;
 *   out[r][c] = +0, then fl(acc + fl(v[g][c] * alpha[p][c / (dv / heads)])) in increasing p: the
 *   bits of euler_gpu_gather_segment_reduce_w_t (add) with alpha as the weights.
 * v_dev NULL (dot only, dv == d): v is k, and each gathered row is loaded once for both uses.
 * Tables fp32 / bf16 / fp16, each its own; gather_dev int32 indices (gather_is_ids == 0) or int64
 * ids (index = low word); every row number is clamped to its table's last row.  The destinations
 * come in exactly one of the three forms of euler_gpu_edge_softmax.  out_dev is [size, dv]
 * (out_dtype: any of the three, one rounding); an empty destination is a zero row.  alpha_dev
 * (fp32 [e, heads], may be NULL) receives alpha, 0 for updates that belong to no destination;
 * logits_dev (may be NULL) the logits of the updates that have one.  A segment whose maximum
 * logit is not finite is outside the contract, as for euler_gpu_edge_softmax.
 * segment_attention_grad: the destination side of the backward in one pass, from the saved
 * alpha_dev and the incoming grad_dev [size, dv]: da = DOT_c grad[r] * v[g] per head (the order
 * above over dv / heads), dl = the gradient of euler_gpu_edge_softmax_grad,
 *   dot:       ds = fl(scale * dl),  dq_dst[r] = the ordered fold of k[g] with ds   ([size, d]);
 *   additive:  ds = a < 0 ? fl(dl * negative_slope) : dl,  dq_dst[r][h] = +0 + ds_0 + ds_1 ...
 * ds_dev is fp32 [e, heads] (0 for updates without a destination), dq_dst_dev fp32 [size, d].
 * The source-side gradients (grouped by gathered row) are euler_gpu_gather_scatter_w_t calls.
 * No float atomics; explicit keys that are not grouped cost GroupScatterKeys' one host wait.
 * EULER_GPU_EINVAL: unknown kind or dtype, heads < 1 or not dividing d / dv (additive: d !=
 * heads), additive without v, not exactly one segment form, count with e != size * count,
 * e >= 2^31, a null buffer, a table without rows.  size == 0 and e == 0 touches nothing. */
int euler_gpu_segment_attention(void* stream, int32_t kind, const void* q_dev, int32_t q_dtype,
                                int64_t q_rows, const int32_t* q_index_dev, const void* k_dev,
                                int32_t k_dtype, int64_t k_rows, const void* v_dev, int32_t v_dtype,
                                int64_t v_rows, const void* gather_dev, int32_t gather_is_ids,
                                const int32_t* indices_dev, const int64_t* seg_ptr_dev,
                                int64_t count, int64_t e, int64_t d, int64_t dv, int32_t heads,
                                int32_t size, float scale, float negative_slope, void* out_dev,
                                int32_t out_dtype, float* alpha_dev, float* logits_dev);
int euler_gpu_segment_attention_grad(void* stream, int32_t kind, const void* q_dev, int32_t q_dtype,
                                     int64_t q_rows, const int32_t* q_index_dev, const void* k_dev,
                                     int32_t k_dtype, int64_t k_rows, const void* v_dev,
                                     int32_t v_dtype, int64_t v_rows, const void* gather_dev,
                                     int32_t gather_is_ids, const int32_t* indices_dev,
                                     const int64_t* seg_ptr_dev, int64_t count, int64_t e, int64_t d,
                                     int64_t dv, int32_t heads, int32_t size, float scale,
                                     float negative_slope, const float* alpha_dev,
                                     const void* grad_dev, int32_t grad_dtype, float* ds_dev,
                                     float* dq_dst_dev);
/* relation_reduce: the aggregation of RGCN's RelationConv (relation_conv.py:53-70) by linearity -
 * mean_e W[t_e] x_e = (sum_t W_t * sum_{e: t_e = t} x_e) / deg - as the reduce of gathered rows
 * per (destination, relation): out_dev is [size, num_relations, d], which one dense GEMM with the
 * relation matrices then finishes; the [e, dim, fea_dim] block of per-edge matrices is never built.
 * Update p has a destination (below), a row of params and the relation edge_type_dev[p] (int32,
 * by the update's position in the INPUT).  It is valid when it has a destination in [0, size) and
 * 0 <= type < num_relations; an invalid update (the -1 the samplers write beside a default_node
 * fill) belongs to no bucket: it is left out of every sum, maximum and count and its row is not
 * read.  out[r][t][c] folds the widened params rows of the valid updates of bucket (r, t) in input
 * order, all in fp32: mode 0 add, 1 max (from -1e9), 2 the sum / fl(n_valid(r) + 1e-7f) with
 * n_valid(r) the valid updates of the destination (RelationConv's aggr = 'mean'), 3 the sum /
 * fl(cnt(r, t) + 1e-7f) (the 1 / c_{i,r} of the RGCN paper).  The bits are those of
 * euler_gpu_gather_scatter with the keys dst * R + type (-1 for an invalid update): add, max and
 * mode 3 as its add, max and mean; mode 2 its add divided by the destination's denominator.
 * Every bucket is written exactly once: an empty one is 0 (add, the means) or -1e9 (max).
 * counts_dev (may be NULL) receives cnt(r, t) as [size, num_relations] int32.
 * gather_dev: NULL (update p is row p; params_rows >= e), int32 indices (gather_is_ids == 0) or
 * the int64 ids a sampler returned (index = low word), either clamped to params_rows - 1 exactly
 * as euler_gpu_gather_segment_reduce_ids does.  The destinations come in exactly one of the
 * three forms of euler_gpu_edge_softmax: indices_dev (int32 keys, any order; grouped by one
 * stable sort a call when they are not non-decreasing, which waits on the host), seg_ptr_dev or
 * count > 0 with e == size * count; the last two only enqueue - no allocation, no host wait.
 * Storage: params fp32 / bf16 / fp16, out_dtype fp32 or in_dtype (one rounding at the store).
 * EULER_GPU_EINVAL: mode outside 0..3, num_relations < 1, size * num_relations >= 2^31,
 * e >= 2^31, a mean with e or count >= 2^24, not exactly one segment form, count with
 * e != size * count, a null buffer, an unknown dtype, out_dtype neither fp32 nor in_dtype, a
 * table shorter than the rows read.  size == 0 or d == 0 returns EULER_GPU_OK and touches
 * nothing; e == 0 with size > 0 writes the empty-bucket values (and zero counts). */
int euler_gpu_relation_reduce(void* stream, int32_t mode, const void* params_dev, int32_t in_dtype,
                              int64_t params_rows, const void* gather_dev, int32_t gather_is_ids,
                              const int32_t* edge_type_dev, int32_t num_relations,
                              const int32_t* indices_dev, const int64_t* seg_ptr_dev, int64_t count,
                              int64_t e, int64_t d, int32_t size,
                              void* out_dev, int32_t out_dtype, int32_t* counts_dev);
/* triple_score: the energies of knowledge-graph embedding (calculate_energy of
 * examples/TransX/transX.py:72-79,105-133 and examples/distmult/distmult.py:74-79,99-126) - the
 * lookup of the rows of src, rel_id, dst and the [b, k] negatives, their l2 normalisation
 * (normalize != 0: x / sqrt(max(sum x^2, 1e-12f)), tf.nn.l2_normalize) and the scores - in one
 * pass: 3 + k table rows read and 1 + K' floats written per triple, no [b, k, d] intermediate.
 * With h, r, t, n_j the (normalised) rows and e = a + r - c, the score s(a, r, c) is
 * kind 0 trans_l1 -sum |e|, 1 trans_l2 -sqrt(sum e * e), 2 distmult sum (a * r) * c.
 * pos_out_dev [b] = s(h, r, t).  neg_out_dev [b, K']: corrupt 0 front, K' = k, s(n_j, r, t);
 * 1 tail, K' = k, s(h, r, n_j); 2 both, K' = 2 k, the front scores then the tail scores of the
 * same negatives.  Ids are signed int64; an id outside [0, rows) of its table names no row: it is
 * never dereferenced, reads as a row of zeros and gets a zero gradient row.  The tables are fp32,
 * bf16 or fp16, each its own type, widened exactly; all arithmetic is fp32, every sum over columns
 * in the fixed order stated in euler_amd/csrc/kg_score.h (it depends on d, the types and the
 * 16-byte alignment of the two tables, never on b, k or the launch).
 * triple_score_grad: from g_pos_dev [b] and g_neg_dev [b, K'] the fp32 gradients of the RAW rows
 * per occurrence - g_src_dev, g_rel_dev, g_dst_dev [b, d], g_neg_rows_dev [b, k, d] - through
 * the scores and the normalisation (sign(0) = 0 for trans_l1; a zero gradient where the l2 norm
 * is 0); a table's gradient is their scatter_add by id.
 * Both only enqueue: no allocation, no host wait.  EULER_GPU_EINVAL: kind or corrupt outside
 * 0..2, an unknown dtype, k < 0, a table with fewer than 1 row, b * max(k, 1) * 2 >= 2^31,
 * d >= 2^31, a null required buffer, k > 0 with neg_dev or its outputs null, a buffer not aligned
 * to its type.  b == 0 or d == 0 returns EULER_GPU_OK and touches nothing; k == 0 leaves the
 * negative outputs untouched (neg_dev and they may be NULL). */
int euler_gpu_triple_score(void* stream, int32_t kind, int32_t normalize, int32_t corrupt,
                           const void* ent_dev, int32_t ent_dtype, int64_t ent_rows,
                           const void* rel_dev, int32_t rel_dtype, int64_t rel_rows,
                           const int64_t* src_dev, const int64_t* rel_id_dev,
                           const int64_t* dst_dev, const int64_t* neg_dev, int64_t b, int64_t k,
                           int64_t d, float* pos_out_dev, float* neg_out_dev);
int euler_gpu_triple_score_grad(void* stream, int32_t kind, int32_t normalize, int32_t corrupt,
                                const void* ent_dev, int32_t ent_dtype, int64_t ent_rows,
                                const void* rel_dev, int32_t rel_dtype, int64_t rel_rows,
                                const int64_t* src_dev, const int64_t* rel_id_dev,
                                const int64_t* dst_dev, const int64_t* neg_dev, int64_t b,
                                int64_t k, int64_t d, const float* g_pos_dev,
                                const float* g_neg_dev, float* g_src_dev, float* g_rel_dev,
                                float* g_dst_dev, float* g_neg_rows_dev);
/* triple_score_proj: triple_score with the projection of TransH or TransD fused in
 * (projection / generate_embedding of examples/TransX/transH.py:43-66 and transD.py:46-73): the
 * lookups of the extra tables, the projection of every entity row, the normalisations and the
 * scores in one pass, no [b, k, d] intermediate.  N(x) is tf.nn.l2_normalize as in triple_score.
 * proj 1 "hyperplane" (TransH): ent_aux_dev is NULL and rel_aux_dev is hyper [rel_rows, d];
 *   w = N(hyper[rel_id]), r = N(rel[rel_id]); an entity row x is NOT normalised and becomes
 *   x - (sum x * w) w; the scores take the projected h, t, n_j.
 * proj 2 "transfer" (TransD): ent_aux_dev is ent_transfer [ent_rows, d] and rel_aux_dev is
 *   rel_transfer [rel_rows, d]; with rho = rel_transfer[rel_id] (raw), x = ent[i] and
 *   a = ent_transfer[i] an entity row becomes N(x + (sum x * a) rho); r = N(rel[rel_id]).
 * kind is 0 trans_l1 or 1 trans_l2 of triple_score; corrupt, pos_out_dev [b] and neg_out_dev
 * [b, K'] are triple_score's; the projection of n_j serves its front and its tail score.  The
 * tables indexed by an entity id share ent_dtype and ent_rows, those indexed by a relation id
 * rel_dtype and rel_rows (fp32, bf16 or fp16, widened exactly).  Ids are signed int64; an id
 * outside [0, rows) names no row in any table it indexes: it is never dereferenced, reads as
 * zeros and gets zero gradient rows.  All arithmetic is fp32 in the fixed order stated in
 * euler_amd/csrc/kg_proj.h (it depends on d, the types and the alignment of all tables passed,
 * never on b, k or the launch).
 * triple_score_proj_grad: from g_pos_dev [b] and g_neg_dev [b, K'] the fp32 gradients of the RAW
 * rows per occurrence - g_src_dev, g_rel_dev, g_dst_dev [b, d] and g_neg_rows_dev [b, k, d] as in
 * triple_score_grad, g_rel_aux_dev [b, d] for hyper / rel_transfer and, for proj 2 only (NULL for
 * proj 1), g_src_aux_dev, g_dst_aux_dev [b, d] and g_neg_aux_rows_dev [b, k, d] for ent_transfer;
 * a table's gradient is their scatter_add by id.
 * Both only enqueue: no allocation, no host wait.  EULER_GPU_EINVAL: the rules of triple_score,
 * proj outside 1..2, kind outside 0..1 (distmult takes no projection), a missing aux table or
 * aux gradient buffer, an aux table or aux gradient buffer that should be NULL.  b == 0 or
 * d == 0 returns EULER_GPU_OK and touches nothing; k == 0 leaves the negative outputs untouched
 * (neg_dev and they may be NULL). */
int euler_gpu_triple_score_proj(void* stream, int32_t proj, int32_t kind, int32_t corrupt,
                                const void* ent_dev, const void* ent_aux_dev, int32_t ent_dtype,
                                int64_t ent_rows, const void* rel_dev, const void* rel_aux_dev,
                                int32_t rel_dtype, int64_t rel_rows, const int64_t* src_dev,
                                const int64_t* rel_id_dev, const int64_t* dst_dev,
                                const int64_t* neg_dev, int64_t b, int64_t k, int64_t d,
                                float* pos_out_dev, float* neg_out_dev);
int euler_gpu_triple_score_proj_grad(void* stream, int32_t proj, int32_t kind, int32_t corrupt,
                                     const void* ent_dev, const void* ent_aux_dev,
                                     int32_t ent_dtype, int64_t ent_rows, const void* rel_dev,
                                     const void* rel_aux_dev, int32_t rel_dtype, int64_t rel_rows,
                                     const int64_t* src_dev, const int64_t* rel_id_dev,
                                     const int64_t* dst_dev, const int64_t* neg_dev, int64_t b,
                                     int64_t k, int64_t d, const float* g_pos_dev,
                                     const float* g_neg_dev, float* g_src_dev, float* g_rel_dev,
                                     float* g_dst_dev, float* g_neg_rows_dev, float* g_rel_aux_dev,
                                     float* g_src_aux_dev, float* g_dst_aux_dev,
                                     float* g_neg_aux_rows_dev);
/* triple_score_matrix: triple_score with TransR's per-relation matrix projection fused in
 * (generate_embedding of examples/TransX/transR.py:41-68): tables ent [ent_rows, de],
 * rel [rel_rows, dr] and matrix [rel_rows, de * dr], read row-major as M_rho [de, dr]; an entity
 * row x is NOT normalised and becomes N(x . M_rho), r = N(rel[rho]), N = tf.nn.l2_normalize as in
 * triple_score.  kind is 0 trans_l1 or 1 trans_l2 over the dr columns; corrupt, pos_out_dev [b]
 * and neg_out_dev [b, K'] are triple_score's; the projection of n_j serves its front and its tail
 * score.  No triple fetches a matrix of its own and no [b, k, de * dr] block exists: the triples
 * are worked on grouped by relation and a workgroup stages M_rho once per run of equal relation.
 * The three tables are fp32, bf16 or fp16, each its own type, widened exactly.  Ids are signed
 * int64; an id outside [0, rows) names no row in any table it indexes (a rel_id removes rel[rho]
 * AND M_rho): never dereferenced, reads as zeros, gets zero gradient rows.  All arithmetic is
 * fp32 in the fixed orders stated in euler_amd/csrc/kg_matrix.h (they depend on de, dr, the types
 * and the alignment of rel, never on b, k, the grouping or the launch).
 * THE GROUPING is prepared by the caller, with key(t) = rel_id[t] if 0 <= rel_id[t] < rel_rows,
 * else rel_rows:
 *   order_dev [b]        a permutation of 0 .. b - 1 that sorts key(t) ascending and is STABLE
 *                        (equal keys keep increasing t).
 *   seg_ptr_dev [nseg+1] non-decreasing positions into order_dev; segment s is the positions
 *   seg_rel_dev [nseg]   [seg_ptr[s], seg_ptr[s + 1]) and must hold exactly the triples whose key
 *                        is seg_rel[s].  Lengths may be 0: nseg = rel_rows with seg_rel[s] = s is
 *                        valid and needs no host wait.  Triples of key rel_rows belong to no
 *                        segment.
 * An order that is not a permutation, or wrong segments, are the caller's error and give wrong
 * numbers only: an entry of order_dev outside [0, b) is skipped, seg_ptr is clamped to [0, b], a
 * triple whose key is not its segment's relation and a segment whose seg_rel names no relation
 * contribute nothing; no kernel reads or writes outside its buffers.
 * triple_score_matrix_grad: from g_pos_dev [b] and g_neg_dev [b, K'] the fp32 gradients of the RAW
 * rows per occurrence - g_src_dev, g_dst_dev [b, de], g_neg_rows_dev [b, k, de], g_rel_dev
 * [b, dr]; a table's gradient is their scatter_add by id - the rows gz (the gradient of every
 * projected row before its normalisation) gz_src_dev, gz_dst_dev [b, dr], gz_neg_rows_dev
 * [b, k, dr], which the caller provides as scratch, and g_matrix_dev [nseg, de * dr] in the
 * matrix's dtype: row s is the gradient of M_{seg_rel[s]}, summed over the segment's occurrences
 * in the stated order (no float atomics) and written once; +0 for a segment without a term.
 * nseg == 0 computes no matrix gradient (seg_ptr_dev, seg_rel_dev and g_matrix_dev may be NULL).
 * Both only enqueue (the gradient three kernels): no allocation, no host wait; both can be
 * captured into a graph.  EULER_GPU_EINVAL: the rules of triple_score_proj, de or dr above 512,
 * ent_rows >= 2^31, order_dev null, nseg < 0 or >= 2^31, nseg > 0 with a null segment array or
 * g_matrix_dev.  b == 0, de == 0 or dr == 0 returns EULER_GPU_OK and touches nothing; k == 0
 * leaves the negative outputs untouched (neg_dev and they may be NULL). */
int euler_gpu_triple_score_matrix(void* stream, int32_t kind, int32_t corrupt, const void* ent_dev,
                                  int32_t ent_dtype, int64_t ent_rows, int64_t de,
                                  const void* rel_dev, int32_t rel_dtype, int64_t rel_rows,
                                  int64_t dr, const void* matrix_dev, int32_t matrix_dtype,
                                  const int64_t* src_dev, const int64_t* rel_id_dev,
                                  const int64_t* dst_dev, const int64_t* neg_dev, int64_t b,
                                  int64_t k, const int64_t* order_dev, float* pos_out_dev,
                                  float* neg_out_dev);
int euler_gpu_triple_score_matrix_grad(void* stream, int32_t kind, int32_t corrupt,
                                       const void* ent_dev, int32_t ent_dtype, int64_t ent_rows,
                                       int64_t de, const void* rel_dev, int32_t rel_dtype,
                                       int64_t rel_rows, int64_t dr, const void* matrix_dev,
                                       int32_t matrix_dtype, const int64_t* src_dev,
                                       const int64_t* rel_id_dev, const int64_t* dst_dev,
                                       const int64_t* neg_dev, int64_t b, int64_t k,
                                       const int64_t* order_dev, const int64_t* seg_ptr_dev,
                                       const int64_t* seg_rel_dev, int64_t nseg,
                                       const float* g_pos_dev, const float* g_neg_dev,
                                       float* g_src_dev, float* g_rel_dev, float* g_dst_dev,
                                       float* g_neg_rows_dev, float* gz_src_dev, float* gz_dst_dev,
                                       float* gz_neg_rows_dev, void* g_matrix_dev);
/* skipgram_loss: the loss head of the walk-based models (DeepWalk, node2vec, LINE, unsupervised
 * GraphSAGE: tf_euler/python/solution/base_unsupervise.py with PosNegLogits of
 * solution/logits.py:30-34, xent_loss of solution/losses.py:27-33 and mrr_score / hitk_score /
 * mr_score of utils/metrics.py:51-83) in one pass: the lookup of t = target[src[i]] and of the
 * p + k context rows c_j = context[pos[i][j]] (j < p), context[neg[i][j - p]] (j >= p), the
 * logits x_j = sum t * c_j, the sigmoid cross-entropy softplus(-x_j) of a positive and
 * softplus(x_j) of a negative, and the rank of the LAST positive - 1 + p + k table rows read once
 * each per pair row, no [b, 1 + k, d] block, no matmul, no sort.
 * logits_dev [b, p + k] fp32, positives first.  rank_dev [b] int32: how many of the k negatives
 * and the first p - 1 positives have a logit >= the last positive's (tf.nn.top_k's
 * lower-index-first rule on concat([neg, pos]): a tie goes against the positive).  row_loss_dev
 * [b]: the terms of a row added in the order j = 0 .. p + k - 1.  loss_dev [1]: the row sums
 * reduced in a fixed order that is a function of b alone, divided once by float(b * (p + k)).
 * The tables are fp32, bf16 or fp16, each its own type (they may be the same table), widened
 * exactly; ids are signed int64; an id outside [0, rows) of its table names no row: it is never
 * dereferenced, reads as a row of zeros (its term, ln 2, still counts) and gets a zero gradient
 * row.  All arithmetic is correctly rounded fp32 in the order stated in
 * euler_amd/csrc/skipgram.h, exp and log1p included: the same call returns the same bits, and no
 * float atomic is used.  NaN logits are outside the contract.
 * skipgram_loss_grad: from the forward's logits_dev and the scalar g_dev [1] (the gradient of
 * the loss) the fp32 gradients of the RAW rows per occurrence - g_src_dev [b, d] (target),
 * g_pos_dev [b, p, d] and g_neg_dev [b, k, d] (context); no dot product is taken again.  A
 * table's gradient is their scatter_add by id.
 * Both only enqueue (the forward two kernels): no allocation, no host wait; both can be captured
 * into a graph.  EULER_GPU_EINVAL, checked before anything is enqueued, so every output is
 * written entirely or not at all: an unknown dtype, b < 0, k < 0, p < 1, d < 1, d >= 2^31, a
 * table with fewer than 1 or with 2^31 or more rows, b * (p + k) >= 2^31, a null required buffer,
 * k > 0 with neg_dev or g_neg_dev null, a buffer not aligned to its type.  b == 0: the forward
 * writes loss_dev = +0 and touches nothing else (every other buffer may be NULL), the gradient
 * touches nothing.  k == 0: neg_dev and g_neg_dev may be NULL. */
int euler_gpu_skipgram_loss(void* stream, const void* target_dev, int32_t target_dtype,
                            int64_t target_rows, const void* context_dev, int32_t context_dtype,
                            int64_t context_rows, const int64_t* src_dev, const int64_t* pos_dev,
                            const int64_t* neg_dev, int64_t b, int64_t p, int64_t k, int64_t d,
                            float* logits_dev, int32_t* rank_dev, float* row_loss_dev,
                            float* loss_dev);
int euler_gpu_skipgram_loss_grad(void* stream, const void* target_dev, int32_t target_dtype,
                                 int64_t target_rows, const void* context_dev,
                                 int32_t context_dtype, int64_t context_rows,
                                 const int64_t* src_dev, const int64_t* pos_dev,
                                 const int64_t* neg_dev, int64_t b, int64_t p, int64_t k,
                                 int64_t d, const float* logits_dev, const float* g_dev,
                                 float* g_src_dev, float* g_pos_dev, float* g_neg_dev);
/* table_topk / table_rank: exact search over a whole embedding table - what a user does with a
 * trained table.  table_topk is the step of the reference's knn/knn.py:35-77 (the nearest
 * embeddings of a set of queries, returned as (distance, idx) through faiss) without an index and
 * without a [q, n] score block; table_rank is the rank behind mrr_score / mr_score / hitk_score of
 * utils/metrics.py:51-83, taken over EVERY row of the table where the reference ranks a positive
 * against sampled negatives only.
 * table_dev [n, d] and queries_dev [q, d]: fp32, bf16 or fp16, each its own type, widened exactly.
 * metric: 0 ip (sum q_c x_c, larger is better), 1 cos ((ip * inv_q) * inv_x,
 * inv = 1 / sqrt(max(sum x_c^2, 1e-12)), larger is better), 2 l2 (sum (q_c - x_c)^2, the squared
 * distance as faiss METRIC_L2 returns it, smaller is better), 3 l1 (sum |q_c - x_c|, smaller is
 * better: TransE's energy with q = h + r).  All arithmetic is correctly rounded fp32 in the
 * summation order stated in euler_amd/csrc/table_search.h: a score is a function of the two rows,
 * their types and the chunk width alone; the same call returns the same bits.
 * Row a precedes row b for a query iff its score is better, or b's is NaN and a's is not, or the
 * two compare equal (+0 == -0, any two NaNs) and a < b.
 * exclude_dev [q] int64, or NULL: a row the query neither returns nor counts (its own row when
 * the queries come from the table); a value outside [0, n) excludes nothing.
 * table_topk: rows_out [q, k] int64 = the first min(k, candidates) rows in that order,
 * scores_out [q, k] fp32 their scores; past the candidates rows = -1 and scores = -inf (ip, cos)
 * or +inf (l2, l1).
 * table_rank: rank_out [q] int32 = the number of rows r != target[q], r != exclude[q] whose score
 * is better than or EQUAL to that of row target_dev[q] (a tie goes against the target, the rule of
 * skipgram_loss's rank; a NaN score is never counted); -1 for a target outside [0, n).
 * Both enqueue two kernels and take their scratch (O(q * k * slabs), slabs <= 512 a function of n
 * and q alone) from the stream's pool: no host wait.  The outputs are written by the last kernel
 * alone.  EULER_GPU_EINVAL, checked before anything is enqueued: a metric outside 0..3, an unknown
 * dtype, d < 1, d >= 2^31, n or q outside 0 .. 2^31 - 1, k outside 1..64, a null required buffer
 * (table_dev may be NULL when n == 0), a buffer not aligned to its type.  q == 0 touches nothing
 * (every buffer may be NULL); n == 0 writes the fills (top-k) or -1 (rank). */
int euler_gpu_table_topk(void* stream, int32_t metric, const void* table_dev, int32_t table_dtype,
                         int64_t n, int64_t d, const void* queries_dev, int32_t q_dtype, int64_t q,
                         int64_t k, const int64_t* exclude_dev, float* scores_out,
                         int64_t* rows_out);
int euler_gpu_table_rank(void* stream, int32_t metric, const void* table_dev, int32_t table_dtype,
                         int64_t n, int64_t d, const void* queries_dev, int32_t q_dtype, int64_t q,
                         const int64_t* target_dev, const int64_t* exclude_dev, int32_t* rank_out);
/* neighbor_reduce: the aggregation over every queried node's STORED (full) neighbour list, read
 * straight from the graph's rows - SGCN's S^K X, APPNP's power iteration (appnp_conv.py:54-60), a
 * GCN layer over full neighbours (gcn_conv.py:33-51), the embeddings of all nodes after training -
 * in one pass: what euler_gpu_get_full_neighbor (core/graph/node.cc:175-197) followed by
 * euler_gpu_gather_segment_reduce_ids[_w]_t or euler_gpu_gather_reduce_norm_t (scatter_op.cc,
 * gather_op.cc) computes, bit for bit, without the list of the edges (16 bytes per listed edge
 * written and 12 read back), without the host wait for its total, and without the 2^31 limit on
 * that total.  euler_amd/csrc/mp_rows.h states the contract:
 *   out[i][c] = reduce over the updates p of nodes_dev[i], in the enumerated order, of
 *               fl(table[min((uint32) low word of nbr[p], table_rows - 1)][c] * w(p))
 * the updates being the entries of the row's listed edge-type groups as get_full_neighbor
 * enumerates them (groups in listed order, a type listed twice read twice, a type outside [0, T)
 * skipped, an id without a row: none).  mode 0 add (from +0), 1 max (from -1e9), 2 mean (the sum
 * divided by length + 1e-7f).  weight_kind 0: w = 1; 1: w = fl(prefix_w[p] - prefix_w[p - 1]) (0
 * for the row's first entry), the edge weight get_full_neighbor returns; 2: w = fl(norm_dst[i] *
 * norm_src[g]) for the neighbour's index g = (uint32) low word of its id, norm_src fp32
 * [table_rows], norm_dst fp32 [n]; 0 when g >= table_rows.  The product and the sum are separate
 * fp32 roundings (mp_weighted.h).  self_loop != 0 appends the table row of nodes_dev[i] itself
 * (same clamp; weight 1, or fl(norm_dst[i] * norm_src[nodes[i]]) for kind 2; counted by a mean),
 * whether or not the node has a row.  root_dev (NULL: no epilogue, root_a / root_b are not read)
 * is [n, d] in root_dtype (fp32 or table_dtype): out = fl(fl(agg * root_a) + fl(root[i] * root_b))
 * before the one rounding to out_dtype (fp32 or table_dtype).  table_dev is [table_rows, d] in
 * fp32 / bf16 / fp16, indexed by node id.  A queried node is one wave-slot's loop: a column's sum
 * is never split.  EULER_GPU_ENOGRAPH: g NULL.  EULER_GPU_EINVAL, in this order: an unknown dtype,
 * out_dtype / root_dtype neither fp32 nor table_dtype; mode; weight_kind; a negative n, d or k;
 * (n == 0 or d == 0 returns EULER_GPU_OK and touches nothing;) a null buffer; k > 32; table_rows
 * outside [1, 2^31); n >= 2^31; norm tables not exactly with weight_kind 2; a buffer not aligned
 * to its type.  All of it is host arithmetic in front of the first HIP call.
 * neighbor_degree: out_dev[i] = the listed degree of nodes_dev[i] (what get_full_neighbor's
 * offsets differ by; + 1 with self_loop; INT32_MAX past it) as int32 (as_norm == 0) or as
 * 1 / sqrt((float)deg) in fp32, 0 at degree 0 (euler_gpu_gcn_norm's rule).  No host wait. */
int euler_gpu_neighbor_reduce(const euler_gpu_graph* g, void* stream, int32_t mode,
                              const uint64_t* nodes_dev, int64_t n, const int32_t* edge_types_host,
                              int32_t k, int32_t weight_kind, int32_t self_loop, const void* table_dev,
                              int32_t table_dtype, int64_t table_rows, int64_t d,
                              const float* norm_dst_dev, const float* norm_src_dev, const void* root_dev,
                              int32_t root_dtype, float root_a, float root_b, void* out_dev,
                              int32_t out_dtype);
int euler_gpu_neighbor_degree(const euler_gpu_graph* g, void* stream, const uint64_t* nodes_dev,
                              int64_t n, const int32_t* edge_types_host, int32_t k, int32_t self_loop,
                              int32_t as_norm, void* out_dev);
/* supervise_loss: the loss head of the supervised models (GraphSAGE, GCN, GAT, ... and the graph
 * classifiers: SuperviseModel.__call__ after out_fc, tf_euler/python/mp_utils/base.py:24-47,
 * SuperviseSolution of solution/base_supervise.py, GraphModel of mp_utils/base_graph.py:24-47,
 * with f1_score / acc_score / auc_score of utils/metrics.py:29-48) in ONE read of the logits and
 * the labels: p = sigmoid(x), sigmoid_cross_entropy_with_logits(z, x) (soft labels allowed), its
 * mean, the prediction floor(p + 0.5), the streaming counts tp / fp / fn / correct / total and the
 * two histograms behind tf.metrics.auc.  The contract is stated in euler_amd/csrc/supervise.h.
 * logits_dev [b, c]: fp32, bf16 or fp16, widened exactly.  The labels come in ONE of two forms:
 * labels_dev [b, c] (fp32, bf16 or fp16; graph and nodes_dev NULL), or the graph form (labels_dev
 * NULL): nodes_dev [b] and the float feature slot fid of `graph`, read straight from the graph's
 * feature table as euler_gpu_get_dense_feature_t reads it (an unknown node or slot: zeros; a
 * slot shorter than c: zero filled; a longer one: truncated; a 16-bit table: widened) - no [b, c]
 * label block exists.
 * prob_dev [b, c] fp32 (may be NULL): p.  diff_dev [b, c] fp32 (may be NULL): p - z, what the
 * gradient needs.  row_loss_dev [b]: the terms of a row added in the order 0 .. c - 1.  loss_dev
 * [1]: the row sums reduced in the fixed order of skipgram_loss, a function of b alone, divided
 * once by float(b * c).  These are WRITTEN.  counts_dev [5] int64 (tp, fp, fn, correct, total)
 * and hist_dev [2][thresholds + 1] int64 (may be NULL; row 0: label != 0, row 1: label == 0; bucket
 * = the number of thresholds of tf.metrics.auc's table strictly below p) are ADDED TO - they
 * stream across calls - with integer atomics only: the same bits on every run, and no float
 * atomic anywhere.
 * supervise_loss_grad: from diff_dev and the scalar g_dev [1] (the gradient of the loss)
 * g_logits_dev [b, c] = (g / float(b * c)) * diff, rounded once to logits_dtype.
 * Both only enqueue (the forward two kernels): no allocation, no host wait; both can be captured
 * into a graph.  EULER_GPU_EINVAL, checked before anything is enqueued, so every output is
 * written entirely or not at all: an unknown dtype, b < 0, c < 1, b * c >= 2^31, thresholds < 2
 * with hist_dev given, both label forms or neither, a null required buffer, a buffer not aligned
 * to its element type.  b == 0: the forward writes loss_dev = +0 and touches nothing else (every
 * buffer but loss_dev and counts_dev may be NULL, the labels of both forms included), the gradient
 * touches nothing.  NaN logits are
 * outside the contract. */
int euler_gpu_supervise_loss(void* stream, const void* logits_dev, int32_t logits_dtype, int64_t b,
                             int64_t c, const void* labels_dev, int32_t labels_dtype,
                             const euler_gpu_graph* graph, const uint64_t* nodes_dev, int32_t fid,
                             int32_t thresholds, float* prob_dev, float* diff_dev,
                             float* row_loss_dev, float* loss_dev, int64_t* counts_dev,
                             int64_t* hist_dev);
int euler_gpu_supervise_loss_grad(void* stream, const float* diff_dev, const float* g_dev, int64_t b,
                                  int64_t c, void* g_logits_dev, int32_t logits_dtype);
/* store_update / store_add / store_take: the in-place embedding stores of ScalableSage /
 * ScalableGCN (tf_euler/python/utils/embedding.py:24-68, encoders.py:713-748) - tf.scatter_update,
 * tf.scatter_add and embedding_lookup with the optional clearing update of encoders.py:738-743 -
 * on a table [rows, d] (fp32 / bf16 / fp16, contiguous) that is MODIFIED IN PLACE; no [rows, d]
 * temporary and no [e, d] block of per-occurrence rows exists.  The contract is stated in
 * euler_amd/csrc/embed_store.h.  ids_dev: signed int64 [e], the row index is the id; an id outside
 * [0, rows) names no row: it is never dereferenced, is left out of update / add and reads as a
 * row of +0 in take.  The source row of occurrence p is values[p] (row_index_dev == NULL and
 * count == 0; m must equal e), values[row_index_dev[p]] (int32 [e]; an entry outside [0, m) removes
 * the occurrence) or values[p / count] (count > 0, e % count == 0, m == e / count).  values_dev is
 * [m, d], fp32 or the table's dtype (narrowing: one round to nearest even).
 * update: table[id] = the source row of the LAST occurrence of id (same dtype: the bits).
 * add: acc = widen(table[id]); acc = fl32(acc + widen(source row)) for the occurrences of id in
 * increasing p; table[id] = round(acc) - no float atomics, the same bits on every call and for
 * every launch geometry.
 * take: out_dev [e, d] (the table's dtype or fp32) receives table[ids[p]] as it was before the
 * call for every occurrence; clear != 0 leaves every row an in-range id names at +0.
 * All three only enqueue: no host wait, no device-to-host copy; scratch is stream-ordered and
 * every check precedes the first write, so an error leaves the table untouched.
 * EULER_GPU_EINVAL: an unknown dtype, a values / out dtype that is neither fp32 nor the table's,
 * rows < 1, e or d >= 2^31 (or < 0), row_index and count both given, count < 0, count > 0 with
 * e % count != 0 or m != e / count, the plain form with m != e, a null required buffer, a buffer
 * not aligned to its element type.  e == 0 or d == 0 returns EULER_GPU_OK and touches nothing. */
int euler_gpu_store_update(void* stream, void* table_dev, int32_t table_dtype, int64_t rows,
                           int64_t d, const int64_t* ids_dev, int64_t e, const void* values_dev,
                           int32_t values_dtype, int64_t m, const int32_t* row_index_dev,
                           int64_t count);
int euler_gpu_store_add(void* stream, void* table_dev, int32_t table_dtype, int64_t rows,
                        int64_t d, const int64_t* ids_dev, int64_t e, const void* values_dev,
                        int32_t values_dtype, int64_t m, const int32_t* row_index_dev,
                        int64_t count);
int euler_gpu_store_take(void* stream, void* table_dev, int32_t table_dtype, int64_t rows,
                         int64_t d, const int64_t* ids_dev, int64_t e, int32_t clear,
                         void* out_dev, int32_t out_dtype);
/* sparse_optim_step: ONE optimiser step - kind 0 sgd, 1 momentum, 2 adagrad, 3 adam, the four of
 * the reference's tf_euler/python/utils/optimizers.py - on the rows of table_dev [rows, d] (fp32 /
 * bf16 / fp16, contiguous) that ids_dev names, IN PLACE, from the gradient rows of the
 * occurrences: no coalesce, no [distinct, d] temporary, no float atomics.  The contract, every
 * formula included, is stated in euler_amd/csrc/sparse_optim.h.
 * state0_dev / state1_dev: fp32 [rows, d], contiguous, modified in place - sgd: both NULL;
 * momentum: the accumulator, NULL; adagrad: the sum of squares, NULL; adam: exp_avg, exp_avg_sq.
 * ids_dev, grad_dev / grad_dtype / m, row_index_dev and count are values_dev & co. of store_add:
 * an id outside [0, rows) names no row, the gradient row of occurrence p is grad[p],
 * grad[row_index_dev[p]] or grad[p / count], grad is fp32 or the table's dtype.  Per distinct
 * live id and column: g = the sum of its occurrences in increasing p (fp32, one rounding per add,
 * starting from the first occurrence), then the step in correctly rounded fp32 operations, then
 * ONE rounding to the table's dtype.  The same call gives the same bits, for every launch
 * geometry.  The scalars are fp32 values the caller computed in double and rounded once: lr, mu
 * (momentum), eps, om1 = 1 - beta1, om2 = 1 - beta2, step_size = lr * sqrt(1 - beta2^t) /
 * (1 - beta1^t); those the kind does not use are ignored but checked.  Rows no live id names keep
 * their bits in the table and the state.
 * Only enqueues (three launches): no host wait; scratch is stream-ordered and released on every
 * exit; every check precedes the first write, so an error leaves the table and the state
 * untouched.  EULER_GPU_EINVAL: an unknown kind or dtype, a grad dtype that is neither fp32 nor
 * the table's, a scalar that is negative or not finite, a state pointer missing for the kind or
 * given where the kind has none, rows < 1, e or d >= 2^31 (or < 0), the count / row_index / m
 * rules of store_add, a null required buffer, a buffer not aligned to its element type.  e == 0
 * or d == 0 returns EULER_GPU_OK and touches nothing. */
int euler_gpu_sparse_optim_step(void* stream, int32_t kind, void* table_dev, int32_t table_dtype,
                                int64_t rows, int64_t d, float* state0_dev, float* state1_dev,
                                const int64_t* ids_dev, int64_t e, const void* grad_dev,
                                int32_t grad_dtype, int64_t m, const int32_t* row_index_dev,
                                int64_t count, float lr, float mu, float eps, float om1, float om2,
                                float step_size);
/* gather_segment_topk: the step of the reference's LGCEncoder (LGCN,
 * tf_euler/python/utils/encoders.py:911-914: get_dense_feature, reshape [B, nb, d], transpose,
 * tf.nn.top_k, transpose) in one pass - for every destination r and every column c the k largest
 * values among the rows its segment gathers, in descending order, without the [e, d] block.  The
 * rules are stated in euler_amd/csrc/mp_topk.h:
 * Segment of r: seg_ptr_dev[r] .. seg_ptr_dev[r + 1] (int64 [size + 1]), or r * count ..
 * (r + 1) * count (seg_ptr_dev NULL, count > 0, e == size * count); exactly one of the two.
 * Candidate of position p and column c: params[g[p]][c] widened exactly to fp32, g = gather_dev:
 * int32 [e] (gather_is_ids == 0), signed int64 ids [e] (gather_is_ids != 0, compared in 64 bits)
 * or NULL (g[p] = p).  An index outside [0, params_rows) names no row: it is never dereferenced,
 * reads as a row of +0 and DOES take part as a candidate (a default_node fill's feature row is
 * zeros in the reference); its gradient is dropped.
 * Order: a precedes b iff a > b, or a is NaN and b is not (NaN greatest, as torch.topk); otherwise
 * the earlier position precedes (stable); +0 == -0, NaN == NaN.
 * out_dev [size, k, d] (fp32 or in_dtype): out[r][j][c] = the j-th candidate in that order for
 * j < min(k, len) - the bits of the table element for every non-NaN, a NaN for a NaN -, `fill`
 * rounded once to out_dtype for j >= len.  sel_dev [size, k, d] int32 (NULL: not wanted): that
 * candidate's position p, -1 for j >= len.
 * segment_topk_grad: per_edge_dev [e, d] fp32 is +0 everywhere except
 * per_edge[sel[r][j][c]][c] = grad[r][j][c] (grad_dev [size, k, d], fp32 / bf16 / fp16, widened)
 * for sel >= 0 - one writer per element at most, no atomics; positions outside every segment stay
 * +0.  The table gradient is the scatter_add of per_edge by g, indices outside the table left out.
 * Both only enqueue on `stream`: no allocation, no host wait, no LDS, no atomics.
 * EULER_GPU_EINVAL: k outside 1..16, an unknown dtype, out_dtype neither fp32 nor in_dtype, both
 * or neither of seg_ptr_dev / count, the count form with e != size * count, e or d >= 2^31 (or a
 * negative extent), a null required buffer, params_rows < 1, a buffer not aligned to its element
 * type; every check precedes the first write.  size == 0 or d == 0 (grad: e == 0 or d == 0)
 * returns EULER_GPU_OK and touches nothing. */
int euler_gpu_gather_segment_topk(void* stream, const void* params_dev, int32_t in_dtype,
                                  int64_t params_rows, const void* gather_dev,
                                  int32_t gather_is_ids, const int64_t* seg_ptr_dev, int64_t count,
                                  int64_t e, int64_t d, int32_t size, int32_t k, float fill,
                                  void* out_dev, int32_t out_dtype, int32_t* sel_dev);
int euler_gpu_segment_topk_grad(void* stream, const void* grad_dev, int32_t grad_dtype,
                                const int32_t* sel_dev, int64_t e, int64_t d, int32_t size,
                                int32_t k, float* per_edge_dev);

/* ---- shard ops (multi-GPU) --------------------------------------------------
 * ID_SPLIT (core/kernels/id_split_op.cc:46-99): stable bucket of ids by
 * owner(id) = (id % partitions) % shards.  shard_off_host [shards+1] is
 * returned after a stream sync; shard_ids_dev / merge_idx_dev have n entries.
 * euler_gpu_merge_rows is IDX_MERGE/DATA_MERGE (idx_merge_op.cc:61-77,
 * data_merge_op.cc:44-67) for fixed-size rows: out[merge_idx[j]] = in[j]. */
int euler_gpu_id_split(void* stream, const uint64_t* ids_dev, int64_t n,
                       int32_t partitions, int32_t shards,
                       int64_t* shard_off_host, uint64_t* shard_ids_dev,
                       int32_t* merge_idx_dev);
/* InflateIdx (tf_euler/kernels/inflate_idx_op.cc:34-66, op InflateIdx of tf_euler/ops/util_ops.cc):
 * idx_dev holds n values that are exactly 0 .. U-1 for some U; out_dev[i] = the place of entry
 * i after a stable sort by value (entries with a smaller value + equal entries before i).
 * EULER_GPU_EINVAL when a value lies outside [0, number of distinct values) - the reference's
 * InvalidArgument; out_dev is then unspecified.  Synchronizes the stream (the check). */
int euler_gpu_inflate_idx(void* stream, const int32_t* idx_dev, int64_t n, int32_t* out_dev);
/* Split sizes between the ranks of one node without the GPU: an all-to-all of
 * up to 8 int64 per peer through a POSIX shared-memory mailbox.  Replaces what
 * the reference carries inside its per-shard gRPC requests / replies
 * (core/kernels/remote_op.cc:62-142); RCCL needs both sides' counts on the host
 * before the data moves.  One rank creates the region (create = 1, the name is
 * new), the others open it afterwards; every rank then calls
 * euler_shm_alltoall_i64 in the same order (send / recv: [world * width], peer
 * p's message at p * width).  timeout_ms <= 0 means 60 s. */
typedef struct euler_shm euler_shm;
int euler_shm_open(const char* name, int32_t rank, int32_t world, int32_t create,
                   euler_shm** out);
int euler_shm_alltoall_i64(euler_shm* s, const int64_t* send, int64_t* recv,
                           int32_t width, int64_t timeout_ms);
int32_t euler_shm_attached(const euler_shm* s);
int euler_shm_unlink(euler_shm* s);
void euler_shm_close(euler_shm* s);

/* Front end of a multi-GPU hop in one call: the DISTINCT ids of the batch
 * (ID_UNIQUE, which the reference's optimizer puts before ID_SPLIT:
 * parser/compiler.cc:76-90) bucketed by owner into shard_ids_dev (<= n entries,
 * shard s at [shard_off_host[s], shard_off_host[s+1])), and pos_dev[i] = index
 * in shard_ids_dev of ids_dev[i].  The shards answer in the order they were
 * asked, so row pos_dev[i] of the concatenated answers is position i's row:
 * euler_gpu_expand_rows finishes the hop (IDX_MERGE / DATA_MERGE / DATA_GATHER
 * in one pass).  An id may occur more than once in shard_ids_dev (hash-slot
 * collisions are not resolved); results are unaffected.  Synchronises once.
 * dense_owner_dev (optional): scratch of dense_limit + 1 uint32 the caller keeps
 * between calls (contents irrelevant) when every id of the graph is below
 * dense_limit (euler_gpu_graph_id_range): duplicates are then found with one
 * store and one load per id in a table indexed by the id itself instead of two
 * rounds of hashing; ids >= dense_limit are "no such node" and share one
 * representative (every owner answers the default row for them).
 * root_mask_dev (optional, [ceil(n / root_group)] bytes) has the meaning it has
 * in euler_gpu_sample_neighbor: marked groups sample as node id 0. */
int euler_gpu_dedup_split(void* stream, const uint64_t* ids_dev, int64_t n,
                          const uint8_t* root_mask_dev, int32_t root_group,
                          int32_t partitions, int32_t shards, uint32_t* dense_owner_dev,
                          int64_t dense_limit, int64_t* shard_off_host,
                          uint64_t* shard_ids_dev, int32_t* pos_dev);
/* The same call in two halves, for callers that keep several minibatches in
 * flight from one host thread: _begin enqueues everything (the bucket sizes end
 * in a pinned buffer of the handle, an event marks their arrival) and returns;
 * _end waits for that event only and hands out shard_off_host [shards + 1].  One
 * call in flight per handle; shard_ids_dev / pos_dev are valid in stream order
 * after _begin. */
typedef struct euler_gpu_front euler_gpu_front;
int euler_gpu_front_create(euler_gpu_front** out);
void euler_gpu_front_destroy(euler_gpu_front* f);
int euler_gpu_dedup_split_begin(euler_gpu_front* f, void* stream, const uint64_t* ids_dev,
                                int64_t n, const uint8_t* root_mask_dev, int32_t root_group,
                                int32_t partitions, int32_t shards,
                                uint32_t* dense_owner_dev, int64_t dense_limit,
                                uint64_t* shard_ids_dev, int32_t* pos_dev);
int euler_gpu_dedup_split_end(euler_gpu_front* f, int64_t* shard_off_host);
/* Wire format of the result exchange: one int32 row per root = [ids (2 words
 * each) | weights | types | mask | pad], 4 * count + 2 words; with ONE listed
 * edge type (single_type >= 0) the type column stays off the wire - 3 * count +
 * 2 words, padded to an even number (rows stay 8-byte aligned) - and is rebuilt on arrival (single_type, or -1 for a masked row).
 * pack_rows writes the rows from the sampler's outputs [m, count] (+ row mask
 * [m]); expand_packed reads the concatenated answers back per position through
 * pos_dev (merge + gather + unpack in one pass).  single_type = -1: full rows. */
int euler_gpu_pack_rows(void* stream, const uint64_t* id_dev, const float* w_dev,
                        const int32_t* t_dev, const uint8_t* mask_dev, int64_t m,
                        int32_t count, int32_t single_type, int32_t* packed_dev);
int euler_gpu_expand_packed(void* stream, const int32_t* pos_dev, int64_t n,
                            int32_t count, int32_t single_type, const int32_t* packed_dev,
                            uint64_t* out_id_dev, float* out_w_dev, int32_t* out_t_dev,
                            uint8_t* out_mask_dev);
/* out row i = row pos_dev[i] of (row_id, row_w, row_t [m, count], row_mask [m]). */
int euler_gpu_expand_rows(void* stream, const int32_t* pos_dev, int64_t n,
                          int32_t count, const uint64_t* row_id_dev,
                          const float* row_w_dev, const int32_t* row_t_dev,
                          const uint8_t* row_mask_dev, uint64_t* out_id_dev,
                          float* out_w_dev, int32_t* out_t_dev, uint8_t* out_mask_dev);
int euler_gpu_merge_rows(void* stream, const void* in_dev,
                         const int32_t* merge_idx_dev, int64_t n_rows,
                         int64_t row_bytes, void* out_dev);
/* ---- multi-GPU hop for C / C++ hosts ------------------------------------------
 * What ID_SPLIT -> REMOTE -> IDX_MERGE / DATA_MERGE does over gRPC in the
 * reference (core/kernels/id_split_op.cc:46-99, remote_op.cc:60-142,
 * idx_merge_op.cc:32-78, data_merge_op.cc:44-67), as ONE call per rank: every
 * rank (one process per GPU, holding the shard owner(id) = (id % partitions) %
 * world == rank) calls it with its own batch, and the calls exchange ids and wire
 * rows through `tr`.  The result equals the unsharded euler_gpu_sample_neighbor /
 * euler_gpu_sample_fanout (TF layout) bit for bit.  All ranks must make the same
 * sequence of calls (also a rank whose batch is empty: n = 0).
 *
 * The transport is two callbacks over one opaque pointer:
 *   alltoall_counts  host-side all-to-all of one int64 per peer (send[p] = rows this
 *                    rank will send to p -> recv[p] = rows it gets from p);
 *   alltoallv        all-to-all(v) of DEVICE rows of row_bytes each, enqueued on
 *                    `stream` (send_rows / recv_rows per peer, buffers packed in
 *                    peer order).
 * euler_gpu_transport_rccl fills it for an ncclComm_t (ncclSend / ncclRecv groups
 * over xGMI; the RCCL the host process already loaded is resolved at run time, this
 * library does not link it); `counts` = an euler_shm mailbox the ranks opened, or
 * NULL = the counts travel through the communicator (a device sync per hop).
 *
 * Memory: the per-call scratch of the euler_gpu_sharded_* entries (bucketed ids, wire rows, a
 * walk's levels, the rows a node2vec step fetches) comes from blocks the library keeps per
 * (device, stream) once it has allocated them - at most 32 GB per process, beyond that a
 * released block goes back to the driver.  (Stream-ordered allocations of gigabyte blocks of
 * ever different sizes stalled for seconds once in a few hundred calls.) */
typedef struct euler_gpu_transport {
  int32_t rank, world;
  void* user;
  int (*alltoall_counts)(void* user, const int64_t* send, int64_t* recv);
  int (*alltoallv)(void* user, const void* send_dev, const int64_t* send_rows,
                   void* recv_dev, const int64_t* recv_rows, int64_t row_bytes,
                   void* stream);
} euler_gpu_transport;
int euler_gpu_transport_rccl(void* nccl_comm, int32_t rank, int32_t world,
                             euler_shm* counts, euler_gpu_transport* out);
void euler_gpu_transport_rccl_release(euler_gpu_transport* t);
/* One hop; arguments as euler_gpu_sample_neighbor (TF layout), out_mask_dev [n]
 * optional. */
int euler_gpu_sharded_sample_neighbor(const euler_gpu_graph* shard,
                                      const euler_gpu_transport* tr, void* stream,
                                      uint64_t seed, uint32_t call_id,
                                      const uint64_t* roots_dev, int64_t n,
                                      const uint8_t* root_mask_dev, int32_t root_group,
                                      const int32_t* edge_types_host, int32_t k,
                                      int32_t count, int64_t default_node,
                                      int32_t partitions, uint64_t* out_id_dev,
                                      float* out_w_dev, int32_t* out_t_dev,
                                      uint8_t* out_mask_dev);
/* The fanout; arguments as euler_gpu_sample_fanout (workspace_dev:
 * euler_gpu_sample_fanout_workspace bytes). */
int euler_gpu_sharded_sample_fanout(const euler_gpu_graph* shard,
                                    const euler_gpu_transport* tr, void* stream,
                                    uint64_t seed, uint32_t call_id,
                                    const uint64_t* roots_dev, int64_t n,
                                    const int32_t* edge_types_host, int32_t k,
                                    const int32_t* counts_host, int32_t layers,
                                    int64_t default_node, int32_t partitions,
                                    uint64_t* const* out_id_dev, float* const* out_w_dev,
                                    int32_t* const* out_t_dev, void* workspace_dev);

/* TF RandomWalk with p = q = 1 over the sharded graph
 * (tf_euler/kernels/random_walk_op.cc:207-247: one sampleNB(edge_types, 1) query per step,
 * each ID_UNIQUE -> ID_SPLIT -> REMOTE -> MERGE -> GATHER): starts_dev [n] int64 ->
 * out_dev [n, walk_len + 1] int64 (missing neighbour -> default_node), bit-identical to
 * euler_gpu_random_walk on the unsharded graph.  The walk runs over LEVELS of distinct nodes
 * (walkers that meet stay together: the draw is keyed by the node), one front end + id
 * exchange + owners' draw + answer exchange per step, the walkers' paths written once at
 * the end.  The whole walk is ENQUEUED (round 6): a level and its per-owner buckets live in
 * slabs of a fixed stride (the largest walker count of a rank + 1, rounded up to 2 048 words:
 * a header word = the entries behind it, the entries, padding), their sizes stay on the device,
 * every message has the slab's size - so the host exchanges ONE number per peer per CALL (the
 * ranks' walker counts, through tr->alltoall_counts) and then only enqueues: per step the
 * front end (mark + one kernel that ranks and places; from step 16 on the level is sent as it
 * is), tr->alltoallv of world equal messages, the owners' draw over the slabs received, the
 * answers back into the next level.  The wire carries world x stride words per exchange
 * instead of the level's distinct nodes.  euler_gpu_set_tuning(63, 0) (euler_gpu_measure.h)
 * keeps the polled form: exchanges sized from the bucket sizes, one host wait per step and
 * cohort.  cohorts (1..16, the same on every rank): the walkers are split into that many
 * independent walks whose steps alternate on `stream` (the polled form hides its waits with
 * them; the enqueued form has none to hide).  dense_owner_dev / dense_limit: the id-indexed
 * table of euler_gpu_dedup_split (NULL / 0 = hashing).  stats_host (optional, int64[4]):
 * host waits, level entries summed over the steps, ids sent to other ranks, cohorts - asking
 * for them makes the enqueued call wait for the stream once at its end (the sizes never
 * reached the host otherwise).  All ranks must call it together (also with n = 0). */
int euler_gpu_sharded_random_walk(const euler_gpu_graph* shard, const euler_gpu_transport* tr,
                                  void* stream, uint64_t seed, uint32_t call_id,
                                  const int64_t* starts_dev, int64_t n,
                                  const int32_t* edge_types_host, int32_t k, int32_t walk_len,
                                  int64_t default_node, int32_t partitions, int32_t cohorts,
                                  uint32_t* dense_owner_dev, int64_t dense_limit,
                                  int64_t* out_dev, int64_t* stats_host);

/* TF RandomWalk with p or q != 1 (node2vec) over the sharded graph, as the reference's client
 * runs it (tf_euler/kernels/random_walk_op.cc:83-168: per step one `v(nodes).outV(edge_types)`
 * query for the walkers' current nodes - ID_UNIQUE -> ID_SPLIT -> REMOTE -> MERGE, one row per
 * distinct node - the previous step's rows kept as the parents', BuildWeights and the draw on
 * the client): starts_dev [n] int64 -> out_dev [n, walk_len + 1] int64, bit-identical to
 * euler_gpu_random_walk(p, q) on the unsharded graph (the draw of step s is keyed by the
 * walker's index and call_id + s).  Per step and rank: front end (distinct nodes by owner) ->
 * ids to the owners -> their full rows (euler_gpu_get_full_neighbor) -> row lengths, ids and
 * weights back (all-to-all(v)s sized from the lengths) -> euler_gpu_node2vec_step on the
 * fetched rows.  The host waits three times per step (bucket sizes, the owners' row offsets,
 * the value counts per peer).  stats_host (optional, int64[4]): host waits, rows asked, row
 * entries received (summed over the steps), ids sent to other ranks.  All ranks call it
 * together (also with n = 0). */
int euler_gpu_sharded_node2vec_walk(const euler_gpu_graph* shard, const euler_gpu_transport* tr,
                                    void* stream, uint64_t seed, uint32_t call_id,
                                    const int64_t* starts_dev, int64_t n,
                                    const int32_t* edge_types_host, int32_t k, int32_t walk_len,
                                    float p, float q, int64_t default_node, int32_t partitions,
                                    uint32_t* dense_owner_dev, int64_t dense_limit,
                                    int64_t* out_dev, int64_t* stats_host);

/* SAMPLE_NODE_SPLIT (core/kernels/sample_node_split_op.cc:57-85), host only:
 * shard_weight_host[shards+1] (last = total) -> split_cnt_host[shards]. */
int euler_gpu_sample_node_split(uint64_t seed, uint32_t call_id, int32_t count,
                                const float* shard_weight_host, int32_t shards,
                                int32_t* split_cnt_host);

/* ---- index memory ------------------------------------------------------------
 * The weight-bucket index (csrc/wb_index.h) is built on the first sampling / walk / block call
 * of a graph with non-uniform, non-decreasing running sums: 128 bytes per 4 edges of rows
 * with more than 10 edges + 8 + 8 T bytes per row (about 40 GB for 100M nodes / 1B edges; a graph
 * it serves does not get the 13 bytes per edge of EdgeBlocks the pivot-level search needs - those
 * are built, also on first use, only for graphs without a serving index).  It is an
 * optimisation that is DECLINED - the pivot-level search then serves, same results - when
 * it would take more than `max_free_fraction` of the HBM that is free at that moment
 * (default 0.5) or more than `max_bytes` (default: no absolute cap; 0 = never build it),
 * or when anything fails while it is built.  Process-wide; affects graphs whose index has
 * not been built yet.  Negative arguments leave a value unchanged.  The environment sets
 * the defaults: EULER_GPU_WB_INDEX=0, EULER_GPU_WB_INDEX_MAX_GB, EULER_GPU_WB_INDEX_MAX_FRACTION. */
int euler_gpu_set_index_budget(int64_t max_bytes, double max_free_fraction);

/* The 2-hop fanout of single listed types in the (unique rows, index) form - the GQL result
 * before DATA_GATHER (core/kernels/data_gather_op.cc:33-80; ID_UNIQUE: id_unique_op.cc:35-64):
 * hop 1 dense ([n, counts[0]] as euler_gpu_sample_fanout), hop 2 as DISTINCT rows:
 * rows_{id,w,t}_dev are [n * counts[0], counts[1]] row slots, row_index_dev [n * counts[0]]
 * (uint32) names the row of every hop-1 sample - the dense hop-2 tensors are
 * rows[row_index].  Roots are processed in groups of 4 (tuning key 28); a group fills the
 * first D of its 4 * counts[0] row slots, D = the distinct children it drew, the rest stay
 * untouched.  Plain graphs only (one edge-type group per node, identity id map, no neighbour
 * id 0, counts[1] even): EULER_GPU_EINVAL otherwise.  workspace: as euler_gpu_sample_fanout. */
int euler_gpu_sample_fanout_unique(const euler_gpu_graph* g, void* stream, uint64_t seed,
                                   uint32_t call_id, const uint64_t* roots_dev, int64_t n,
                                   const int32_t* edge_types_host, const int32_t* counts_host,
                                   int64_t default_node, uint64_t* out_id1_dev, float* out_w1_dev,
                                   int32_t* out_t1_dev, uint32_t* row_index_dev,
                                   uint64_t* rows_id_dev, float* rows_w_dev, int32_t* rows_t_dev,
                                   void* workspace_dev);
/* TF SampleFanoutWithFeature (tf_euler/kernels/sample_fanout_with_feature_op.cc:135-233;
 * op tf_euler/ops/neighbor_ops.cc:282-321): euler_gpu_sample_fanout plus the dense
 * features of every layer's nodes (layer 0 = the roots), enqueued back to back on `stream`
 * - no host round trip.  dense_out_dev[(layer) * n_dense + j] is a [m_layer, dims[j]]
 * float32 buffer (m_0 = n, m_{l+1} = m_l * counts[l]); zero rows for default_node,
 * unknown nodes and missing slots.  (The sparse features of the op need their sizes on
 * the host: euler_gpu_get_sparse_feature per layer, euler_amd/euler_ops/neighbor_ops.py.) */
int euler_gpu_sample_fanout_with_feature(const euler_gpu_graph* g, void* stream, uint64_t seed,
                                         uint32_t call_id, const uint64_t* roots_dev, int64_t n,
                                         const int32_t* edge_types_host, int32_t k,
                                         const int32_t* counts_host, int32_t layers,
                                         int64_t default_node, uint64_t* const* out_id_dev,
                                         float* const* out_w_dev, int32_t* const* out_t_dev,
                                         void* workspace_dev, const int32_t* dense_fids_host,
                                         const int32_t* dense_dims_host, int32_t n_dense,
                                         float* const* dense_out_dev);

/* ---- edge records (edge_kernels.hip) ------------------------------------------
 * The reference keeps one Edge object per record in an unordered_map<EdgeID, Edge*>
 * (core/graph/graph.h:87-104).  Here an edge store: 32-byte slots {src, dst, type, weight,
 * ordinal} in an open-addressing table of 128-byte lines (4 slots, at most half full, linear
 * probing by line), an ordinal -> slot map, the per-type alias tables of the edge sampler and
 * the edge features in the ragged layout of the node features.  No store exists until one of
 * the three constructors runs; a constructor replaces the graph's store.  Every byte is counted
 * in euler_gpu_graph_bytes, and a failed build returns its allocations. */
/* The records of a dataset: Edge/<x>_<partition>.dat as euler_gpu_dat_open_edges reads them. */
int euler_gpu_graph_load_edges(euler_gpu_graph* g, const char* data_path, int32_t shard_index,
                               int32_t shards);
/* Host records in ordinal order; (src, dst, type) must be distinct (EULER_GPU_EINVAL). */
int euler_gpu_graph_set_edges(euler_gpu_graph* g, const euler_gpu_host_edges* edges);
/* One record per distinct (src, dst, type) entry of the graph's rows, built on the device:
 * ordinals in row order, then entry order, first occurrence kept; the weight is the entry's
 * own (running sum minus the one before it in the row).  No features. */
int euler_gpu_graph_edges_from_rows(euler_gpu_graph* g);
int64_t euler_gpu_graph_num_edge_records(const euler_gpu_graph* g);   /* -1: no store */
/* The store's feature tables replaced by those of *edges (edges->n == the record count, rows in
 * ordinal order; the record arrays are not read) - features for a store edges_from_rows built. */
int euler_gpu_graph_set_edge_features(euler_gpu_graph* g, const euler_gpu_host_edges* edges);
/* Records [first, first + n) in ordinal order to host arrays (any may be NULL). */
int euler_gpu_graph_export_edges(const euler_gpu_graph* g, int64_t first, int64_t n,
                                 uint64_t* src_host, uint64_t* dst_host, int32_t* type_host,
                                 float* weight_host);
/* The edge sampler (Graph::BuildGlobalEdgeSampler, core/graph/graph.cc:372-405) rebuilt over the
 * records in the order `order_host` lists their ordinals (a permutation of 0..n-1; NULL =
 * ordinal order, what every constructor builds).  The reference enumerates its unordered_map. */
int euler_gpu_graph_set_edge_sampler(euler_gpu_graph* g, const int64_t* order_host);
/* API_SAMPLE_EDGE / Graph::SampleEdge (core/graph/graph.cc:277-326, core/kernels/
 * sample_edge_op.cc:32-78): out_dev [count, 3] int64 (src, dst, type).  The draws are exactly
 * euler_gpu_sample_node's (same domain, stream and draw indices).  edge_types_host[k]: one type,
 * {-1} = all types, or a list; the reference's -1 / list path never initialises its type
 * collection - here they draw a type by edge_weight_sums_ as SampleNode does.
 * A zero weight sum: EULER_GPU_EEMPTY, nothing written. */
int euler_gpu_sample_edge(const euler_gpu_graph* g, void* stream, uint64_t seed, uint32_t call_id,
                          const int32_t* edge_types_host, int32_t k, int32_t count,
                          int64_t* out_dev);
/* Graph::GetEdgeByID (core/graph/graph.h:94-104): edges_dev [n, 3] int64 (src, dst, type) ->
 * ordinals [n] int64, -1 where there is no such record. */
int euler_gpu_edge_ordinals(const euler_gpu_graph* g, void* stream, const int64_t* edges_dev,
                            int64_t n, int64_t* out_dev);
/* TF GetEdgeDenseFeature (tf_euler/kernels/get_edge_dense_feature_op.cc): [n, dim] float32,
 * zero-filled, truncated to dim; zeros for an unknown edge or slot. */
int euler_gpu_get_edge_dense_feature(const euler_gpu_graph* g, void* stream,
                                     const int64_t* edges_dev, int64_t n, int32_t fid,
                                     int32_t dim, float* out_dev);
/* TF GetEdgeSparseFeature (tf_euler/kernels/get_edge_sparse_feature_op.cc): the COO triple and
 * two-call protocol of euler_gpu_get_sparse_feature; an empty or unknown edge contributes
 * (row, 0) = default_value. */
int euler_gpu_get_edge_sparse_feature(const euler_gpu_graph* g, void* stream,
                                      const int64_t* edges_dev, int64_t n, int32_t fid,
                                      int64_t default_value, int64_t* row_off_dev,
                                      int64_t* nnz_host, int64_t* max_len_host,
                                      int64_t* indices_dev, int64_t* values_dev);
/* TF GetEdgeBinaryFeature (tf_euler/kernels/get_edge_binary_feature_op.cc:90-115): the bytes of
 * slot fid of every edge, concatenated: call 1 (bytes_dev NULL) fills offsets_dev [n+1] int64 and
 * *total_host; call 2 the bytes.  An unknown edge or slot is empty. */
int euler_gpu_get_edge_binary_feature(const euler_gpu_graph* g, void* stream,
                                      const int64_t* edges_dev, int64_t n, int32_t fid,
                                      int64_t* offsets_dev, int64_t* total_host,
                                      uint8_t* bytes_dev);
/* TF GetBinaryFeature (tf_euler/kernels/get_binary_feature_op.cc) over the node rows, the same
 * two calls.  The node binary features of a loaded dataset reach the device on the first call. */
int euler_gpu_get_binary_feature(const euler_gpu_graph* g, void* stream, const uint64_t* nodes_dev,
                                 int64_t n, int32_t fid, int64_t* offsets_dev, int64_t* total_host,
                                 uint8_t* bytes_dev);

/* ---- graph labels --------------------------------------------
 * Graph::GetGraphLabel's index (core/graph/graph.cc:439-457): label -> the nodes that carry it.
 * A loaded dataset's labels are the node binary feature binary_graph_label (euler.meta); the
 * index is built on the device on the first label call.  Table order: by the smallest node id
 * of a label; nodes of a label: ascending ids (Q14).  An empty value is no label (Q15).  A graph
 * without labels answers EULER_GPU_EEMPTY; a sharded graph (shards > 1) EULER_GPU_EINVAL.
 *
 * Labels by node id for a graph not read from .dat (replaces the binary_graph_label feature the
 * reference's converter writes, tf_euler/python/dataset/multigraph_util.py:68-90): label i is
 * bytes_host[offsets_host[i] .. offsets_host[i + 1]).  An id without a row, or an id listed
 * twice, is EULER_GPU_EINVAL and the old index stays intact. */
int euler_gpu_graph_set_graph_labels(euler_gpu_graph* g, const uint64_t* ids_host, int64_t n,
                                     const int64_t* offsets_host, const uint8_t* bytes_host);
/* The number of labels (0 when the graph has none, < 0 an error code). */
int64_t euler_gpu_graph_num_graph_labels(const euler_gpu_graph* g);
/* The label table in table order: offsets_host [labels + 1]; bytes_host [offsets_host[labels]]
 * (NULL: offsets only - the usual two calls). */
int euler_gpu_graph_export_graph_labels(const euler_gpu_graph* g, int64_t* offsets_host,
                                        uint8_t* bytes_host);
/* Label strings -> table ids (-1 for an unknown label), on the host. */
int euler_gpu_graph_label_ids(const euler_gpu_graph* g, int64_t n, const int64_t* offsets_host,
                              const uint8_t* bytes_host, int64_t* out_host);
/* The index's size: labelled nodes and the device bytes it holds. */
int euler_gpu_graph_label_index_info(const euler_gpu_graph* g, int64_t* n_labelled_host,
                                     int64_t* index_bytes_host);
/* API_SAMPLE_GRAPH_LABEL (core/kernels/sample_graph_label_op.cc:32-66): `count` label ids drawn
 * uniformly with replacement, RNG domain 7, stream 0: draw j is sample j, label =
 * min(floor(u * L), L - 1).  out_dev [count] int64. */
int euler_gpu_sample_graph_label(const euler_gpu_graph* g, void* stream, uint64_t seed,
                                 uint32_t call_id, int32_t count, int64_t* out_dev);
/* API_GET_GRAPH_BY_LABEL (core/kernels/get_graph_by_label_op.cc:32-75) on label ids: two calls
 * like euler_gpu_get_full_neighbor - out_dev NULL fills idx_dev [n, 2] int32 (start, end) and
 * *total_host (synchronises the stream); the second call writes the node ids.  A negative or
 * unknown id gives an empty range. */
int euler_gpu_get_graph_by_label(const euler_gpu_graph* g, void* stream, const int64_t* label_ids_dev,
                                 int64_t n, int32_t* idx_dev, int64_t* total_host, uint64_t* out_dev);
/* The whole-graph block of WholeDataFlow (tf_euler/python/dataflow/whole_dataflow.py:37-63): for
 * nodes_dev [n] (any order, duplicates and unknown ids allowed), every (j, c) such that nodes[c]
 * is an out-neighbour of nodes[j] by one of the k listed edge types, sorted by j then c; then the
 * self loops (i, i) when add_self_loops.  out_dev is int64 [2, cap]: sources in row 0, targets in
 * row 1.  *total_host = edges + loops; when that exceeds cap nothing is written and the caller
 * asks again with room (one call when the capacity suffices).  A neighbour listed twice (two
 * edge types, a repeated edge) gives one pair.  Costs O(n + listed edges); reads three sizes on
 * the host per call (listed edges, hits, block edges).  Synchronises the stream. */
int euler_gpu_whole_graph_block(const euler_gpu_graph* g, void* stream, const uint64_t* nodes_dev,
                                int64_t n, const int32_t* edge_types_host, int32_t k,
                                int32_t add_self_loops, int64_t cap, int64_t* total_host,
                                int64_t* out_dev);

/* Tuning keys, phase timers and byte counters (A/B measurements, bench.py's roofline leg) are
 * not part of the product surface: include/euler_gpu_measure.h. */

#ifdef __cplusplus
}
#endif
#endif  /* EULER_GPU_H_ */
