// Edge records on the device for gfx950: the edge store (records, (src, dst, type) -> ordinal
// lookup, edge sampler, edge features), its three constructors, and the kernels of
// Graph::SampleEdge (core/graph/graph.cc:277-326), Graph::GetEdgeByID (core/graph/graph.h:
// 94-104) and the TF edge / binary feature ops (tf_euler/kernels/get_edge_*_feature_op.cc,
// get_binary_feature_op.cc) with their C-ABI entry points.
//
// Store layout (common.h: EdgeStoreView), per record: 64 bytes of 32-byte slots (4 to a
// 128-byte line, at most half used), a 32-byte alias entry whose ids are slot positions and an
// 8-byte ordinal -> slot map: 104 bytes, features not counted.  A lookup hashes the triple to a
// line and reads it with 8 lanes (one 16-byte load each, ONE request per line - beyond the ~2 GiB
// the address-translation caches reach every lane-request to a line pays its own translation,
// DESIGN §4.2); the feature row of the ordinal is the next line.  A draw of the sampler reads
// its alias entry and then the slot it names: two lines.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <numeric>
#include <vector>

#include "device_mem.h"
#include "node_sampler.h"

namespace euler_gpu {

namespace {

constexpr int kGroup = 8;          // lanes per lookup: 8 x 16 bytes = one line

__device__ __forceinline__ uint64_t EdgeLine(uint64_t n_lines, uint64_t src, uint64_t dst,
                                             int32_t type) {
  const uint64_t h = Mix64(src ^ Mix64(dst ^ ((uint64_t)(uint32_t)type << 40)));
  return __umul64hi(h, n_lines);   // [0, n_lines) without a power-of-two table
}

__device__ __forceinline__ uint64_t RowIdOf(const GraphView& v, int64_t row) {
  return v.row_id ? v.row_id[row] : v.id_base + v.id_stride * (uint64_t)row;
}

// The 8 lanes of a group look up one triple; every lane of the group gets the ordinal (-1: no
// such record).  Lane j of the group loads bytes [16 j, 16 j + 16) of the line: even lanes hold
// a slot's {src, dst}, odd lanes its {type, weight, ordinal}.  A line with an empty slot ends the
// probe (records are inserted into the first free slot of their probe sequence).
__device__ __forceinline__ int64_t GroupFind(const EdgeStoreView& s, uint64_t src, uint64_t dst,
                                             int32_t type, int sub) {
  const int base = (int)(threadIdx.x & 63) & ~(kGroup - 1);
  uint64_t line = EdgeLine(s.n_lines, src, dst, type);
  for (uint64_t p = 0; p < s.n_lines; ++p) {
    const uint4 q = reinterpret_cast<const uint4*>(s.slots + 4 * line)[sub];
    const uint64_t lo = (uint64_t)q.x | ((uint64_t)q.y << 32);
    const uint64_t hi = (uint64_t)q.z | ((uint64_t)q.w << 32);
    const int keys = (sub & 1) == 0 && lo == src && hi == dst;
    const int pair_keys = __shfl_xor(keys, 1, kGroup);
    const bool odd = (sub & 1) != 0;
    const bool used = odd && (int64_t)hi >= 0;
    const bool hit = used && pair_keys && (int32_t)q.x == type;
    const uint64_t hm = (__ballot(hit) >> base) & 0xffu;
    if (hm) return (int64_t)__shfl((long long)hi, base + __ffsll((long long)hm) - 1);
    const uint64_t em = (__ballot(odd && !used) >> base) & 0xffu;
    if (em) return -1;
    line = line + 1 == s.n_lines ? 0 : line + 1;
  }
  return -1;
}

// Values of slot `fid` of record `rec` (GET_EDGE_FEATURE / GET_NODE_FEATURE): none for an
// unknown record or slot.
__device__ __forceinline__ int32_t SlotRange(const FeatTable& t, int64_t rec, int32_t fid,
                                             int64_t* first) {
  *first = 0;
  if (rec < 0 || fid < 0 || fid >= t.n_slots) return 0;
  const int32_t* idx = t.uniform ? t.idx : t.idx + rec * (int64_t)t.n_slots;
  const int32_t pre = fid == 0 ? 0 : idx[fid - 1];
  *first = (t.uniform ? rec * t.stride : t.ptr[rec]) + pre;
  return idx[fid] - pre;
}

struct EdgeQuery {
  EdgeStoreView s;
  const int64_t* edges;   // [n, 3] (src, dst, type)
  int64_t n;
  int32_t fid;
  int32_t dim;
};

// Groups stride over the queried edges; the loop condition is the same in a group's lanes.
#define EDGE_GROUP_LOOP(q, i, sub)                                                          \
  const int sub = (int)(threadIdx.x & (kGroup - 1));                                       \
  const int64_t n_groups = ((int64_t)gridDim.x * blockDim.x) / kGroup;                     \
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; i < (q).n;   \
       i += n_groups)

__device__ __forceinline__ int64_t QueryOrdinal(const EdgeQuery& q, int64_t i, int sub) {
  const int64_t* e = q.edges + 3 * i;
  return GroupFind(q.s, (uint64_t)e[0], (uint64_t)e[1], (int32_t)e[2], sub);
}

__global__ __launch_bounds__(256) void EdgeOrdinalKernel(const EdgeQuery q, int64_t* out) {
  EDGE_GROUP_LOOP(q, i, sub) {
    const int64_t ord = QueryOrdinal(q, i, sub);
    if (sub == 0) out[i] = ord;
  }
}

// Lookup fused with the dense fetch: the group writes the [dim] row, zeros past the slot's values.
__global__ __launch_bounds__(256) void EdgeDenseKernel(const EdgeQuery q, float* out) {
  EDGE_GROUP_LOOP(q, i, sub) {
    const int64_t ord = QueryOrdinal(q, i, sub);
    int64_t first;
    const int32_t len = SlotRange(q.s.f32, ord, q.fid, &first);
    const float* v = static_cast<const float*>(q.s.f32.val) + first;
    float* o = out + i * (int64_t)q.dim;
    for (int32_t k = sub; k < q.dim; k += kGroup) o[k] = k < len ? v[k] : 0.f;
  }
}

// counts[i]: values of the slot (sparse: at least 1, the default entry); max_len: their maximum.
__global__ __launch_bounds__(256) void EdgeCountKernel(const EdgeQuery q, const FeatTable t,
                                                       int32_t at_least, int64_t* counts,
                                                       unsigned long long* max_len) {
  int32_t local_max = 0;
  EDGE_GROUP_LOOP(q, i, sub) {
    const int64_t ord = QueryOrdinal(q, i, sub);
    int64_t first;
    const int32_t len = max(SlotRange(t, ord, q.fid, &first), at_least);
    if (sub == 0) counts[i] = len;
    local_max = max(local_max, len);
  }
  // one atomic per wave (one per item serialises on the one address: 1.5 ms per 1M items)
  if (max_len == nullptr) return;
  for (int off = 32; off > 0; off >>= 1) local_max = max(local_max, __shfl_xor(local_max, off));
  if ((threadIdx.x & 63) == 0 && local_max > 0) atomicMax(max_len, (unsigned long long)local_max);
}

__global__ __launch_bounds__(256) void EdgeSparseFillKernel(const EdgeQuery q, const int64_t* off,
                                                            int64_t default_value,
                                                            int64_t* indices, int64_t* values) {
  EDGE_GROUP_LOOP(q, i, sub) {
    const int64_t ord = QueryOrdinal(q, i, sub);
    int64_t first;
    const int32_t len = SlotRange(q.s.u64, ord, q.fid, &first);
    const uint64_t* v = static_cast<const uint64_t*>(q.s.u64.val) + first;
    const int64_t o = off[i];
    if (len < 1) {
      if (sub == 0) {
        indices[2 * o] = i;
        indices[2 * o + 1] = 0;
        values[o] = default_value;
      }
      continue;
    }
    for (int32_t k = sub; k < len; k += kGroup) {
      indices[2 * (o + k)] = i;
      indices[2 * (o + k) + 1] = k;
      values[o + k] = (int64_t)v[k];
    }
  }
}

__global__ __launch_bounds__(256) void EdgeBinaryFillKernel(const EdgeQuery q, const int64_t* off,
                                                            uint8_t* bytes) {
  EDGE_GROUP_LOOP(q, i, sub) {
    const int64_t ord = QueryOrdinal(q, i, sub);
    int64_t first;
    const int32_t len = SlotRange(q.s.bin, ord, q.fid, &first);
    const uint8_t* v = static_cast<const uint8_t*>(q.s.bin.val) + first;
    for (int32_t k = sub; k < len; k += kGroup) bytes[off[i] + k] = v[k];
  }
}

// Binary features of node rows: one lane per node counts, one wave per node copies.
__global__ __launch_bounds__(256) void NodeBinaryCountKernel(const GraphView g, const FeatTable t,
                                                             const uint64_t* nodes, int64_t n,
                                                             int32_t fid, int64_t* counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int64_t first;
    counts[i] = SlotRange(t, FindRow(g, nodes[i]), fid, &first);
  }
}

__global__ __launch_bounds__(256) void NodeBinaryFillKernel(const GraphView g, const FeatTable t,
                                                            const uint64_t* nodes, int64_t n,
                                                            int32_t fid, const int64_t* off,
                                                            uint8_t* bytes) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += n_waves) {
    int64_t first;
    const int32_t len = SlotRange(t, FindRow(g, nodes[i]), fid, &first);
    const uint8_t* v = static_cast<const uint8_t*>(t.val) + first;
    for (int32_t k = lane; k < len; k += 64) bytes[off[i] + k] = v[k];
  }
}

// SampleEdge: SampleNode's draw over alias entries whose ids are slot positions, then the slot.
__global__ __launch_bounds__(256) void SampleEdgeKernel(const SampleNodeArgs a,
                                                        const EdgeSlot* slots, int64_t* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride) {
    const EdgeSlot& e = slots[SampleNodeDraw(a, i)];
    const ulonglong2 k = *reinterpret_cast<const ulonglong2*>(&e.src);
    out[3 * i] = (int64_t)k.x;
    out[3 * i + 1] = (int64_t)k.y;
    out[3 * i + 2] = e.type;
  }
}

// ---- construction
// Record i claims the first free slot of its probe sequence (the ordinal field is the claim).
__global__ void InsertRecordsKernel(EdgeSlot* slots, uint64_t n_lines, const uint64_t* src,
                                    const uint64_t* dst, const int32_t* type, const float* weight,
                                    int64_t n, int64_t* slot_of) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uint64_t line = EdgeLine(n_lines, src[i], dst[i], type[i]);
    for (uint64_t p = 0; p < n_lines; ++p) {
      int64_t at = -1;
      for (int j = 0; j < 4 && at < 0; ++j) {
        EdgeSlot* sl = slots + 4 * line + j;
        if (atomicCAS(reinterpret_cast<unsigned long long*>(&sl->ord), ~0ull,
                      (unsigned long long)i) == ~0ull)
          at = (int64_t)(4 * line + j);
      }
      if (at >= 0) {
        EdgeSlot* sl = slots + at;
        sl->src = src[i]; sl->dst = dst[i]; sl->type = type[i]; sl->weight = weight[i];
        slot_of[i] = at;
        break;
      }
      line = line + 1 == n_lines ? 0 : line + 1;
    }
  }
}

// After the inserts: a record that a lookup of its own triple does not find is a repeat.
__global__ __launch_bounds__(256) void CheckDistinctKernel(const EdgeStoreView s, const uint64_t* src,
                                                           const uint64_t* dst, const int32_t* type,
                                                           int64_t n, int32_t* repeats) {
  const int sub = (int)(threadIdx.x & (kGroup - 1));
  const int64_t n_groups = ((int64_t)gridDim.x * blockDim.x) / kGroup;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; i < n; i += n_groups) {
    const int64_t ord = GroupFind(s, src[i], dst[i], type[i], sub);
    if (sub == 0 && ord != i) atomicAdd(repeats, 1);
  }
}

// edges_from_rows, pass 1: one lane per row inserts the row's entries in entry order with
// ordinal = the entry's global index.  A repeat of (src, dst, type) can only come from the same
// row and type segment, i.e. from this lane: a slot claimed by an entry of the segment is
// compared (this lane wrote it), any other claimed slot is passed by.
__global__ void RowsInsertKernel(const GraphView v, EdgeSlot* slots, uint64_t n_lines,
                                 int64_t* first) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < v.n_rows; r += stride) {
    const uint64_t src = RowIdOf(v, r);
    const RowMeta m = LoadRowMeta(v, r);
    for (int32_t t = 0; t < v.T; ++t) {
      const int64_t b = m.row_ptr + (t == 0 ? 0 : m.type_end[t - 1]);
      const int64_t e = m.row_ptr + m.type_end[t];
      for (int64_t ent = b; ent < e; ++ent) {
        const uint64_t dst = v.nbr[ent];
        uint64_t line = EdgeLine(n_lines, src, dst, t);
        bool placed = false, repeat = false;
        for (uint64_t p = 0; p < n_lines && !placed && !repeat; ++p) {
          for (int j = 0; j < 4 && !placed && !repeat; ++j) {
            EdgeSlot* sl = slots + 4 * line + j;
            const int64_t old = (int64_t)atomicCAS(reinterpret_cast<unsigned long long*>(&sl->ord),
                                                   ~0ull, (unsigned long long)ent);
            if (old == -1) {
              sl->src = src; sl->dst = dst; sl->type = t;
              sl->weight = __fsub_rn(v.prefix_w[ent], ent == m.row_ptr ? 0.f : v.prefix_w[ent - 1]);
              placed = true;
            } else if (old >= b && old < ent) {
              repeat = sl->dst == dst;
            }
          }
          line = line + 1 == n_lines ? 0 : line + 1;
        }
        first[ent] = placed ? 1 : 0;
      }
    }
  }
}

// pass 2: the claimed slots' records at their ordinals (exclusive scan of the first-occurrence
// flags of the entries)
__global__ void RowsRecordsKernel(const EdgeSlot* slots, uint64_t n_slots, const int64_t* ord_of_entry,
                                  uint64_t* src, uint64_t* dst, int32_t* type, float* weight) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < (int64_t)n_slots; s += stride) {
    const EdgeSlot e = slots[s];
    if (e.ord < 0) continue;
    const int64_t o = ord_of_entry[e.ord];
    src[o] = e.src; dst[o] = e.dst; type[o] = e.type; weight[o] = e.weight;
  }
}

// Records [first, first + n) in ordinal order (any output may be null).
__global__ void GatherRecordsKernel(const EdgeStoreView s, int64_t first, int64_t n, uint64_t* src,
                                    uint64_t* dst, int32_t* type, float* weight, int64_t* slot) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t at = s.slot_of[first + i];
    const EdgeSlot& e = s.slots[at];
    if (src) src[i] = e.src;
    if (dst) dst[i] = e.dst;
    if (type) type[i] = e.type;
    if (weight) weight[i] = e.weight;
    if (slot) slot[i] = at;
  }
}

// ---- host side
// (the allocations of one store build are an AllocList: returned on failure, handed to the graph
// on success; temporaries of a build, not part of the store, are DevBufs)

// A host feature table -> device.  uniform: every record has record 0's slot ends and its
// values start at r * (record 0's length): one row of ends, no offsets.
template <typename V>
FeatTable UploadTable(AllocList* a, int64_t n, int32_t slots, const int64_t* ptr,
                      const int32_t* idx, const V* val) {
  FeatTable t{};
  if (slots <= 0 || n <= 0 || !ptr || !idx) return t;
  t.n_slots = slots;
  const int64_t len0 = ptr[1] - ptr[0];
  bool uniform = ptr[0] == 0;
  for (int64_t r = 0; r < n && uniform; ++r) {
    uniform = ptr[r] == r * len0 &&
              std::memcmp(idx + r * slots, idx, (size_t)slots * sizeof(int32_t)) == 0;
  }
  t.uniform = uniform ? 1 : 0;
  t.stride = uniform ? len0 : 0;
  t.ptr = uniform ? nullptr : a->Upload(ptr, (size_t)n + 1);
  t.idx = a->Upload(idx, uniform ? (size_t)slots : (size_t)(n * slots));
  t.val = a->Upload(val, (size_t)ptr[n]);
  return t;
}

// The edge sampler over the store's records, enumerated in `order` (null = ordinal order).
int BuildEdgeSampler(const EdgeStoreView& s, int32_t n_types, const int64_t* order,
                     AllocList* a, NodeSamplerView* view, std::vector<float>* sums) {
  const int64_t n = s.n;
  std::vector<uint64_t> ids((size_t)n);
  std::vector<int32_t> types((size_t)n);
  std::vector<float> weights((size_t)n);
  {
    DevBuf tmp;
    EG_HIP(tmp.alloc((size_t)std::max<int64_t>(n, 1) * 16));
    int64_t* slot = tmp.as<int64_t>();
    int32_t* ty = reinterpret_cast<int32_t*>(slot + n);
    float* w = reinterpret_cast<float*>(ty + n);
    hipLaunchKernelGGL(GatherRecordsKernel, dim3(GridFor(n, 256)), dim3(256), 0, 0, s, 0, n,
                       nullptr, nullptr, ty, w, slot);
    int rc = CheckLaunch("edge sampler: gather");
    if (rc != EULER_GPU_OK) return rc;
    EG_HIP(hipMemcpy(ids.data(), slot, (size_t)n * 8, hipMemcpyDeviceToHost));
    EG_HIP(hipMemcpy(types.data(), ty, (size_t)n * 4, hipMemcpyDeviceToHost));
    EG_HIP(hipMemcpy(weights.data(), w, (size_t)n * 4, hipMemcpyDeviceToHost));
  }
  if (order) {
    std::vector<char> seen((size_t)n, 0);
    std::vector<uint64_t> ids2((size_t)n);
    std::vector<int32_t> types2((size_t)n);
    std::vector<float> weights2((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t o = order[i];
      if (o < 0 || o >= n || seen[(size_t)o])
        return Fail(EULER_GPU_EINVAL, "set_edge_sampler: order is not a permutation of the ordinals");
      seen[(size_t)o] = 1;
      ids2[(size_t)i] = ids[(size_t)o]; types2[(size_t)i] = types[(size_t)o];
      weights2[(size_t)i] = weights[(size_t)o];
    }
    ids.swap(ids2); types.swap(types2); weights.swap(weights2);
  }
  std::vector<AliasEntry> entries;
  const int rc = BuildAliasTables(ids, types, weights, n_types, view, &entries, sums, "edge");
  if (rc != EULER_GPU_OK) return rc;
  view->entries = a->Upload(entries.data(), entries.size());
  return view->entries ? EULER_GPU_OK : a->rc;
}

// Installs a built store (its allocations and sampler) in place of the graph's.
void InstallStore(euler_gpu_graph* g, const EdgeStoreView& s, AllocList* a,
                  const NodeSamplerView& sampler, std::vector<float>* sums) {
  DestroyEdgeStore(g);
  g->edges = s;
  g->has_edges = true;
  // the sampler's table is the last allocation of the build; kept apart so that
  // set_edge_sampler can replace it alone
  g->edge_sampler_alloc = a->list.back();
  a->list.pop_back();
  g->edge_allocs.swap(a->list);
  for (auto& p : g->edge_allocs) g->bytes += p.second;
  g->bytes += g->edge_sampler_alloc.second;
  g->edge_sampler = sampler;
  g->edge_weight_sums.swap(*sums);
}

int NumTypes(const std::vector<int32_t>& type, int32_t declared, int32_t* out) {
  int32_t T = std::max<int32_t>(declared, 1);
  for (int32_t t : type) {
    if (t < 0 || t >= kMaxNodeTypes) return Fail(EULER_GPU_EINVAL, "edge store: edge type out of 0..31");
    T = std::max(T, t + 1);
  }
  *out = T;
  return EULER_GPU_OK;
}

// The store over n records in ordinal order, given as DEVICE arrays; features from the host
// description `e` (may be null: none).
int BuildStore(euler_gpu_graph* g, int64_t n, int32_t T, const uint64_t* src, const uint64_t* dst,
               const int32_t* ty, const float* w, const euler_gpu_host_edges* e) {
  AllocList a("edge store: ");
  EdgeStoreView s{};
  s.n = n;
  s.n_lines = (uint64_t)std::max<int64_t>((n + 1) / 2, 1);
  EdgeSlot* slots = a.Alloc<EdgeSlot>((size_t)(4 * s.n_lines));
  int64_t* slot_of = slots ? a.Alloc<int64_t>((size_t)n) : nullptr;
  if (slot_of) {
    s.slots = slots; s.slot_of = slot_of;
    DevBuf tmp;
    hipError_t he = hipMemset(slots, 0xff, (size_t)(4 * s.n_lines) * sizeof(EdgeSlot));
    if (he == hipSuccess) he = tmp.alloc(16);
    if (he == hipSuccess) he = hipMemset(tmp.as(), 0, 16);
    if (he != hipSuccess) {
      a.rc = Fail(EULER_GPU_EHIP, std::string("edge store: ") + hipGetErrorString(he));
    } else {
      int32_t* repeats = tmp.as<int32_t>();
      hipLaunchKernelGGL(InsertRecordsKernel, dim3(GridFor(n, 256)), dim3(256), 0, 0, slots,
                         s.n_lines, src, dst, ty, w, n, slot_of);
      a.rc = CheckLaunch("edge store: insert");
      if (a.rc == EULER_GPU_OK) {
        hipLaunchKernelGGL(CheckDistinctKernel, dim3(GridFor(n * kGroup, 256)), dim3(256), 0, 0,
                           s, src, dst, ty, n, repeats);
        a.rc = CheckLaunch("edge store: check");
      }
      int32_t rep = 0;
      if (a.rc == EULER_GPU_OK &&
          hipMemcpy(&rep, repeats, 4, hipMemcpyDeviceToHost) == hipSuccess && rep > 0)
        a.rc = Fail(EULER_GPU_EINVAL, "set_edges: " + std::to_string(rep) +
                                          " records repeat an earlier (src, dst, type)");
    }
  }
  if (e && a.rc == EULER_GPU_OK)
    s.f32 = UploadTable(&a, n, e->n_float_features, e->feat_ptr, e->feat_idx, e->feat_val);
  if (e && a.rc == EULER_GPU_OK)
    s.u64 = UploadTable(&a, n, e->n_u64_features, e->ufeat_ptr, e->ufeat_idx, e->ufeat_val);
  if (e && a.rc == EULER_GPU_OK)
    s.bin = UploadTable(&a, n, e->n_binary_features, e->bfeat_ptr, e->bfeat_idx, e->bfeat_val);
  NodeSamplerView sampler{};
  std::vector<float> sums;
  if (a.rc == EULER_GPU_OK) a.rc = BuildEdgeSampler(s, T, nullptr, &a, &sampler, &sums);
  if (a.rc != EULER_GPU_OK) {
    a.Release();
    return a.rc;
  }
  InstallStore(g, s, &a, sampler, &sums);
  return EULER_GPU_OK;
}

int BuildFromHost(euler_gpu_graph* g, const euler_gpu_host_edges* e) {
  const int64_t n = e->n;
  if (n <= 0 || !e->src || !e->dst || !e->type || !e->weight)
    return Fail(EULER_GPU_EINVAL, "set_edges: need n > 0 records with src, dst, type and weight");
  if (e->n_float_features < 0 || e->n_u64_features < 0 || e->n_binary_features < 0)
    return Fail(EULER_GPU_EINVAL, "set_edges: negative feature slot count");
  int32_t T = 0;
  int rc = NumTypes(std::vector<int32_t>(e->type, e->type + n), e->n_edge_types, &T);
  if (rc != EULER_GPU_OK) return rc;
  DeviceGuard dg(g->device);
  DevBuf tmp;
  EG_HIP(tmp.alloc((size_t)n * 24));
  uint64_t* src = tmp.as<uint64_t>();
  uint64_t* dst = src + n;
  int32_t* ty = reinterpret_cast<int32_t*>(dst + n);
  float* w = reinterpret_cast<float*>(ty + n);
  EG_HIP(hipMemcpy(src, e->src, (size_t)n * 8, hipMemcpyHostToDevice));
  EG_HIP(hipMemcpy(dst, e->dst, (size_t)n * 8, hipMemcpyHostToDevice));
  EG_HIP(hipMemcpy(ty, e->type, (size_t)n * 4, hipMemcpyHostToDevice));
  EG_HIP(hipMemcpy(w, e->weight, (size_t)n * 4, hipMemcpyHostToDevice));
  return BuildStore(g, n, T, src, dst, ty, w, e);
}

// First occurrences of the rows' (src, dst, type) entries through a scratch table sized for every
// entry, then the store over them (sized for the records that remain).
int BuildFromRows(euler_gpu_graph* g) {
  const GraphView& v = g->view;
  const int64_t E = v.n_edges;
  if (E <= 0) return Fail(EULER_GPU_EINVAL, "edges_from_rows: the graph has no edges");
  if (v.T > kMaxNodeTypes) return Fail(EULER_GPU_EINVAL, "edges_from_rows: more than 32 edge types");
  DeviceGuard dg(g->device);
  const uint64_t n_lines = (uint64_t)std::max<int64_t>((E + 1) / 2, 1);
  DevBuf table, flags;
  EG_HIP(table.alloc((size_t)(4 * n_lines) * sizeof(EdgeSlot)));
  EG_HIP(hipMemset(table.as(), 0xff, (size_t)(4 * n_lines) * sizeof(EdgeSlot)));
  EG_HIP(flags.alloc((size_t)(2 * E + 2) * 8));
  EdgeSlot* slots = table.as<EdgeSlot>();
  int64_t* first = flags.as<int64_t>();
  int64_t* ord = first + E + 1;
  EG_HIP(hipMemset(first + E, 0, 8));
  hipLaunchKernelGGL(RowsInsertKernel, dim3(GridFor(v.n_rows, 64)), dim3(64), 0, 0, v, slots,
                     n_lines, first);
  int rc = CheckLaunch("edges_from_rows: insert");
  if (rc == EULER_GPU_OK) rc = ExclusiveScanI64(0, first, ord, E + 1);
  if (rc != EULER_GPU_OK) return rc;
  int64_t n = 0;
  EG_HIP(hipMemcpy(&n, ord + E, 8, hipMemcpyDeviceToHost));
  DevBuf recs;
  EG_HIP(recs.alloc((size_t)n * 24 + 16));
  uint64_t* src = recs.as<uint64_t>();
  uint64_t* dst = src + n;
  int32_t* ty = reinterpret_cast<int32_t*>(dst + n);
  float* w = reinterpret_cast<float*>(ty + n);
  hipLaunchKernelGGL(RowsRecordsKernel, dim3(GridFor((int64_t)(4 * n_lines), 256)), dim3(256), 0, 0,
                     slots, 4 * n_lines, ord, src, dst, ty, w);
  rc = CheckLaunch("edges_from_rows: records");
  if (rc != EULER_GPU_OK) return rc;
  table.reset();     // (returned before the store takes its own blocks)
  flags.reset();
  return BuildStore(g, n, std::max<int32_t>(v.T, 1), src, dst, ty, w, nullptr);
}

}  // namespace

int EnsureNodeBinary(const euler_gpu_graph* g) {
  std::lock_guard<std::mutex> lk(g->bin_mu);
  if (g->node_bin_ready || g->bin_host_slots == 0) return EULER_GPU_OK;
  DeviceGuard dg(g->device);
  AllocList a("edge store: ");
  const int64_t n = (int64_t)g->bin_host_ptr.size() - 1;
  const FeatTable t = UploadTable(&a, n, g->bin_host_slots, g->bin_host_ptr.data(),
                                  g->bin_host_idx.data(), g->bin_host_val.data());
  if (a.rc != EULER_GPU_OK) { a.Release(); return a.rc; }
  euler_gpu_graph* mg = const_cast<euler_gpu_graph*>(g);   // the upload is the graph's from now on
  mg->bytes += a.HandOver(&mg->allocations);
  g->node_bin = t;
  g->node_bin_ready = true;
  return EULER_GPU_OK;
}

namespace {

int CheckEdgeQuery(const euler_gpu_graph* g, const char* what, int64_t n, const void* edges) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, std::string(what) + ": null graph");
  if (!g->has_edges)
    return Fail(EULER_GPU_ENOGRAPH, std::string(what) + ": the graph has no edge records "
                                    "(load_edges / set_edges / edges_from_rows)");
  if (n < 0) return Fail(EULER_GPU_EINVAL, std::string(what) + ": n < 0");
  if (n > 0 && !edges) return Fail(EULER_GPU_EINVAL, std::string(what) + ": null edges");
  return EULER_GPU_OK;
}

// The two calls of a ragged result: (1) counts -> offsets [n+1] (+ total, max) on the host,
// (2) the fill.  `count` launches the count kernel into counts [n] (max into counts[n + 1]).
// Stream-ordered scratch freed on every exit.
template <typename CountFn>
int RaggedOffsets(hipStream_t st, int64_t n, CountFn count, int64_t* off_dev, int64_t* total_host,
                  int64_t* max_host) {
  StreamBuf scratch(st);
  EG_HIP(scratch.alloc((size_t)(n + 2) * sizeof(int64_t)));
  int64_t* counts = scratch.as<int64_t>();
  EG_HIP(hipMemsetAsync(counts + n, 0, 2 * sizeof(int64_t), st));
  count(counts, reinterpret_cast<unsigned long long*>(counts + n + 1));
  const int rc = ExclusiveScanI64(st, counts, off_dev, n + 1);
  if (rc != EULER_GPU_OK) return rc;
  int64_t total = 0, mx = 0;
  EG_HIP(hipMemcpyAsync(&total, off_dev + n, 8, hipMemcpyDeviceToHost, st));
  EG_HIP(hipMemcpyAsync(&mx, counts + n + 1, 8, hipMemcpyDeviceToHost, st));
  EG_HIP(hipStreamSynchronize(st));
  if (total_host) *total_host = total;
  if (max_host) *max_host = mx;
  return EULER_GPU_OK;
}

EdgeQuery MakeQuery(const euler_gpu_graph* g, const int64_t* edges, int64_t n, int32_t fid,
                    int32_t dim) {
  EdgeQuery q{};
  q.s = g->edges; q.edges = edges; q.n = n; q.fid = fid; q.dim = dim;
  return q;
}

}  // namespace

void DestroyEdgeStore(euler_gpu_graph* g) {
  g->bytes -= FreeBlocks(&g->edge_allocs);
  if (g->edge_sampler_alloc.first) {
    (void)hipFree(g->edge_sampler_alloc.first);   // owned by the graph, kept apart from the list
    g->bytes -= g->edge_sampler_alloc.second;
  }
  g->edge_sampler_alloc = {nullptr, 0};
  g->edges = EdgeStoreView{};
  g->edge_sampler = NodeSamplerView{};
  g->has_edges = false;
  g->edge_weight_sums.clear();
}

}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_graph_load_edges(euler_gpu_graph* g, const char* data_path, int32_t shard_index,
                               int32_t shards) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "load_edges: null graph");
  if (!data_path) return Fail(EULER_GPU_EINVAL, "load_edges: null path");
  DatEdges d;
  int rc = LoadDatEdges(data_path, shard_index, shards, &d);
  if (rc != EULER_GPU_OK) return rc;
  if (d.src.empty()) return Fail(EULER_GPU_EIO, "load_edges: no edge records");
  euler_gpu_host_edges e{};
  d.Describe(&e);
  return BuildFromHost(g, &e);
}

int euler_gpu_graph_set_edges(euler_gpu_graph* g, const euler_gpu_host_edges* edges) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "set_edges: null graph");
  if (!edges) return Fail(EULER_GPU_EINVAL, "set_edges: null records");
  return BuildFromHost(g, edges);
}

int euler_gpu_graph_edges_from_rows(euler_gpu_graph* g) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "edges_from_rows: null graph");
  return BuildFromRows(g);
}

int64_t euler_gpu_graph_num_edge_records(const euler_gpu_graph* g) {
  return g && g->has_edges ? g->edges.n : -1;
}

int euler_gpu_graph_set_edge_features(euler_gpu_graph* g, const euler_gpu_host_edges* edges) {
  int rc = CheckEdgeQuery(g, "set_edge_features", 0, nullptr);
  if (rc != EULER_GPU_OK) return rc;
  const euler_gpu_host_edges* e = edges;
  if (!e || e->n != g->edges.n || e->n_float_features < 0 || e->n_u64_features < 0 ||
      e->n_binary_features < 0)
    return Fail(EULER_GPU_EINVAL, "set_edge_features: need the store's record count of feature rows");
  DeviceGuard dg(g->device);
  AllocList a("edge store: ");
  const int64_t n = e->n;
  const FeatTable f32 = UploadTable(&a, n, e->n_float_features, e->feat_ptr, e->feat_idx, e->feat_val);
  const FeatTable u64 = a.rc == EULER_GPU_OK
      ? UploadTable(&a, n, e->n_u64_features, e->ufeat_ptr, e->ufeat_idx, e->ufeat_val) : FeatTable{};
  const FeatTable bin = a.rc == EULER_GPU_OK
      ? UploadTable(&a, n, e->n_binary_features, e->bfeat_ptr, e->bfeat_idx, e->bfeat_val) : FeatTable{};
  if (a.rc != EULER_GPU_OK) { a.Release(); return a.rc; }
  (void)hipDeviceSynchronize();          // (no launch may still read the old tables)
  for (const FeatTable* t : {&g->edges.f32, &g->edges.u64, &g->edges.bin}) {
    for (const void* p : {(const void*)t->ptr, (const void*)t->idx, t->val}) {
      auto it = std::find_if(g->edge_allocs.begin(), g->edge_allocs.end(),
                             [p](const std::pair<void*, int64_t>& x) { return p && x.first == p; });
      if (it == g->edge_allocs.end()) continue;
      (void)hipFree(it->first);            // a replaced table leaves the store's list
      g->bytes -= it->second;
      g->edge_allocs.erase(it);
    }
  }
  g->bytes += a.HandOver(&g->edge_allocs);
  g->edges.f32 = f32; g->edges.u64 = u64; g->edges.bin = bin;
  return EULER_GPU_OK;
}

int euler_gpu_graph_export_edges(const euler_gpu_graph* g, int64_t first, int64_t n,
                                 uint64_t* src_host, uint64_t* dst_host, int32_t* type_host,
                                 float* weight_host) {
  int rc = CheckEdgeQuery(g, "export_edges", 0, nullptr);
  if (rc != EULER_GPU_OK) return rc;
  if (first < 0 || n < 0 || first + n > g->edges.n)
    return Fail(EULER_GPU_EINVAL, "export_edges: range outside the records");
  if (n == 0) return EULER_GPU_OK;
  DeviceGuard dg(g->device);
  DevBuf tmp;
  EG_HIP(tmp.alloc((size_t)n * 24));
  uint64_t* src = tmp.as<uint64_t>();
  uint64_t* dst = src + n;
  int32_t* ty = reinterpret_cast<int32_t*>(dst + n);
  float* w = reinterpret_cast<float*>(ty + n);
  hipLaunchKernelGGL(GatherRecordsKernel, dim3(GridFor(n, 256)), dim3(256), 0, 0, g->edges, first,
                     n, src, dst, ty, w, nullptr);
  rc = CheckLaunch("export_edges");
  if (rc != EULER_GPU_OK) return rc;
  if (src_host) EG_HIP(hipMemcpy(src_host, src, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (dst_host) EG_HIP(hipMemcpy(dst_host, dst, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (type_host) EG_HIP(hipMemcpy(type_host, ty, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (weight_host) EG_HIP(hipMemcpy(weight_host, w, (size_t)n * 4, hipMemcpyDeviceToHost));
  return EULER_GPU_OK;
}

int euler_gpu_graph_set_edge_sampler(euler_gpu_graph* g, const int64_t* order_host) {
  int rc = CheckEdgeQuery(g, "set_edge_sampler", 0, nullptr);
  if (rc != EULER_GPU_OK) return rc;
  DeviceGuard dg(g->device);
  AllocList a("edge store: ");
  NodeSamplerView sampler{};
  std::vector<float> sums;
  rc = BuildEdgeSampler(g->edges, g->edge_sampler.n_types, order_host, &a, &sampler, &sums);
  if (rc != EULER_GPU_OK) { a.Release(); return rc; }
  (void)hipDeviceSynchronize();          // (no launch may still read the old table)
  (void)hipFree(g->edge_sampler_alloc.first);   // the replaced table; the new one is handed over below
  g->bytes -= g->edge_sampler_alloc.second;
  g->edge_sampler_alloc = a.list.back();
  g->bytes += g->edge_sampler_alloc.second;
  g->edge_sampler = sampler;
  g->edge_weight_sums.swap(sums);
  return EULER_GPU_OK;
}

int euler_gpu_sample_edge(const euler_gpu_graph* g, void* stream, uint64_t seed, uint32_t call_id,
                          const int32_t* edge_types_host, int32_t k, int32_t count,
                          int64_t* out_dev) {
  int rc = CheckEdgeQuery(g, "sample_edge", 0, nullptr);
  if (rc != EULER_GPU_OK) return rc;
  if (count < 0 || k < 1 || !edge_types_host)
    return Fail(EULER_GPU_EINVAL, "sample_edge: bad arguments");
  SampleNodeArgs a{};
  a.s = g->edge_sampler;
  a.seed = seed; a.call_id = call_id; a.count = count;
  rc = PrepareSampleNode(g->edge_sampler, edge_types_host, k, "sample_edge", "edge", &a);
  if (rc != EULER_GPU_OK) return rc;
  if (count == 0) return EULER_GPU_OK;
  if (!out_dev) return Fail(EULER_GPU_EINVAL, "sample_edge: null output");
  hipLaunchKernelGGL(SampleEdgeKernel, dim3(GridFor(count, 256)), dim3(256), 0,
                     (hipStream_t)stream, a, g->edges.slots, out_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_edge_ordinals(const euler_gpu_graph* g, void* stream, const int64_t* edges_dev,
                            int64_t n, int64_t* out_dev) {
  int rc = CheckEdgeQuery(g, "edge_ordinals", n, edges_dev);
  if (rc != EULER_GPU_OK || n == 0) return rc;
  if (!out_dev) return Fail(EULER_GPU_EINVAL, "edge_ordinals: null output");
  hipLaunchKernelGGL(EdgeOrdinalKernel, dim3(GridFor(n * kGroup, 256)), dim3(256), 0,
                     (hipStream_t)stream, MakeQuery(g, edges_dev, n, 0, 0), out_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_get_edge_dense_feature(const euler_gpu_graph* g, void* stream,
                                     const int64_t* edges_dev, int64_t n, int32_t fid,
                                     int32_t dim, float* out_dev) {
  int rc = CheckEdgeQuery(g, "get_edge_dense_feature", n, edges_dev);
  if (rc != EULER_GPU_OK) return rc;
  if (dim < 0) return Fail(EULER_GPU_EINVAL, "get_edge_dense_feature: dim < 0");
  if (n == 0 || dim == 0) return EULER_GPU_OK;
  if (!out_dev) return Fail(EULER_GPU_EINVAL, "get_edge_dense_feature: null output");
  hipLaunchKernelGGL(EdgeDenseKernel, dim3(GridFor(n * kGroup, 256)), dim3(256), 0,
                     (hipStream_t)stream, MakeQuery(g, edges_dev, n, fid, dim), out_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_get_edge_sparse_feature(const euler_gpu_graph* g, void* stream,
                                      const int64_t* edges_dev, int64_t n, int32_t fid,
                                      int64_t default_value, int64_t* row_off_dev,
                                      int64_t* nnz_host, int64_t* max_len_host,
                                      int64_t* indices_dev, int64_t* values_dev) {
  int rc = CheckEdgeQuery(g, "get_edge_sparse_feature", n, edges_dev);
  if (rc != EULER_GPU_OK) return rc;
  if (n == 0) {
    if (nnz_host) *nnz_host = 0;
    if (max_len_host) *max_len_host = 0;
    return EULER_GPU_OK;
  }
  if (!row_off_dev) return Fail(EULER_GPU_EINVAL, "get_edge_sparse_feature: null offsets");
  hipStream_t st = (hipStream_t)stream;
  const EdgeQuery q = MakeQuery(g, edges_dev, n, fid, 0);
  if (indices_dev == nullptr) {
    return RaggedOffsets(st, n, [&](int64_t* counts, unsigned long long* mx) {
      hipLaunchKernelGGL(EdgeCountKernel, dim3(GridFor(n * kGroup, 256)), dim3(256), 0, st, q,
                         q.s.u64, 1, counts, mx);
    }, row_off_dev, nnz_host, max_len_host);
  }
  if (!values_dev) return Fail(EULER_GPU_EINVAL, "get_edge_sparse_feature: null values");
  hipLaunchKernelGGL(EdgeSparseFillKernel, dim3(GridFor(n * kGroup, 256)), dim3(256), 0, st, q,
                     row_off_dev, default_value, indices_dev, values_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_get_edge_binary_feature(const euler_gpu_graph* g, void* stream,
                                      const int64_t* edges_dev, int64_t n, int32_t fid,
                                      int64_t* offsets_dev, int64_t* total_host,
                                      uint8_t* bytes_dev) {
  int rc = CheckEdgeQuery(g, "get_edge_binary_feature", n, edges_dev);
  if (rc != EULER_GPU_OK) return rc;
  if (!offsets_dev) return Fail(EULER_GPU_EINVAL, "get_edge_binary_feature: null offsets");
  hipStream_t st = (hipStream_t)stream;
  const EdgeQuery q = MakeQuery(g, edges_dev, n, fid, 0);
  if (bytes_dev == nullptr) {
    return RaggedOffsets(st, n, [&](int64_t* counts, unsigned long long*) {
      if (n > 0)                           // (no maximum: the result has none)
        hipLaunchKernelGGL(EdgeCountKernel, dim3(GridFor(n * kGroup, 256)), dim3(256), 0, st, q,
                           q.s.bin, 0, counts, nullptr);
    }, offsets_dev, total_host, nullptr);
  }
  if (n == 0) return EULER_GPU_OK;
  hipLaunchKernelGGL(EdgeBinaryFillKernel, dim3(GridFor(n * kGroup, 256)), dim3(256), 0, st, q,
                     offsets_dev, bytes_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_get_binary_feature(const euler_gpu_graph* g, void* stream, const uint64_t* nodes_dev,
                                 int64_t n, int32_t fid, int64_t* offsets_dev, int64_t* total_host,
                                 uint8_t* bytes_dev) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "get_binary_feature: null graph");
  if (n < 0 || (n > 0 && !nodes_dev) || !offsets_dev)
    return Fail(EULER_GPU_EINVAL, "get_binary_feature: bad arguments");
  int rc = EnsureNodeBinary(g);
  if (rc != EULER_GPU_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const FeatTable t = g->node_bin;          // n_slots 0 when the graph has none: every row empty
  if (bytes_dev == nullptr) {
    return RaggedOffsets(st, n, [&](int64_t* counts, unsigned long long*) {
      if (n > 0)
        hipLaunchKernelGGL(NodeBinaryCountKernel, dim3(GridFor(n, 256)), dim3(256), 0, st, g->view,
                           t, nodes_dev, n, fid, counts);
    }, offsets_dev, total_host, nullptr);
  }
  if (n == 0) return EULER_GPU_OK;
  hipLaunchKernelGGL(NodeBinaryFillKernel, dim3(GridFor(n * 64, 256)), dim3(256), 0, st, g->view,
                     t, nodes_dev, n, fid, offsets_dev, bytes_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

}  // extern "C"
