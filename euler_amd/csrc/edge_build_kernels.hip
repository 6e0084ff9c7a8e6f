// The device passes of a graph built from an edge list (edge_build.h states them, their bytes and
// their limits) and the argument ladder of euler_gpu_graph_create_from_edges.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cstring>
#include <vector>

#include "device_fns.h"
#include "device_mem.h"
#include "edge_build.h"

namespace euler_gpu {

namespace {

// The list: entry p < E is edge p, entry E + p is edge p reversed (undirected lists only).
struct EdgeList {
  const uint64_t* src;
  const uint64_t* dst;
  const int32_t* type;       // or nullptr: all 0
  const float* w;            // or nullptr: all 1.0f
  int64_t E;
  int64_t total;             // E, or 2 E
};
__device__ __forceinline__ uint64_t ListSrc(const EdgeList& l, int64_t p) {
  return p < l.E ? l.src[p] : l.dst[p - l.E];
}
__device__ __forceinline__ uint64_t ListDst(const EdgeList& l, int64_t p) {
  return p < l.E ? l.dst[p] : l.src[p - l.E];
}
__device__ __forceinline__ int32_t ListType(const EdgeList& l, int64_t p) {
  return l.type ? l.type[p < l.E ? p : p - l.E] : 0;
}
__device__ __forceinline__ float ListWeight(const EdgeList& l, int64_t p) {
  return l.w ? l.w[p < l.E ? p : p - l.E] : 1.0f;
}

// What the passes report: flags end a property with a plain store of the value that ends it (every
// writer stores the same word), counts grow by vector atomics.
struct EbState {
  int32_t zero_nbr;                  // starts 0
  int32_t monotone;                  // starts 1
  int32_t uniform;                   // starts 1
  int32_t identity;                  // starts 1
  unsigned long long bad_type;       // entries whose type is outside [0, T)
  unsigned long long src_miss;       // entries whose src is no row
  unsigned long long dup;            // rows whose id an earlier slot of the table already holds
  unsigned long long max_id;
  unsigned long long n_long;         // rows longer than kEbLaneRow
  unsigned long long n_unique;       // distinct ids (nodes NULL)
};

__global__ __launch_bounds__(256) void EbConcatIdsKernel(const uint64_t* __restrict__ src,
                                                         const uint64_t* __restrict__ dst, int64_t E,
                                                         uint64_t* __restrict__ ids) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < E; p += stride) {
    ids[p] = src[p];
    ids[E + p] = dst[p];
  }
}

// identity: row r has the id base + r * stride; max_id: the largest id, unsigned
__global__ __launch_bounds__(256) void EbIdScanKernel(const uint64_t* __restrict__ row_id, int64_t n,
                                                      uint64_t base, uint64_t stride, EbState* st) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  uint64_t top = 0;
  bool same = true;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += step) {
    const uint64_t id = row_id[r];
    top = id > top ? id : top;
    same &= id == base + (uint64_t)r * stride;
  }
  if (!same) st->identity = 0;
  if (top != 0) atomicMax(&st->max_id, (unsigned long long)top);
}

// A slot is claimed through its row word (~0 = empty), so that 0 is a key like any other.  The
// table has room for 2 n + 1 keys: every insert meets an empty slot.
__global__ __launch_bounds__(256) void EbHashInsertKernel(const uint64_t* __restrict__ row_id, int64_t n,
                                                          uint64_t* slots, uint64_t mask) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint64_t key = row_id[r];
  uint64_t h = Mix64(key) & mask;
  for (uint64_t probes = 0; probes <= mask; ++probes) {
    const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(slots + 2 * h + 1),
                                             ~0ULL, (unsigned long long)r);
    if (old == ~0ULL) { slots[2 * h] = key; return; }
    h = (h + 1) & mask;
  }
}

// An id twice among the rows: the probe for the later copy stops at the earlier one
__global__ __launch_bounds__(256) void EbHashVerifyKernel(GraphView map, const uint64_t* __restrict__ row_id,
                                                          EbState* st) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= map.n_rows) return;
  if (FindRow(map, row_id[r]) != r) atomicAdd(&st->dup, 1ULL);
}

template <typename K>
__global__ __launch_bounds__(256) void EbKeysKernel(EdgeList l, GraphView map, int32_t T, K* __restrict__ keys,
                                                    uint32_t* __restrict__ pos, EbState* st) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < l.total; p += stride) {
    int64_t row = FindRow(map, ListSrc(l, p));
    int32_t t = ListType(l, p);
    if (t < 0 || t >= T) { atomicAdd(&st->bad_type, 1ULL); t = 0; }
    if (row < 0) { atomicAdd(&st->src_miss, 1ULL); row = 0; }
    keys[p] = (K)((uint64_t)row * (uint64_t)T + (uint64_t)t);
    pos[p] = (uint32_t)p;
  }
}

// seg[q] = the first sorted entry whose key is >= q (q = n_keys: total)
template <typename K>
__global__ __launch_bounds__(256) void EbSegmentsKernel(const K* __restrict__ keys, int64_t total,
                                                        int64_t n_keys, int64_t* __restrict__ seg) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= n_keys; q += stride) {
    int64_t lo = 0, hi = total;               // keys[lo - 1] < q <= keys[hi]
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((uint64_t)keys[mid] < (uint64_t)q) lo = mid + 1; else hi = mid;
    }
    seg[q] = lo;
  }
}

__global__ __launch_bounds__(256) void EbGatherKernel(EdgeList l, const uint32_t* __restrict__ pos,
                                                      uint64_t* __restrict__ nbr, float* __restrict__ w,
                                                      EbState* st) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  bool zero = false;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < l.total; j += stride) {
    const int64_t p = (int64_t)pos[j];
    const uint64_t id = ListDst(l, p);
    zero |= id == 0;
    nbr[j] = id;
    w[j] = ListWeight(l, p);
  }
  if (zero) st->zero_nbr = 1;
}

// Node::Init (core/graph/node.cc:46-66) for the rows of up to kEbLaneRow entries, a lane each:
// the running sum over the whole row and each group's own sum are sequential f32 chains.  A longer
// row gets its record's offset here and goes on the list of the wave kernel.
__global__ __launch_bounds__(256) void EbPrefixLaneKernel(int32_t T, int32_t meta_stride, int64_t n_rows,
                                                          const int64_t* __restrict__ seg, float* w_inout,
                                                          uint8_t* __restrict__ row_meta,
                                                          int64_t* __restrict__ long_rows, EbState* st) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const int64_t* s = seg + r * T;
  const int64_t base = s[0];
  const int64_t deg = s[T] - base;
  uint8_t* rec = row_meta + r * (int64_t)meta_stride;
  *reinterpret_cast<int64_t*>(rec) = base;
  if (deg > kEbLaneRow) {
    long_rows[atomicAdd(&st->n_long, 1ULL)] = r;
    return;
  }
  int32_t* type_end = reinterpret_cast<int32_t*>(rec + 8);
  float* type_prefix = reinterpret_cast<float*>(rec + 8 + 4 * T);
  float sum = 0.f, tsum = 0.f, prev = 0.f;
  bool mono = true, uni = true;
  int64_t j = 0;
  for (int32_t t = 0; t < T; ++t) {
    const int64_t end = s[t + 1] - base;
    float tw = 0.f;
    for (; j < end; ++j) {
      const float x = w_inout[base + j];
      sum = __fadd_rn(sum, x);
      tw = __fadd_rn(tw, x);
      w_inout[base + j] = sum;
      mono &= sum >= prev;                    // false for NaN too
      uni &= sum == (float)(j + 1);           // (j + 1 <= kEbLaneRow < 2^24)
      prev = sum;
    }
    type_end[t] = (int32_t)end;
    tsum = __fadd_rn(tsum, tw);
    type_prefix[t] = tsum;
  }
  if (!mono) st->monotone = 0;
  if (!uni) st->uniform = 0;
}

// ... and for the longer rows, a wave each.  Per step the wave loads kEbChunk raw weights into LDS
// (coalesced), lane 0 turns them into the running sums in entry order - the two chains are the
// ones of the lane kernel, fed from LDS - and all lanes store the sums and test them against
// their predecessors for the flags.
__global__ __launch_bounds__(64) void EbPrefixWaveKernel(int32_t T, int32_t meta_stride,
                                                         const int64_t* __restrict__ seg, float* w_inout,
                                                         uint8_t* __restrict__ row_meta,
                                                         const int64_t* __restrict__ long_rows, int64_t n_long,
                                                         EbState* st) {
  __shared__ float buf[kEbChunk];
  const int lane = threadIdx.x;
  bool mono = true, uni = true;
  for (int64_t i = blockIdx.x; i < n_long; i += gridDim.x) {
    const int64_t r = long_rows[i];
    const int64_t* s = seg + r * T;
    const int64_t base = s[0];
    const int64_t deg = s[T] - base;
    uint8_t* rec = row_meta + r * (int64_t)meta_stride;
    int32_t* type_end = reinterpret_cast<int32_t*>(rec + 8);
    float* type_prefix = reinterpret_cast<float*>(rec + 8 + 4 * T);
    float sum = 0.f, tsum = 0.f, tw = 0.f;      // lane 0's chains
    int32_t t = 0;                              // ... and the group its next entry is in
    float carry = 0.f;                          // the sum before this step's first entry
    for (int64_t c = 0; c < deg; c += kEbChunk) {
      const int len = (int)(deg - c < kEbChunk ? deg - c : kEbChunk);
      for (int k = lane; k < len; k += 64) buf[k] = w_inout[base + c + k];
      __syncthreads();
      if (lane == 0) {
        int64_t j = c;
        const int64_t stop = c + len;
        while (j < stop) {
          while (t < T - 1 && j >= s[t + 1] - base) {      // group t is complete (or empty)
            tsum = __fadd_rn(tsum, tw); type_prefix[t] = tsum; tw = 0.f; ++t;
          }
          int64_t run = t < T - 1 ? s[t + 1] - base : deg;
          if (run > stop) run = stop;
          // eight weights at a time: the LDS reads are issued together, the adds stay one chain
          for (; j + 8 <= run; j += 8) {
            float x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = buf[j - c + q];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              sum = __fadd_rn(sum, x[q]);
              tw = __fadd_rn(tw, x[q]);
              x[q] = sum;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) buf[j - c + q] = x[q];
          }
          for (; j < run; ++j) {
            const float x = buf[j - c];
            sum = __fadd_rn(sum, x);
            tw = __fadd_rn(tw, x);
            buf[j - c] = sum;
          }
        }
      }
      __syncthreads();
      for (int k = lane; k < len; k += 64) {
        const float cur = buf[k];
        const float prev = k > 0 ? buf[k - 1] : carry;
        const int64_t j = c + k;
        mono &= cur >= prev;                             // false for NaN too
        uni &= cur == (float)(j + 1) && j + 1 < (1 << 24);
        w_inout[base + c + k] = cur;
      }
      carry = buf[len - 1];
      __syncthreads();
    }
    if (lane == 0) {
      for (; t < T; ++t) { tsum = __fadd_rn(tsum, tw); type_prefix[t] = tsum; tw = 0.f; }
      for (int32_t x = 0; x < T; ++x) type_end[x] = (int32_t)(s[x + 1] - base);
    }
  }
  if (!mono) st->monotone = 0;
  if (!uni) st->uniform = 0;
}

// slot values [n, d] -> columns [off, off + d) of the rows of stride `stride`
__global__ __launch_bounds__(256) void EbFeatureKernel(const float* __restrict__ in, int64_t n, int64_t d,
                                                       int64_t stride, int64_t off, float* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  const int64_t total = n * d;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    const int64_t r = i / d;
    out[r * stride + off + (i - r * d)] = in[i];
  }
}

// feat_ptr[r] = r * stride (r = 0 .. n), feat_idx[r * F + f] = ends[f]
__global__ __launch_bounds__(256) void EbFeatIndexKernel(int64_t n, int32_t F, int64_t stride,
                                                         const int32_t* __restrict__ ends,
                                                         int64_t* __restrict__ feat_ptr,
                                                         int32_t* __restrict__ feat_idx) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += step) {
    feat_ptr[r] = r * stride;
    if (r < n)
      for (int32_t f = 0; f < F; ++f) feat_idx[r * F + f] = ends[f];
  }
}

int KeyBits(uint64_t n_keys) {          // the bits of n_keys - 1, at least 1
  int bits = 1;
  while (n_keys > 1 && bits < 64 && ((n_keys - 1) >> bits) != 0) ++bits;
  return bits;
}

// Drains the stream and books the time since the previous lap to `pass`
struct PassClock {
  hipStream_t st;
  float* ms;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  hipError_t Lap(int pass) {
    const hipError_t e = hipStreamSynchronize(st);
    const auto t1 = std::chrono::steady_clock::now();
    ms[pass] += std::chrono::duration<float, std::milli>(t1 - t0).count();
    t0 = t1;
    return e;
  }
};

// keys -> sorted (key, position) -> seg, for one key width.  The double buffers are `pairs`.
template <typename K>
int SortedSegments(hipStream_t st, const EdgeList& l, const GraphView& map, int32_t T, uint64_t n_keys,
                   EbState* state, DevBuf* pairs, const uint32_t** pos_sorted, int64_t* seg, PassClock* clock) {
  const size_t n = (size_t)l.total;
  EG_HIP(pairs->alloc(n * 2 * (sizeof(K) + 4) + 64));
  K* keys_a = pairs->as<K>();
  K* keys_b = keys_a + n;
  uint32_t* pos_a = reinterpret_cast<uint32_t*>(keys_b + n);
  uint32_t* pos_b = pos_a + n;
  if (n > 0) {
    hipLaunchKernelGGL(EbKeysKernel<K>, dim3(GridFor((int64_t)n, 256)), dim3(256), 0, st, l, map, T, keys_a, pos_a,
                       state);
    EG_HIP(hipGetLastError());
  }
  EbState host;
  EG_HIP(hipMemcpyAsync(&host, state, sizeof(host), hipMemcpyDeviceToHost, st));
  EG_HIP(clock->Lap(kEbKeys));
  const char* const who = "graph_create_from_edges: ";
  if (host.bad_type != 0)
    return Fail(EULER_GPU_EINVAL, std::string(who) + std::to_string(host.bad_type) + " edges have a type outside [0, " +
                                      std::to_string(T) + ")");
  if (host.src_miss != 0)
    return Fail(EULER_GPU_EINVAL, std::string(who) + std::to_string(host.src_miss) +
                                      " entries of the list (the edges, then their reverses when undirected) have a "
                                      "src that is not in nodes");
  hipcub::DoubleBuffer<K> dk(keys_a, keys_b);
  hipcub::DoubleBuffer<uint32_t> dp(pos_a, pos_b);
  if (n > 0) {
    const int bits = std::min(KeyBits(n_keys), (int)sizeof(K) * 8);
    size_t tmp_bytes = 0;
    EG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, dk, dp, (int64_t)n, 0, bits, st));
    DevBuf tmp;
    EG_HIP(tmp.alloc(tmp_bytes + 16));
    EG_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.as(), tmp_bytes, dk, dp, (int64_t)n, 0, bits, st));
    EG_HIP(hipStreamSynchronize(st));       // (the scratch goes back with tmp)
  }
  EG_HIP(clock->Lap(kEbSort));
  hipLaunchKernelGGL(EbSegmentsKernel<K>, dim3(GridFor((int64_t)n_keys + 1, 256)), dim3(256), 0, st, dk.Current(),
                     (int64_t)n, (int64_t)n_keys, seg);
  EG_HIP(hipGetLastError());
  EG_HIP(clock->Lap(kEbSegments));
  *pos_sorted = dp.Current();
  return EULER_GPU_OK;
}

}  // namespace

int CheckDevEdges(const euler_gpu_dev_edges* e, euler_gpu_graph** out) {
  const char* const who = "graph_create_from_edges: ";
  auto bad = [who](const char* why) { return Fail(EULER_GPU_EINVAL, std::string(who) + why); };
  if (out) *out = nullptr;
  if (!e || !out) return bad("null argument");
  if (e->n_edges < 0 || (e->nodes && e->n_nodes < 0) || e->n_features < 0) return bad("negative size");
  if (e->n_edge_types < 1 || e->n_edge_types > kMaxListedTypes) return bad("need 1..32 edge types");
  if (e->n_node_types < 0 || e->n_node_types > kMaxNodeTypes) return bad("need 0..32 node types (0 = 1)");
  if (e->n_edges > 0 && (!e->src || !e->dst)) return bad("null src or dst");
  if (!e->nodes && e->n_features > 0) return bad("features need nodes (the rows' order is what places them)");
  if (!e->nodes && (e->node_type || e->node_weight))
    return bad("node_type and node_weight need nodes (the rows' order is what places them)");
  const int64_t N = e->nodes ? e->n_nodes : 0;
  if (e->n_features > 0) {
    if (!e->features || !e->feature_dims) return bad("null feature array");
    int64_t sum = 0;
    for (int32_t f = 0; f < e->n_features; ++f) {
      if (e->feature_dims[f] < 1) return bad("a feature width < 1");
      if (N > 0 && !e->features[f]) return bad("null feature array");
      sum += e->feature_dims[f];
    }
    if (sum >= (1LL << 31)) return bad("the feature widths sum to 2^31 or more");
  }
  auto off = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  bool misaligned = off(e->src, 8) || off(e->dst, 8) || off(e->nodes, 8) || off(e->type, 4) || off(e->weight, 4) ||
                    off(e->node_type, 4) || off(e->node_weight, 4);
  for (int32_t f = 0; f < e->n_features; ++f) misaligned |= off(e->features[f], 4);
  if (misaligned) return bad("a buffer is not aligned to its type");
  if (e->n_edges >= (1LL << 31) || (e->undirected && e->n_edges >= (1LL << 30)))
    return bad("the list (E entries, 2 E when undirected) must have fewer than 2^31 entries");
  return EULER_GPU_OK;
}

int BuildRowsFromEdges(const euler_gpu_dev_edges* e, hipStream_t st, AllocList* blocks, GraphView* vp,
                       EdgeBuildFacts* facts) {
  const char* const who = "graph_create_from_edges: ";
  GraphView& v = *vp;
  const int32_t T = e->n_edge_types;
  const int block = 256;
  EdgeList l{e->src, e->dst, e->type, e->weight, e->n_edges, e->undirected ? 2 * e->n_edges : e->n_edges};
  PassClock clock{st, facts->pass_ms};

  DevBuf state_buf;
  EG_HIP(state_buf.alloc(sizeof(EbState)));
  EbState* state = state_buf.as<EbState>();
  EbState host{};
  host.monotone = 1; host.uniform = 1; host.identity = 1;
  EG_HIP(hipMemcpyAsync(state, &host, sizeof(host), hipMemcpyHostToDevice, st));
  EG_HIP(hipStreamSynchronize(st));             // (host is read by the copy until then)

  // ---- rows
  int64_t N = 0;
  uint64_t* row_id = nullptr;
  if (e->nodes) {
    N = e->n_nodes;
    row_id = blocks->Alloc<uint64_t>((size_t)N);
    if (blocks->rc != EULER_GPU_OK) return blocks->rc;
    if (N > 0) EG_HIP(hipMemcpyAsync(row_id, e->nodes, (size_t)N * 8, hipMemcpyDeviceToDevice, st));
  } else {
    const int64_t n_ids = 2 * l.E;
    if (n_ids > 0) {
      DevBuf ids_buf;
      EG_HIP(ids_buf.alloc((size_t)n_ids * 16 + 64));
      uint64_t* ids_a = ids_buf.as<uint64_t>();
      uint64_t* ids_b = ids_a + n_ids;
      hipLaunchKernelGGL(EbConcatIdsKernel, dim3(GridFor(l.E, block)), dim3(block), 0, st, l.src, l.dst, l.E, ids_a);
      EG_HIP(hipGetLastError());
      hipcub::DoubleBuffer<uint64_t> d(ids_a, ids_b);
      size_t sort_bytes = 0, unique_bytes = 0;
      EG_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, d, n_ids, 0, 64, st));
      EG_HIP(hipcub::DeviceSelect::Unique(nullptr, unique_bytes, ids_a, ids_b, &state->n_unique, n_ids, st));
      DevBuf tmp;
      EG_HIP(tmp.alloc(std::max(sort_bytes, unique_bytes) + 16));
      EG_HIP(hipcub::DeviceRadixSort::SortKeys(tmp.as(), sort_bytes, d, n_ids, 0, 64, st));
      // the distinct ids go to the sort's other buffer, which it is done with
      EG_HIP(hipcub::DeviceSelect::Unique(tmp.as(), unique_bytes, d.Current(), d.Alternate(), &state->n_unique,
                                          n_ids, st));
      unsigned long long n_unique = 0;
      EG_HIP(hipMemcpyAsync(&n_unique, &state->n_unique, 8, hipMemcpyDeviceToHost, st));
      EG_HIP(hipStreamSynchronize(st));
      N = (int64_t)n_unique;
      row_id = blocks->Alloc<uint64_t>((size_t)N);
      if (blocks->rc != EULER_GPU_OK) return blocks->rc;
      EG_HIP(hipMemcpyAsync(row_id, d.Alternate(), (size_t)N * 8, hipMemcpyDeviceToDevice, st));
      EG_HIP(hipStreamSynchronize(st));         // (ids_buf and tmp go back here)
    } else {
      row_id = blocks->Alloc<uint64_t>(0);
      if (blocks->rc != EULER_GPU_OK) return blocks->rc;
    }
  }
  EG_HIP(clock.Lap(kEbRows));
  v.n_rows = N;
  v.n_edges = l.total;
  v.T = T;
  v.meta_stride = 8 + 8 * T;
  v.row_id = row_id;

  // ---- id map
  uint64_t first[2] = {0, 0};
  if (N > 0) EG_HIP(hipMemcpyAsync(first, row_id, (size_t)(N > 1 ? 2 : 1) * 8, hipMemcpyDeviceToHost, st));
  EG_HIP(hipStreamSynchronize(st));
  bool identity = N > 0;
  const uint64_t base = first[0];
  uint64_t stride = 1;
  if (N > 1) {
    stride = first[1] - first[0];
    if (first[1] <= first[0]) identity = false;
  }
  if (N > 0) {
    hipLaunchKernelGGL(EbIdScanKernel, dim3(GridFor(N, block)), dim3(block), 0, st, row_id, N, base, stride, state);
    EG_HIP(hipGetLastError());
    EG_HIP(hipMemcpyAsync(&host, state, sizeof(host), hipMemcpyDeviceToHost, st));
    EG_HIP(hipStreamSynchronize(st));
    identity = identity && host.identity != 0;
    facts->max_id = host.max_id;
  }
  if (identity) {
    v.map_mode = 0; v.id_base = base; v.id_stride = stride;
  } else {
    uint64_t cap = 16;
    while (cap < (uint64_t)N * 2 + 1) cap <<= 1;
    uint64_t* slots = blocks->Alloc<uint64_t>((size_t)(2 * cap));
    if (blocks->rc != EULER_GPU_OK) return blocks->rc;
    LaunchHashInit(st, slots, cap);             // graph_build.hip's HashInitKernel
    if (N > 0)
      hipLaunchKernelGGL(EbHashInsertKernel, dim3((unsigned)((N + block - 1) / block)), dim3(block), 0, st, row_id, N,
                         slots, cap - 1);
    EG_HIP(hipGetLastError());
    v.map_mode = 1; v.hash_slots = slots; v.hash_mask = cap - 1; v.id_base = 0; v.id_stride = 1;
    if (N > 0 && e->nodes) {
      hipLaunchKernelGGL(EbHashVerifyKernel, dim3((unsigned)((N + block - 1) / block)), dim3(block), 0, st, v, row_id,
                         state);
      EG_HIP(hipGetLastError());
      EG_HIP(hipMemcpyAsync(&host, state, sizeof(host), hipMemcpyDeviceToHost, st));
      EG_HIP(hipStreamSynchronize(st));
      if (host.dup != 0)
        return Fail(EULER_GPU_EINVAL, std::string(who) + "an id occurs more than once in nodes (" +
                                          std::to_string(host.dup) + " repeated rows)");
    }
  }
  EG_HIP(clock.Lap(kEbIdMap));

  // ---- keys, sort, segments
  const uint64_t n_keys = (uint64_t)N * (uint64_t)T;
  DevBuf pairs, seg_buf, long_buf;
  EG_HIP(seg_buf.alloc(((size_t)n_keys + 1) * 8 + 16));
  int64_t* seg = seg_buf.as<int64_t>();
  const uint32_t* pos_sorted = nullptr;
  {
    const int rc = n_keys <= (1ULL << 32)
        ? SortedSegments<uint32_t>(st, l, v, T, n_keys, state, &pairs, &pos_sorted, seg, &clock)
        : SortedSegments<uint64_t>(st, l, v, T, n_keys, state, &pairs, &pos_sorted, seg, &clock);
    if (rc != EULER_GPU_OK) return rc;
  }
  // ---- gather: the graph's own arrays
  uint64_t* nbr = blocks->Alloc<uint64_t>((size_t)l.total);
  float* pw = blocks->Alloc<float>((size_t)l.total);
  uint8_t* meta = blocks->Alloc<uint8_t>((size_t)N * v.meta_stride + 16);
  if (blocks->rc != EULER_GPU_OK) return blocks->rc;
  EG_HIP(hipMemsetAsync(meta, 0, (size_t)N * v.meta_stride + 16, st));
  if (l.total > 0) {
    hipLaunchKernelGGL(EbGatherKernel, dim3(GridFor(l.total, block)), dim3(block), 0, st, l, pos_sorted, nbr, pw,
                       state);
    EG_HIP(hipGetLastError());
  }
  EG_HIP(clock.Lap(kEbGather));
  pairs.reset();

  // ---- prefix sums and row records
  EG_HIP(long_buf.alloc(((size_t)l.total / (kEbLaneRow + 1) + 1) * 8));
  int64_t* long_rows = long_buf.as<int64_t>();
  if (N > 0) {
    hipLaunchKernelGGL(EbPrefixLaneKernel, dim3((unsigned)((N + block - 1) / block)), dim3(block), 0, st, T,
                       v.meta_stride, N, seg, pw, meta, long_rows, state);
    EG_HIP(hipGetLastError());
  }
  EG_HIP(hipMemcpyAsync(&host, state, sizeof(host), hipMemcpyDeviceToHost, st));
  EG_HIP(clock.Lap(kEbPrefixLane));
  if (host.n_long > 0) {
    const int64_t n_long = (int64_t)host.n_long;
    hipLaunchKernelGGL(EbPrefixWaveKernel, dim3((unsigned)std::min<int64_t>(n_long, 256 * 32)), dim3(64), 0, st, T,
                       v.meta_stride, seg, pw, meta, long_rows, n_long, state);
    EG_HIP(hipGetLastError());
  }
  EG_HIP(hipMemcpyAsync(&host, state, sizeof(host), hipMemcpyDeviceToHost, st));
  EG_HIP(clock.Lap(kEbPrefixWave));
  seg_buf.reset();
  long_buf.reset();
  v.nbr = nbr; v.prefix_w = pw; v.row_meta = meta;
  v.has_zero_nbr = host.zero_nbr != 0 ? 1 : 0;
  v.monotone = host.monotone != 0 ? 1 : 0;
  v.uniform_w = (host.uniform != 0 && host.monotone != 0 && l.total > 0) ? 1 : 0;

  // ---- dense features, node types
  DevBuf ends_buf;                              // the slots' ends, for the index kernel only
  std::vector<int32_t> ends;
  if (e->n_features > 0) {
    const int32_t F = e->n_features;
    ends.resize((size_t)F);
    int64_t sum = 0;
    for (int32_t f = 0; f < F; ++f) { sum += e->feature_dims[f]; ends[(size_t)f] = (int32_t)sum; }
    const bool uniform = N > 0;                 // (as the host path: no row, no layout to share)
    bool aligned = uniform;
    for (int32_t f = 0; aligned && f + 1 < F; ++f) aligned = ends[(size_t)f] % 4 == 0;
    EG_HIP(ends_buf.alloc((size_t)F * 4));
    int32_t* ends_dev = ends_buf.as<int32_t>();
    EG_HIP(hipMemcpyAsync(ends_dev, ends.data(), (size_t)F * 4, hipMemcpyHostToDevice, st));
    int64_t* feat_ptr = blocks->Alloc<int64_t>((size_t)N + 1);
    int32_t* feat_idx = blocks->Alloc<int32_t>((size_t)N * F);
    float* feat_val = blocks->Alloc<float>((size_t)N * (size_t)sum);
    if (blocks->rc != EULER_GPU_OK) return blocks->rc;
    hipLaunchKernelGGL(EbFeatIndexKernel, dim3(GridFor(N + 1, block)), dim3(block), 0, st, N, F, sum, ends_dev,
                       feat_ptr, feat_idx);
    for (int32_t f = 0; f < F && N > 0; ++f)
      hipLaunchKernelGGL(EbFeatureKernel, dim3(GridFor(N * e->feature_dims[f], block)), dim3(block), 0, st,
                         e->features[f], N, (int64_t)e->feature_dims[f], sum,
                         (int64_t)(ends[(size_t)f] - e->feature_dims[f]), feat_val);
    EG_HIP(hipGetLastError());
    v.n_float = F;
    v.feat_uniform = uniform ? 1 : 0;
    v.feat_stride = uniform ? sum : 0;
    v.feat_ptr = feat_ptr; v.feat_idx = feat_idx; v.feat_val = feat_val;
    facts->feat_slot_aligned = aligned;
  }
  if (e->node_type && N > 0) {
    int32_t* types = blocks->Alloc<int32_t>((size_t)N);
    if (blocks->rc != EULER_GPU_OK) return blocks->rc;
    EG_HIP(hipMemcpyAsync(types, e->node_type, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
    facts->node_type_dev = types;
  }
  EG_HIP(clock.Lap(kEbFeatures));            // (drains the stream: ends_buf and ends may go)
  return EULER_GPU_OK;
}

}  // namespace euler_gpu
