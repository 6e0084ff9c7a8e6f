// Graph labels (whole-graph classification input path):
//   the label index      Graph::GetGraphLabel / graph_label_ index (core/graph/graph.cc:439-457)
//   API_SAMPLE_GRAPH_LABEL   core/kernels/sample_graph_label_op.cc:32-66
//   API_GET_GRAPH_BY_LABEL   core/kernels/get_graph_by_label_op.cc:32-75
//   the whole-graph block    tf_euler/python/dataflow/whole_dataflow.py:37-63 (Q16)
//
// The index lives in two device arrays: label_nodes [labelled nodes] (uint64 ids, grouped by
// label in table order, ascending ids inside a label) and label_start [labels + 1] (int64): 8 B per
// labelled node and 8 B per label.  The label table itself (bytes, offsets, the string -> id map)
// is kept on the host, where export and lookup run.  It is built on the device: hash every node's label bytes, sort
// by (hash, id) with two stable radix sorts, mark the runs, order the labels by their smallest
// id.  Equal hashes of different labels are found on the device (adjacent entries of one run
// whose bytes differ) and the affected runs are split on the host (rare: tests force them with
// tuning key 74).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "common.h"
#include "device_mem.h"
#include "device_fns.h"

namespace euler_gpu {

thread_local int g_label_hash_bits = 64;   // euler_gpu_set_tuning key 74

namespace {

constexpr uint64_t kNoLabel = ~0ULL;     // hash key of an entry without a label (sorts last)

__device__ __forceinline__ uint64_t RowIdOf(const GraphView& v, int64_t row) {
  return v.row_id ? v.row_id[row] : v.id_base + v.id_stride * (uint64_t)row;
}

// --------------------------------------------------------------- index build
// Entries of a build: (id, first byte, length) of every node that may carry a label.

// from the node binary table: slot `slot` of every row
__global__ __launch_bounds__(256) void EntriesFromSlotKernel(const GraphView v, const FeatTable t,
                                                             int32_t slot, uint64_t* id,
                                                             int64_t* beg, int32_t* len) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < v.n_rows; r += stride) {
    int32_t l = 0;
    int64_t first = 0;
    if (slot < t.n_slots) {
      const int32_t* idx = t.uniform ? t.idx : t.idx + r * (int64_t)t.n_slots;
      const int32_t pre = slot == 0 ? 0 : idx[slot - 1];
      first = (t.uniform ? r * t.stride : t.ptr[r]) + pre;
      l = idx[slot] - pre;
    }
    id[r] = RowIdOf(v, r);
    beg[r] = first;
    len[r] = l;
  }
}

// from host arrays: every id must have a row (bad counts the misses)
__global__ __launch_bounds__(256) void CheckIdsKernel(const GraphView v, const uint64_t* id, int64_t n,
                                                      unsigned long long* bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    if (FindRow(v, id[i]) < 0) atomicAdd(bad, 1ULL);
}

// FNV-1a over the label bytes, finished by Mix64, narrowed to `bits`; kNoLabel for "" (Q15)
__global__ __launch_bounds__(256) void HashKernel(const uint8_t* val, const int64_t* beg,
                                                  const int32_t* len, int64_t n, int32_t bits,
                                                  uint64_t* key, int64_t* iota,
                                                  unsigned long long* n_valid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int32_t l = len[i];
    uint64_t h = kNoLabel;
    if (l > 0) {
      const uint8_t* p = val + beg[i];
      uint64_t f = 0xcbf29ce484222325ULL;
      for (int32_t k = 0; k < l; ++k) f = (f ^ p[k]) * 0x100000001b3ULL;
      h = Mix64(f);
      if (bits < 64) h &= (1ULL << bits) - 1ULL;
      if (h == kNoLabel) h = kNoLabel - 1;
      atomicAdd(n_valid, 1ULL);
    }
    key[i] = h;
    iota[i] = i;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void GatherKernel(const T* in, const int64_t* idx, int64_t n, T* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = in[idx[i]];
}

// sorted by id: two labelled entries of one id (set_graph_labels listed a node twice)
__global__ __launch_bounds__(256) void DupIdsKernel(const uint64_t* sid, const int64_t* perm,
                                                    const int32_t* len, int64_t n,
                                                    unsigned long long* dup) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    if (sid[i] == sid[i - 1] && len[perm[i]] > 0 && len[perm[i - 1]] > 0) atomicAdd(dup, 1ULL);
}

__device__ __forceinline__ bool SameBytes(const uint8_t* val, const int64_t* beg,
                                          const int32_t* len, int64_t a, int64_t b) {
  const int32_t l = len[a];
  if (len[b] != l) return false;
  const uint8_t* p = val + beg[a];
  const uint8_t* q = val + beg[b];
  for (int32_t k = 0; k < l; ++k)
    if (p[k] != q[k]) return false;
  return true;
}

// run heads of the (hash, id) order; a run whose neighbours differ in bytes is a collision
__global__ __launch_bounds__(256) void HeadsKernel(const uint64_t* hs, const int64_t* perm,
                                                   const uint8_t* val, const int64_t* beg,
                                                   const int32_t* len, int64_t nv, int64_t* head,
                                                   unsigned long long* collisions) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    const bool h = i == 0 || hs[i] != hs[i - 1];
    head[i] = h ? 1 : 0;
    if (!h && !SameBytes(val, beg, len, perm[i], perm[i - 1])) atomicAdd(collisions, 1ULL);
  }
}

// excl = exclusive scan of head: segment of i = excl[i] + head[i] - 1; the head of every
// segment records its position and its smallest id
__global__ __launch_bounds__(256) void SegmentsKernel(const int64_t* head, const int64_t* excl,
                                                      const int64_t* perm, const uint64_t* id,
                                                      int64_t nv, int64_t* seg_of, int64_t* seg_head,
                                                      uint64_t* seg_min, int64_t* seg_iota) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    const int64_t s = excl[i] + head[i] - 1;
    seg_of[i] = s;
    if (head[i]) {
      seg_head[s] = i;
      seg_min[s] = id[perm[i]];
      seg_iota[s] = s;
    }
  }
}

// label r of the table = segment order[r]: its size and the length of its bytes
__global__ __launch_bounds__(256) void LabelSizesKernel(const int64_t* order, const int64_t* seg_head,
                                                        const int64_t* perm, const int32_t* len,
                                                        int64_t L, int64_t nv, int64_t* rank,
                                                        int64_t* size, int64_t* blen) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < L; r += stride) {
    const int64_t s = order[r];
    rank[s] = r;
    size[r] = (s + 1 < L ? seg_head[s + 1] : nv) - seg_head[s];
    blen[r] = len[perm[seg_head[s]]];
  }
}

__global__ __launch_bounds__(256) void PlaceNodesKernel(const int64_t* seg_of, const int64_t* seg_head,
                                                        const int64_t* rank, const int64_t* start,
                                                        const int64_t* perm, const uint64_t* id,
                                                        int64_t nv, uint64_t* nodes) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    const int64_t s = seg_of[i];
    nodes[start[rank[s]] + (i - seg_head[s])] = id[perm[i]];
  }
}

// one wave per label copies its bytes
__global__ __launch_bounds__(256) void LabelBytesKernel(const int64_t* order, const int64_t* seg_head,
                                                        const int64_t* perm, const uint8_t* val,
                                                        const int64_t* beg, const int64_t* boff,
                                                        int64_t L, uint8_t* out) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < L; r += n_waves) {
    const uint8_t* p = val + beg[perm[seg_head[order[r]]]];
    const int64_t l = boff[r + 1] - boff[r];
    for (int64_t k = lane; k < l; k += 64) out[boff[r] + k] = p[k];
  }
}

template <typename T>
T* Carve(uint8_t*& at, int64_t n) {
  T* p = reinterpret_cast<T*>(at);
  at += ((size_t)std::max<int64_t>(n, 1) * sizeof(T) + 15) & ~(size_t)15;
  return p;
}

template <typename K, typename V>
int SortPairs(const K* kin, K* kout, const V* vin, V* vout, int64_t n, int end_bit) {
  size_t tmp_bytes = 0;
  EG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, kin, kout, vin, vout, (int)n, 0,
                                            end_bit, (hipStream_t)0));
  DevBuf tmp;
  EG_HIP(tmp.alloc(tmp_bytes + 16));
  EG_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.as(), tmp_bytes, kin, kout, vin, vout, (int)n, 0,
                                            end_bit, (hipStream_t)0));
  return EULER_GPU_OK;
}

template <typename T>
int Download(std::vector<T>* out, const T* dev, int64_t n) {
  out->resize((size_t)n);
  if (n > 0) EG_HIP(hipMemcpy(out->data(), dev, (size_t)n * sizeof(T), hipMemcpyDeviceToHost));
  return EULER_GPU_OK;
}

// The collisions: in every hash run whose entries do not all carry the same bytes, order the
// entries by their bytes (stably: ids stay ascending inside a label) and mark a head wherever the
// bytes change.  Downloads the order, the entries and the bytes; rewrites perm and head.
int SplitCollisions(int64_t m, int64_t nv, const uint64_t* hs_d, int64_t* perm_d, int64_t* head_d,
                    const uint8_t* val_d, int64_t val_bytes, const int64_t* beg_d,
                    const int32_t* len_d) {
  std::vector<uint64_t> hs;
  std::vector<int64_t> perm, beg;
  std::vector<int32_t> len;
  std::vector<uint8_t> val;
  int rc = Download(&hs, hs_d, nv);
  if (rc == EULER_GPU_OK) rc = Download(&perm, (const int64_t*)perm_d, nv);
  if (rc == EULER_GPU_OK) rc = Download(&beg, beg_d, m);
  if (rc == EULER_GPU_OK) rc = Download(&len, len_d, m);
  if (rc == EULER_GPU_OK) rc = Download(&val, val_d, val_bytes);
  if (rc != EULER_GPU_OK) return rc;
  auto bytes_of = [&](int64_t e) {
    return std::string(reinterpret_cast<const char*>(val.data()) + beg[e], (size_t)len[e]);
  };
  std::vector<int64_t> head((size_t)nv, 0);
  for (int64_t a = 0; a < nv;) {
    int64_t b = a + 1;
    while (b < nv && hs[b] == hs[a]) ++b;
    std::vector<std::pair<std::string, int64_t>> run;
    run.reserve((size_t)(b - a));
    for (int64_t i = a; i < b; ++i) run.emplace_back(bytes_of(perm[i]), perm[i]);
    std::stable_sort(run.begin(), run.end(),
                     [](const std::pair<std::string, int64_t>& x,
                        const std::pair<std::string, int64_t>& y) { return x.first < y.first; });
    for (int64_t i = a; i < b; ++i) {
      perm[i] = run[i - a].second;
      head[i] = (i == a || run[i - a].first != run[i - a - 1].first) ? 1 : 0;
    }
    a = b;
  }
  EG_HIP(hipMemcpy(perm_d, perm.data(), (size_t)nv * 8, hipMemcpyHostToDevice));
  EG_HIP(hipMemcpy(head_d, head.data(), (size_t)nv * 8, hipMemcpyHostToDevice));
  return EULER_GPU_OK;
}

// The index over m entries (id_d, beg_d, len_d) whose bytes live in val_d [val_bytes].  On
// success the graph's old index (if any) is replaced; on failure it is left as it was and every
// allocation of this build is returned.
int BuildIndex(const euler_gpu_graph* g, int64_t m, const uint64_t* id_d, const int64_t* beg_d,
               const int32_t* len_d, const uint8_t* val_d, int64_t val_bytes, bool check_dups) {
  if (m >= ((int64_t)1 << 31)) return Fail(EULER_GPU_EINVAL, "graph labels: more than 2^31 nodes");
  const int bits = g_label_hash_bits;
  // scratch: 12 arrays of m (+ 1) words and the counters
  DevBuf ws;
  const size_t per = (size_t)(std::max<int64_t>(m, 1) * 8 + 32);
  EG_HIP(ws.alloc(per * 13 + 64));
  uint8_t* at = ws.as<uint8_t>();
  uint64_t* key = Carve<uint64_t>(at, m);
  uint64_t* key2 = Carve<uint64_t>(at, m + 1);
  int64_t* iota = Carve<int64_t>(at, m);
  int64_t* perm1 = Carve<int64_t>(at, m);
  int64_t* perm2 = Carve<int64_t>(at, m);
  int64_t* head = Carve<int64_t>(at, m + 1);
  int64_t* excl = Carve<int64_t>(at, m + 1);
  int64_t* seg_of = Carve<int64_t>(at, m);
  int64_t* seg_head = Carve<int64_t>(at, m);
  uint64_t* seg_min = Carve<uint64_t>(at, m);
  int64_t* seg_iota = Carve<int64_t>(at, m);
  uint64_t* sorted_id = Carve<uint64_t>(at, m);
  unsigned long long* cnt = Carve<unsigned long long>(at, 4);   // valid, dups, collisions
  EG_HIP(hipMemset(cnt, 0, 32));
  const int grid = GridFor(m, 256);
  hipLaunchKernelGGL(HashKernel, dim3(grid), dim3(256), 0, 0, val_d, beg_d, len_d, m, bits, key,
                     iota, cnt);
  int rc = CheckLaunch("graph labels: hash");
  if (rc != EULER_GPU_OK) return rc;
  // (hash, id) order: by id, then stably by hash
  rc = SortPairs<uint64_t, int64_t>(id_d, sorted_id, iota, perm1, m, 64);
  if (rc != EULER_GPU_OK) return rc;
  if (check_dups) {
    hipLaunchKernelGGL(DupIdsKernel, dim3(grid), dim3(256), 0, 0, sorted_id, perm1, len_d, m, cnt + 1);
    rc = CheckLaunch("graph labels: duplicate ids");
    if (rc != EULER_GPU_OK) return rc;
  }
  hipLaunchKernelGGL(GatherKernel<uint64_t>, dim3(grid), dim3(256), 0, 0, key, perm1, m, key2);
  rc = CheckLaunch("graph labels: gather");
  if (rc == EULER_GPU_OK) rc = SortPairs<uint64_t, int64_t>(key2, key, perm1, perm2, m, 64);
  if (rc != EULER_GPU_OK) return rc;
  unsigned long long c[3] = {0, 0, 0};
  EG_HIP(hipMemcpy(c, cnt, 24, hipMemcpyDeviceToHost));
  if (c[1]) return Fail(EULER_GPU_EINVAL, "set_graph_labels: a node id is listed twice");
  const int64_t nv = (int64_t)c[0];
  if (nv > 0) {
    hipLaunchKernelGGL(HeadsKernel, dim3(GridFor(nv, 256)), dim3(256), 0, 0, key, perm2, val_d, beg_d,
                       len_d, nv, head, cnt + 2);
    rc = CheckLaunch("graph labels: heads");
    if (rc != EULER_GPU_OK) return rc;
    EG_HIP(hipMemcpy(&c[2], cnt + 2, 8, hipMemcpyDeviceToHost));
    if (c[2]) rc = SplitCollisions(m, nv, key, perm2, head, val_d, val_bytes, beg_d, len_d);
    if (rc != EULER_GPU_OK) return rc;
  }
  EG_HIP(hipMemset(head + nv, 0, 8));
  rc = ExclusiveScanI64(0, head, excl, nv + 1);
  if (rc != EULER_GPU_OK) return rc;
  int64_t L = 0;
  EG_HIP(hipMemcpy(&L, excl + nv, 8, hipMemcpyDeviceToHost));
  if (L == 0) {                          // no labels: an empty index, no device memory
    euler_gpu_graph* mg = const_cast<euler_gpu_graph*>(g);
    (void)hipDeviceSynchronize();
    DestroyLabelIndex(mg);
    g->label_off_host.assign(1, 0);
    g->labels_ready = true;
    return EULER_GPU_OK;
  }
  // the index itself
  AllocList a("graph labels: ");
  uint64_t* nodes = a.Alloc<uint64_t>((size_t)nv);
  int64_t* start = nodes ? a.Alloc<int64_t>((size_t)L + 1) : nullptr;
  if (!start) { a.Release(); return a.rc; }
  // the labels' bytes pass through the device once, in scratch: export and lookup are host work
  DevBuf boff_s, bytes_s;
  if (boff_s.alloc(((size_t)L + 1) * 8) != hipSuccess) {
    a.Release();
    return Fail(EULER_GPU_ENOMEM, "graph labels: byte offsets");
  }
  int64_t* boff = boff_s.as<int64_t>();
  std::vector<int64_t> boff_h;
  std::vector<uint8_t> bytes_h;
  if (nv > 0) {
    hipLaunchKernelGGL(SegmentsKernel, dim3(GridFor(nv, 256)), dim3(256), 0, 0, head, excl, perm2,
                       id_d, nv, seg_of, seg_head, seg_min, seg_iota);
    rc = CheckLaunch("graph labels: segments");
    // table order: by the smallest id of a label (Q14); the reused arrays: order -> perm1,
    // rank -> iota, sizes -> key2 (as int64), byte lengths -> excl
    if (rc == EULER_GPU_OK) rc = SortPairs<uint64_t, int64_t>(seg_min, key, seg_iota, perm1, L, 64);
    int64_t* order = perm1;
    int64_t* rank = iota;
    int64_t* size = reinterpret_cast<int64_t*>(key2);
    int64_t* blen = excl;
    if (rc == EULER_GPU_OK) {
      hipLaunchKernelGGL(LabelSizesKernel, dim3(GridFor(L, 256)), dim3(256), 0, 0, order, seg_head,
                         perm2, len_d, L, nv, rank, size, blen);
      rc = CheckLaunch("graph labels: sizes");
    }
    if (rc == EULER_GPU_OK) {
      (void)hipMemset(size + L, 0, 8);
      (void)hipMemset(blen + L, 0, 8);
      rc = ExclusiveScanI64(0, size, start, L + 1);
    }
    if (rc == EULER_GPU_OK) rc = ExclusiveScanI64(0, blen, boff, L + 1);
    if (rc == EULER_GPU_OK) {
      hipLaunchKernelGGL(PlaceNodesKernel, dim3(GridFor(nv, 256)), dim3(256), 0, 0, seg_of, seg_head,
                         rank, start, perm2, id_d, nv, nodes);
      rc = CheckLaunch("graph labels: nodes");
    }
    if (rc == EULER_GPU_OK) rc = Download(&boff_h, (const int64_t*)boff, L + 1);
    uint8_t* lbytes = nullptr;
    if (rc == EULER_GPU_OK) {
      if (bytes_s.alloc((size_t)boff_h[L] + 16) == hipSuccess) lbytes = bytes_s.as<uint8_t>();
      else rc = Fail(EULER_GPU_ENOMEM, "graph labels: label bytes");
    }
    if (lbytes) {
      hipLaunchKernelGGL(LabelBytesKernel, dim3(GridFor(L * 64, 256)), dim3(256), 0, 0, order,
                         seg_head, perm2, val_d, beg_d, boff, L, lbytes);
      rc = CheckLaunch("graph labels: bytes");
      if (rc == EULER_GPU_OK) rc = Download(&bytes_h, (const uint8_t*)lbytes, boff_h[L]);
    }
    if (rc != EULER_GPU_OK) { a.Release(); return rc; }
  } else {
    boff_h.assign(1, 0);
    (void)hipMemset(start, 0, 8);
    (void)hipMemset(boff, 0, 8);
  }
  std::map<std::string, int64_t> lookup;
  for (int64_t r = 0; r < L; ++r)
    lookup.emplace(std::string(reinterpret_cast<const char*>(bytes_h.data()) + boff_h[r],
                               (size_t)(boff_h[r + 1] - boff_h[r])), r);
  // replace the old index
  euler_gpu_graph* mg = const_cast<euler_gpu_graph*>(g);
  (void)hipDeviceSynchronize();          // (no launch may still read the old index)
  DestroyLabelIndex(mg);
  mg->bytes += a.HandOver(&mg->label_allocs);
  g->label_nodes = nodes;
  g->label_start = start;
  g->n_labels = L;
  g->n_labelled = nv;
  g->label_off_host.swap(boff_h);
  g->label_bytes_host.swap(bytes_h);
  g->label_lookup.swap(lookup);
  g->labels_ready = true;
  return EULER_GPU_OK;
}

// The index of a loaded dataset, on first use (caller holds label_mu).
int EnsureLabelIndexLocked(const euler_gpu_graph* g, const char* what) {
  if (g->labels_ready) return EULER_GPU_OK;
  if (g->shards > 1)
    return Fail(EULER_GPU_EINVAL, std::string(what) + ": graph labels of a sharded graph are not "
                                  "supported (each shard holds only part of every graph)");
  const int64_t n = g->view.n_rows;
  if (g->label_slot < 0 || n == 0)
    return Fail(EULER_GPU_EEMPTY, std::string(what) + ": the graph has no graph labels "
                                  "(binary_graph_label / set_graph_labels)");
  int rc = EnsureNodeBinary(g);
  if (rc != EULER_GPU_OK) return rc;
  DeviceGuard dg(g->device);
  DevBuf ent;
  EG_HIP(ent.alloc((size_t)n * 20 + 64));
  uint64_t* id = ent.as<uint64_t>();
  int64_t* beg = reinterpret_cast<int64_t*>(id + n);
  int32_t* len = reinterpret_cast<int32_t*>(beg + n);
  hipLaunchKernelGGL(EntriesFromSlotKernel, dim3(GridFor(n, 256)), dim3(256), 0, 0, g->view,
                     g->node_bin, g->label_slot, id, beg, len);
  rc = CheckLaunch("graph labels: entries");
  if (rc != EULER_GPU_OK) return rc;
  const int64_t val_bytes = g->bin_host_val.size();
  rc = BuildIndex(g, n, id, beg, len, static_cast<const uint8_t*>(g->node_bin.val), val_bytes, false);
  if (rc != EULER_GPU_OK) return rc;
  if (g->n_labels == 0) {
    g->labels_ready = false;
    DestroyLabelIndex(const_cast<euler_gpu_graph*>(g));
    return Fail(EULER_GPU_EEMPTY, std::string(what) + ": the graph has no graph labels");
  }
  return EULER_GPU_OK;
}

// The index, built if need be, with label_mu held by *lk on return: a caller that launches on the
// index keeps the lock until its launches are enqueued, so a concurrent set_graph_labels (which
// takes the lock, drains the device and only then frees the old arrays) cannot free them between.
int EnsureLabelIndex(const euler_gpu_graph* g, const char* what, std::unique_lock<std::mutex>* lk) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, std::string(what) + ": null graph");
  *lk = std::unique_lock<std::mutex>(g->label_mu);
  const int rc = EnsureLabelIndexLocked(g, what);
  if (rc == EULER_GPU_OK && g->n_labels == 0)
    return Fail(EULER_GPU_EEMPTY, std::string(what) + ": the graph has no graph labels");
  return rc;
}

// ------------------------------------------------------------ label queries
__global__ __launch_bounds__(256) void SampleGraphLabelKernel(uint64_t seed, uint32_t call_id,
                                                              int64_t L, int32_t count,
                                                              int64_t* out) {
  const int32_t stride = gridDim.x * blockDim.x;
  for (int32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < count; j += stride) {
    const double u = RngDraw(seed, call_id, kDomainGraphLabel, 0, (uint64_t)j);
    int64_t r = (int64_t)(u * (double)L);
    out[j] = r < L - 1 ? r : L - 1;
  }
}

__global__ __launch_bounds__(256) void LabelCountKernel(const int64_t* ids, int64_t n,
                                                        const int64_t* start, int64_t L,
                                                        int64_t* counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t r = ids[i];
    counts[i] = (r >= 0 && r < L) ? start[r + 1] - start[r] : 0;
  }
}

__global__ __launch_bounds__(256) void LabelIdxKernel(const int64_t* off, int64_t n, int32_t* idx) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    idx[2 * i] = (int32_t)off[i];
    idx[2 * i + 1] = (int32_t)off[i + 1];
  }
}

// one wave per asked label
__global__ __launch_bounds__(256) void LabelFillKernel(const int64_t* ids, int64_t n,
                                                       const int64_t* start, const uint64_t* nodes,
                                                       int64_t L, const int32_t* idx, uint64_t* out) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += n_waves) {
    const int64_t r = ids[i];
    if (r < 0 || r >= L) continue;
    const int64_t b = start[r];
    const int32_t o = idx[2 * i], l = idx[2 * i + 1] - o;
    for (int32_t k = lane; k < l; k += 64) out[o + k] = nodes[b + k];
  }
}

// ------------------------------------------------------------ whole-graph block
// Batch ids -> positions: the positions sorted by id (spos), and an open-addressing table of
// 16-byte slots {id, first position in spos | run length << 32}; length 0 = empty slot.
struct PosSlot {
  uint64_t key;
  uint64_t run;     // start | len << 32
};

__global__ __launch_bounds__(256) void PosInsertKernel(const uint64_t* sid, int64_t n, PosSlot* table,
                                                       uint64_t mask) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t id = sid[i];
    if (i > 0 && sid[i - 1] == id) continue;
    int64_t e = i + 1;
    while (e < n && sid[e] == id) ++e;
    const uint64_t run = (uint64_t)i | ((uint64_t)(e - i) << 32);
    uint64_t h = Mix64(id) & mask;
    for (uint64_t p = 0; p <= mask; ++p) {
      const unsigned long long old = atomicCAS(
          reinterpret_cast<unsigned long long*>(&table[h].run), 0ULL, (unsigned long long)run);
      if (old == 0ULL) { table[h].key = id; break; }
      h = (h + 1) & mask;
    }
  }
}

__device__ __forceinline__ uint64_t PosFind(const PosSlot* table, uint64_t mask, uint64_t id) {
  uint64_t h = Mix64(id) & mask;
  for (uint64_t p = 0; p <= mask; ++p) {
    const PosSlot s = table[h];
    if (s.run == 0) return 0;
    if (s.key == id) return s.run;
    h = (h + 1) & mask;
  }
  return 0;
}

struct BlockArgs {
  GraphView g;
  int32_t k;
  int32_t et[kMaxListedTypes];
};

// listed out-edges of every batch position (0 for an unknown id)
__global__ __launch_bounds__(256) void BlockRowsKernel(const BlockArgs a, const uint64_t* nid, int64_t n,
                                                       int64_t* row, int64_t* cnt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    const int64_t r = FindRow(a.g, nid[j]);
    int64_t d = 0;
    if (r >= 0) {
      const RowMeta rm = LoadRowMeta(a.g, r);
      for (int32_t x = 0; x < a.k; ++x) {
        const int32_t t = a.et[x];
        if (t >= 0 && t < a.g.T) d += rm.type_end[t] - (t == 0 ? 0 : rm.type_end[t - 1]);
      }
    }
    row[j] = r;
    cnt[j] = d;
  }
}

// Listed edge e of the batch: its source position (the last eoff <= e), its neighbour.  A lane
// per listed edge: a hub row is spread over as many lanes as it has edges.
__device__ __forceinline__ uint64_t ListedEdge(const BlockArgs& a, const int64_t* eoff, int64_t n,
                                               const int64_t* row, int64_t e, int64_t* j_out) {
  int64_t lo = 0, hi = n - 1;               // eoff[lo] <= e < eoff[hi + 1]
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (eoff[mid] <= e) lo = mid; else hi = mid - 1;
  }
  *j_out = lo;
  int64_t local = e - eoff[lo];
  const RowMeta rm = LoadRowMeta(a.g, row[lo]);
  for (int32_t x = 0; x < a.k; ++x) {
    const int32_t t = a.et[x];
    if (t < 0 || t >= a.g.T) continue;
    const int32_t b = t == 0 ? 0 : rm.type_end[t - 1];
    const int64_t d = rm.type_end[t] - b;
    if (local < d) return a.g.nbr[rm.row_ptr + b + local];
    local -= d;
  }
  return 0;   // not reached
}

__global__ __launch_bounds__(256) void BlockHitsKernel(const BlockArgs a, const int64_t* eoff, int64_t n,
                                                       const int64_t* row, int64_t lam,
                                                       const PosSlot* table, uint64_t mask,
                                                       int64_t* hits) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < lam; e += stride) {
    int64_t j;
    const uint64_t run = PosFind(table, mask, ListedEdge(a, eoff, n, row, e, &j));
    hits[e] = (int64_t)(run >> 32);
  }
}

__global__ __launch_bounds__(256) void BlockFillKernel(const BlockArgs a, const int64_t* eoff, int64_t n,
                                                       const int64_t* row, int64_t lam,
                                                       const PosSlot* table, uint64_t mask,
                                                       const int64_t* spos, const int64_t* hoff,
                                                       uint64_t* keys) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < lam; e += stride) {
    if (hoff[e + 1] == hoff[e]) continue;
    int64_t j;
    const uint64_t run = PosFind(table, mask, ListedEdge(a, eoff, n, row, e, &j));
    const int64_t s = (int64_t)(run & 0xffffffffULL), l = (int64_t)(run >> 32);
    const int64_t o = hoff[e];
    for (int64_t t = 0; t < l; ++t) keys[o + t] = ((uint64_t)j << 32) | (uint64_t)spos[s + t];
  }
}

__global__ __launch_bounds__(256) void BlockOutKernel(const uint64_t* keys, int64_t E, int64_t n,
                                                      int32_t loops, int64_t cap, int64_t* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t total = E + (loops ? n : 0);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int64_t s, d;
    if (i < E) { s = (int64_t)(keys[i] >> 32); d = (int64_t)(keys[i] & 0xffffffffULL); }
    else { s = d = i - E; }
    out[i] = s;
    out[cap + i] = d;
  }
}

__global__ __launch_bounds__(256) void IotaKernel(int64_t* p, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = i;
}

int BitsFor(int64_t n) {
  int b = 1;
  while (b < 63 && ((int64_t)1 << b) <= n) ++b;
  return b;
}

template <typename K, typename V>
int SortPairsAsync(hipStream_t st, const K* kin, K* kout, const V* vin, V* vout, int64_t n,
                   int end_bit) {
  size_t tmp_bytes = 0;
  EG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, kin, kout, vin, vout, (int)n, 0,
                                            end_bit, st));
  StreamBuf tmp(st);
  EG_HIP(tmp.alloc(tmp_bytes + 16));
  EG_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.as(), tmp_bytes, kin, kout, vin, vout, (int)n, 0,
                                            end_bit, st));
  return EULER_GPU_OK;
}

}  // namespace

void DestroyLabelIndex(euler_gpu_graph* g) {
  g->bytes -= FreeBlocks(&g->label_allocs);
  g->label_nodes = nullptr;
  g->label_start = nullptr;
  g->n_labels = 0;
  g->n_labelled = 0;
  g->labels_ready = false;
  g->label_off_host.clear();
  g->label_bytes_host.clear();
  g->label_lookup.clear();
}

}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_graph_set_graph_labels(euler_gpu_graph* g, const uint64_t* ids_host, int64_t n,
                                     const int64_t* offsets_host, const uint8_t* bytes_host) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "set_graph_labels: null graph");
  if (n < 0 || (n > 0 && (!ids_host || !offsets_host)))
    return Fail(EULER_GPU_EINVAL, "set_graph_labels: bad arguments");
  if (g->shards > 1)
    return Fail(EULER_GPU_EINVAL, "set_graph_labels: graph labels of a sharded graph are not supported");
  const int64_t nb = n > 0 ? offsets_host[n] : 0;
  for (int64_t i = 0; i < n; ++i)
    if (offsets_host[i] < 0 || offsets_host[i + 1] < offsets_host[i] || offsets_host[i + 1] - offsets_host[i] > INT32_MAX)
      return Fail(EULER_GPU_EINVAL, "set_graph_labels: offsets must be non-decreasing from 0");
  if (n > 0 && offsets_host[0] != 0) return Fail(EULER_GPU_EINVAL, "set_graph_labels: offsets[0] != 0");
  if (nb > 0 && !bytes_host) return Fail(EULER_GPU_EINVAL, "set_graph_labels: null bytes");
  std::lock_guard<std::mutex> lk(g->label_mu);
  DeviceGuard dg(g->device);
  std::vector<int64_t> beg(offsets_host, offsets_host + n);
  std::vector<int32_t> len((size_t)n);
  for (int64_t i = 0; i < n; ++i) len[i] = (int32_t)(offsets_host[i + 1] - offsets_host[i]);
  DevBuf ent;
  const size_t bad_at = ((size_t)n * 20 + 15) & ~(size_t)15;     // 8-byte aligned counter
  EG_HIP(ent.alloc(bad_at + 16 + (size_t)nb + 64));
  uint64_t* id = ent.as<uint64_t>();
  int64_t* bg = reinterpret_cast<int64_t*>(id + n);
  int32_t* ln = reinterpret_cast<int32_t*>(bg + n);
  unsigned long long* bad = reinterpret_cast<unsigned long long*>(ent.as<uint8_t>() + bad_at);
  uint8_t* val = reinterpret_cast<uint8_t*>(bad) + 16;
  EG_HIP(hipMemset(bad, 0, 8));
  if (n > 0) {
    EG_HIP(hipMemcpy(id, ids_host, (size_t)n * 8, hipMemcpyHostToDevice));
    EG_HIP(hipMemcpy(bg, beg.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    EG_HIP(hipMemcpy(ln, len.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  }
  if (nb > 0) EG_HIP(hipMemcpy(val, bytes_host, (size_t)nb, hipMemcpyHostToDevice));
  if (n > 0) {
    hipLaunchKernelGGL(CheckIdsKernel, dim3(GridFor(n, 256)), dim3(256), 0, 0, g->view, id, n, bad);
    int rc = CheckLaunch("set_graph_labels: ids");
    if (rc != EULER_GPU_OK) return rc;
  }
  unsigned long long misses = 0;
  EG_HIP(hipMemcpy(&misses, bad, 8, hipMemcpyDeviceToHost));
  if (misses)
    return Fail(EULER_GPU_EINVAL, "set_graph_labels: " + std::to_string(misses) +
                                  " node id(s) not in the graph");
  return BuildIndex(g, n, id, bg, ln, val, nb, true);
}

int64_t euler_gpu_graph_num_graph_labels(const euler_gpu_graph* g) {
  std::unique_lock<std::mutex> lk;
  const int rc = EnsureLabelIndex(g, "num_graph_labels", &lk);
  if (rc == EULER_GPU_EEMPTY) return 0;
  return rc == EULER_GPU_OK ? g->n_labels : rc;
}

int euler_gpu_graph_export_graph_labels(const euler_gpu_graph* g, int64_t* offsets_host,
                                        uint8_t* bytes_host) {
  std::unique_lock<std::mutex> lk;
  const int rc = EnsureLabelIndex(g, "export_graph_labels", &lk);
  if (rc != EULER_GPU_OK) return rc;
  if (!offsets_host) return Fail(EULER_GPU_EINVAL, "export_graph_labels: null offsets");
  std::memcpy(offsets_host, g->label_off_host.data(), (size_t)(g->n_labels + 1) * 8);
  if (bytes_host && !g->label_bytes_host.empty())
    std::memcpy(bytes_host, g->label_bytes_host.data(), g->label_bytes_host.size());
  return EULER_GPU_OK;
}

int euler_gpu_graph_label_ids(const euler_gpu_graph* g, int64_t n, const int64_t* offsets_host,
                              const uint8_t* bytes_host, int64_t* out_host) {
  std::unique_lock<std::mutex> lk;
  const int rc = EnsureLabelIndex(g, "graph_label_ids", &lk);
  if (rc != EULER_GPU_OK) return rc;
  if (n < 0 || (n > 0 && (!offsets_host || !out_host)))
    return Fail(EULER_GPU_EINVAL, "graph_label_ids: bad arguments");
  for (int64_t i = 0; i < n; ++i) {
    const std::string s(reinterpret_cast<const char*>(bytes_host) + offsets_host[i],
                        (size_t)(offsets_host[i + 1] - offsets_host[i]));
    auto it = g->label_lookup.find(s);
    out_host[i] = it == g->label_lookup.end() ? -1 : it->second;
  }
  return EULER_GPU_OK;
}

int euler_gpu_graph_label_index_info(const euler_gpu_graph* g, int64_t* n_labelled_host,
                                     int64_t* index_bytes_host) {
  std::unique_lock<std::mutex> lk;
  const int rc = EnsureLabelIndex(g, "label_index_info", &lk);
  if (rc != EULER_GPU_OK) return rc;
  int64_t b = 0;
  for (auto& p : g->label_allocs) b += p.second;
  if (n_labelled_host) *n_labelled_host = g->n_labelled;
  if (index_bytes_host) *index_bytes_host = b;
  return EULER_GPU_OK;
}

int euler_gpu_sample_graph_label(const euler_gpu_graph* g, void* stream, uint64_t seed,
                                 uint32_t call_id, int32_t count, int64_t* out_dev) {
  std::unique_lock<std::mutex> lk;
  const int rc = EnsureLabelIndex(g, "sample_graph_label", &lk);
  if (rc != EULER_GPU_OK) return rc;
  if (count < 0) return Fail(EULER_GPU_EINVAL, "sample_graph_label: count < 0");
  if (count == 0) return EULER_GPU_OK;
  if (!out_dev) return Fail(EULER_GPU_EINVAL, "sample_graph_label: null output");
  hipLaunchKernelGGL(SampleGraphLabelKernel, dim3(GridFor(count, 256)), dim3(256), 0,
                     (hipStream_t)stream, seed, call_id, g->n_labels, count, out_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_get_graph_by_label(const euler_gpu_graph* g, void* stream, const int64_t* label_ids_dev,
                                 int64_t n, int32_t* idx_dev, int64_t* total_host, uint64_t* out_dev) {
  std::unique_lock<std::mutex> lk;
  int rc = EnsureLabelIndex(g, "get_graph_by_label", &lk);
  if (rc != EULER_GPU_OK) return rc;
  if (n < 0 || (n > 0 && (!label_ids_dev || !idx_dev)))
    return Fail(EULER_GPU_EINVAL, "get_graph_by_label: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (out_dev == nullptr) {
    if (n == 0) { if (total_host) *total_host = 0; return EULER_GPU_OK; }
    StreamBuf scratch(st);
    EG_HIP(scratch.alloc((size_t)(2 * n + 2) * 8));
    int64_t* counts = scratch.as<int64_t>();
    int64_t* off = counts + n + 1;
    EG_HIP(hipMemsetAsync(counts + n, 0, 8, st));
    hipLaunchKernelGGL(LabelCountKernel, dim3(GridFor(n, 256)), dim3(256), 0, st, label_ids_dev, n,
                       g->label_start, g->n_labels, counts);
    rc = ExclusiveScanI64(st, counts, off, n + 1);
    if (rc != EULER_GPU_OK) return rc;
    int64_t total = 0;
    EG_HIP(hipMemcpyAsync(&total, off + n, 8, hipMemcpyDeviceToHost, st));
    EG_HIP(hipStreamSynchronize(st));
    if (total > INT32_MAX) return Fail(EULER_GPU_EINVAL, "get_graph_by_label: more than 2^31 nodes");
    hipLaunchKernelGGL(LabelIdxKernel, dim3(GridFor(n, 256)), dim3(256), 0, st, off, n, idx_dev);
    EG_HIP(hipGetLastError());
    if (total_host) *total_host = total;
    return EULER_GPU_OK;
  }
  if (n == 0) return EULER_GPU_OK;
  hipLaunchKernelGGL(LabelFillKernel, dim3(GridFor(n * 64, 256)), dim3(256), 0, st, label_ids_dev, n,
                     g->label_start, g->label_nodes, g->n_labels, idx_dev, out_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_whole_graph_block(const euler_gpu_graph* g, void* stream, const uint64_t* nodes_dev,
                                int64_t n, const int32_t* edge_types_host, int32_t k,
                                int32_t add_self_loops, int64_t cap, int64_t* total_host,
                                int64_t* out_dev) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "whole_graph_block: null graph");
  if (n < 0 || k < 0 || k > kMaxListedTypes || (k > 0 && !edge_types_host) || (n > 0 && !nodes_dev) ||
      !total_host || cap < 0 || (cap > 0 && !out_dev))
    return Fail(EULER_GPU_EINVAL, "whole_graph_block: bad arguments");
  if (n >= ((int64_t)1 << 31)) return Fail(EULER_GPU_EINVAL, "whole_graph_block: more than 2^31 nodes");
  hipStream_t st = (hipStream_t)stream;
  BlockArgs a{};
  a.g = g->view;
  a.k = k;
  for (int32_t x = 0; x < k; ++x) a.et[x] = edge_types_host[x];
  const int64_t loops = add_self_loops ? n : 0;
  if (n == 0) { *total_host = 0; return EULER_GPU_OK; }
  // positions by id and their table
  uint64_t tcap = 16;
  while (tcap < 2 * (uint64_t)n) tcap <<= 1;
  StreamBuf ws(st);
  const size_t bytes = (size_t)n * 8 * 6 + 256 + tcap * sizeof(PosSlot);   // (Carve pads each array)
  EG_HIP(ws.alloc(bytes));
  uint8_t* at = ws.as<uint8_t>();
  uint64_t* sid = Carve<uint64_t>(at, n);
  int64_t* iota = Carve<int64_t>(at, n);
  int64_t* spos = Carve<int64_t>(at, n);
  int64_t* row = Carve<int64_t>(at, n);
  int64_t* eoff = Carve<int64_t>(at, n + 1);
  int64_t* cnt = Carve<int64_t>(at, n + 1);
  PosSlot* table = reinterpret_cast<PosSlot*>(at);
  const uint64_t mask = tcap - 1;
  EG_HIP(hipMemsetAsync(table, 0, tcap * sizeof(PosSlot), st));
  EG_HIP(hipMemsetAsync(cnt + n, 0, 8, st));
  hipLaunchKernelGGL(IotaKernel, dim3(GridFor(n, 256)), dim3(256), 0, st, iota, n);
  int rc = SortPairsAsync<uint64_t, int64_t>(st, nodes_dev, sid, iota, spos, n, 64);
  if (rc != EULER_GPU_OK) return rc;
  hipLaunchKernelGGL(PosInsertKernel, dim3(GridFor(n, 256)), dim3(256), 0, st, sid, n, table, mask);
  hipLaunchKernelGGL(BlockRowsKernel, dim3(GridFor(n, 256)), dim3(256), 0, st, a, nodes_dev, n, row, cnt);
  rc = ExclusiveScanI64(st, cnt, eoff, n + 1);
  if (rc != EULER_GPU_OK) return rc;
  int64_t lam = 0;
  EG_HIP(hipMemcpyAsync(&lam, eoff + n, 8, hipMemcpyDeviceToHost, st));
  EG_HIP(hipStreamSynchronize(st));                         // host read 1: listed edges
  if (lam >= ((int64_t)1 << 31)) return Fail(EULER_GPU_EINVAL, "whole_graph_block: more than 2^31 listed edges");
  int64_t E = 0;
  StreamBuf ws2(st);
  if (lam > 0) {
    EG_HIP(ws2.alloc((size_t)(lam + 1) * 16 + 64));
    int64_t* hits = ws2.as<int64_t>();
    int64_t* hoff = hits + lam + 1;
    EG_HIP(hipMemsetAsync(hits + lam, 0, 8, st));
    hipLaunchKernelGGL(BlockHitsKernel, dim3(GridFor(lam, 256)), dim3(256), 0, st, a, eoff, n, row, lam,
                       table, mask, hits);
    rc = ExclusiveScanI64(st, hits, hoff, lam + 1);
    if (rc != EULER_GPU_OK) return rc;
    EG_HIP(hipMemcpyAsync(&E, hoff + lam, 8, hipMemcpyDeviceToHost, st));
    EG_HIP(hipStreamSynchronize(st));                       // host read 2: hits
    if (E >= ((int64_t)1 << 31)) return Fail(EULER_GPU_EINVAL, "whole_graph_block: more than 2^31 hits");
    if (E > 0) {
      // (j, c) keys, sorted; a neighbour listed twice in a row (two edge types, or a repeated
      // edge) is one pair, as in SparseGetAdj's mask
      StreamBuf ks(st);
      EG_HIP(ks.alloc((size_t)E * 16 + 64));
      uint64_t* keys = ks.as<uint64_t>();
      uint64_t* skeys = keys + E;
      int64_t* n_sel = reinterpret_cast<int64_t*>(skeys + E);
      hipLaunchKernelGGL(BlockFillKernel, dim3(GridFor(lam, 256)), dim3(256), 0, st, a, eoff, n, row, lam,
                         table, mask, spos, hoff, keys);
      size_t sort_bytes = 0, uniq_bytes = 0;
      const int end_bit = 32 + BitsFor(n);
      EG_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, keys, skeys, (int)E, 0, end_bit, st));
      EG_HIP(hipcub::DeviceSelect::Unique(nullptr, uniq_bytes, skeys, keys, n_sel, (int)E, st));
      StreamBuf tmp(st);
      EG_HIP(tmp.alloc(std::max(sort_bytes, uniq_bytes) + 16));
      EG_HIP(hipcub::DeviceRadixSort::SortKeys(tmp.as(), sort_bytes, keys, skeys, (int)E, 0, end_bit, st));
      EG_HIP(hipcub::DeviceSelect::Unique(tmp.as(), uniq_bytes, skeys, keys, n_sel, (int)E, st));
      EG_HIP(hipMemcpyAsync(&E, n_sel, 8, hipMemcpyDeviceToHost, st));
      EG_HIP(hipStreamSynchronize(st));                     // host read 3: block edges
      *total_host = E + loops;
      if (E + loops > cap) return EULER_GPU_OK;             // the caller asks again with room
      hipLaunchKernelGGL(BlockOutKernel, dim3(GridFor(E + loops, 256)), dim3(256), 0, st, keys, E, n,
                         add_self_loops ? 1 : 0, cap, out_dev);
      EG_HIP(hipGetLastError());
      return EULER_GPU_OK;
    }
  }
  *total_host = E + loops;
  if (E + loops > cap) return EULER_GPU_OK;
  if (loops > 0)
    hipLaunchKernelGGL(BlockOutKernel, dim3(GridFor(loops, 256)), dim3(256), 0, st, nullptr, 0, n, 1, cap,
                       out_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

}  // extern "C"
