// Alias-table neighbour sampling, the opt-in O(1) draw mode: the device build of the neighbour
// alias tables (nb_alias.h: one 32-byte entry per edge), their export, and the draw kernel with the
// entry points euler_gpu_sample_neighbor_alias / euler_gpu_sample_fanout_alias.  The exact mode
// (sample_kernels.hip) is the reference's CDF inversion and stays the default; this mode picks
// different neighbours for the same uniforms and is validated statistically.
//
// The mode builds and reads nothing but the flat arrays and its own tables: no weight-bucket index,
// no side index, no EdgeBlocks.
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "device_mem.h"
#include "nb_alias_draw.h"

namespace euler_gpu {

namespace {

// ---- build: one lane per (row, edge-type group), sequential inside a group as the algorithm is.
// scratch: one int32 per edge - the two stacks of a group grow from the two ends of its slice.
__global__ __launch_bounds__(256) void NbAliasBuildKernel(GraphView g, NbAliasEntry* tab, int32_t* scratch) {
  const int64_t groups = g.n_rows * (int64_t)g.T;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += stride) {
    const int64_t row = i / g.T;
    const int32_t t = (int32_t)(i - row * g.T);
    const RowMeta m = LoadRowMeta(g, row);
    const int32_t b = t == 0 ? 0 : m.type_end[t - 1];
    const int32_t d = m.type_end[t] - b;
    if (d <= 0) continue;
    const int64_t first = m.row_ptr + b;
    const float before = b == 0 ? 0.f : g.prefix_w[first - 1];
    (void)NbAliasBuildGroup(tab + first, scratch + first, g.nbr + first, g.prefix_w + first, before, d);
  }
}

// The allocations of one build; whatever was not handed to the graph goes back with it.
struct TableBuild : AllocList {
  TableBuild() : AllocList("neighbor alias: ") {}
  ~TableBuild() { Release(); }
};

int BuildNbAlias(euler_gpu_graph* g, hipStream_t stream) {
  const GraphView& v = g->view;
  if (v.monotone == 0)
    return Fail(EULER_GPU_EINVAL, "neighbor alias: the graph has rows with negative or NaN weights "
                                  "(running sums that decrease); the alias mode refuses them");
  DeviceGuard dg(g->device);
  TableBuild tb;
  DevBuf scratch;
  const size_t E = (size_t)v.n_edges;
  NbAliasEntry* tab = tb.Alloc<NbAliasEntry>(E);
  if (!tab) return tb.rc;
  if (E > 0) {
    EG_HIP(scratch.alloc(E * sizeof(int32_t)));
    // (entries no group covers - there are none in a well-formed graph - read as "no table")
    EG_HIP(hipMemsetAsync(tab, 0, E * sizeof(NbAliasEntry), stream));
    hipLaunchKernelGGL(NbAliasBuildKernel, dim3(GridFor(v.n_rows * (int64_t)v.T, 256)), dim3(256), 0, stream,
                       v, tab, scratch.as<int32_t>());
    EG_HIP(hipGetLastError());
    // the scratch is released before the call returns, so the build has to have finished
    EG_HIP(hipStreamSynchronize(stream));
  }
  g->nb_alias_bytes = tb.list.empty() ? 0 : tb.list.back().second;
  AdoptBlocks(g, &tb);
  g->nb_alias.store(tab, std::memory_order_release);
  return EULER_GPU_OK;
}

// The tables, built on first use under the graph's mutex: concurrent callers wait for the build.
int EnsureNbAlias(const euler_gpu_graph* cg, hipStream_t stream, const NbAliasEntry** tab) {
  euler_gpu_graph* g = const_cast<euler_gpu_graph*>(cg);
  *tab = g->nb_alias.load(std::memory_order_acquire);
  if (*tab != nullptr) return EULER_GPU_OK;
  std::lock_guard<std::mutex> lk(g->nb_alias_mu);
  *tab = g->nb_alias.load(std::memory_order_acquire);
  if (*tab != nullptr) return EULER_GPU_OK;
  const int rc = BuildNbAlias(g, stream);
  *tab = g->nb_alias.load(std::memory_order_acquire);
  return rc;
}

__global__ void NbAliasExportMetaKernel(GraphView g, const uint64_t* ids, int64_t n, int64_t* deg,
                                        int64_t* off) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t row = FindRow(g, ids[i]);
  if (row < 0) { deg[i] = 0; off[i] = 0; return; }
  const RowMeta m = LoadRowMeta(g, row);
  deg[i] = m.type_end[g.T - 1];
  off[i] = m.row_ptr;
}

// ---- draw
struct NbAliasArgs {
  GraphView g;
  const NbAliasEntry* tab;
  uint64_t seed;
  const uint64_t* roots;
  const uint8_t* root_mask;
  uint64_t* out_id;
  float* out_w;
  int32_t* out_t;
  uint8_t* out_row_mask;
  int64_t n;
  int64_t default_node;
  uint32_t call_id;
  int32_t root_group;
  int32_t k;
  int32_t count;
  int32_t et[kMaxListedTypes];
};

// A lane per sample, the lanes of a root consecutive: 64 consecutive lanes hold consecutive slots,
// so the stores coalesce, and a wave holds ceil(64 / count) + 1 roots at most.  The first lane of
// every root IN THE WAVE looks the id up and reads the row record (FindRow, InitRowSampler) and hands
// the result to the root's other lanes - it is not loaded per sample.  Draws are keyed by (node id,
// j), so duplicate roots get identical rows by construction: no duplicate detection, no workspace.
// 64-bit sample index, grid-stride; the wave's loop is uniform (idle tail lanes stay for the
// cross-lane reads).
template <bool TF_LAYOUT>
__global__ __launch_bounds__(256, kWavesPerSimd) void SampleNeighborAliasKernel(
    const NbAliasArgs a, const int64_t stride_rows, const int32_t stride_slots) {
  const int64_t total = a.n * (int64_t)a.count;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int lane = (int)(threadIdx.x & 63u);
  int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t r = s / a.count;
  int32_t j = (int32_t)(s - r * a.count);
  for (; s - lane < total; s += stride) {
    const bool live = s < total;
    const bool first = live && (j == 0 || lane == 0);
    uint64_t node = 0;
    NbAliasRoot root{-1, 0};
    if (first) {
      node = a.roots[r];
      if (a.root_mask != nullptr && a.root_mask[r / a.root_group]) node = 0;
      root = NbAliasRootOf(a.g, node, a.et, a.k);
    }
    const int src = lane - (j < lane ? j : lane);      // the root's first lane in this wave
    node = (uint64_t)__shfl((long long)node, src);
    root.base = (int64_t)__shfl((long long)root.base, src);
    root.d = __shfl(root.d, src);
    if (live) {
      uint64_t id; float w; int32_t t; bool masked;
      NbAliasSlot(a.g, a.tab, root, a.et, a.k, a.seed, a.call_id, node, j, TF_LAYOUT, a.default_node,
                  &id, &w, &t, &masked);
      a.out_id[s] = id;
      a.out_w[s] = w;
      a.out_t[s] = t;
      if (j == 0 && a.out_row_mask != nullptr) a.out_row_mask[r] = masked ? 1 : 0;
    }
    r += stride_rows;
    j += stride_slots;
    if (j >= a.count) { j -= a.count; ++r; }
  }
}

int LaunchAlias(const euler_gpu_graph* g, hipStream_t stream, uint64_t seed, uint32_t call_id,
                const uint64_t* roots, int64_t n, const uint8_t* root_mask, int32_t root_group,
                const int32_t* edge_types, int32_t k, int32_t count, int32_t layout, int64_t default_node,
                uint64_t* out_id, float* out_w, int32_t* out_t, uint8_t* out_row_mask) {
  if (g == nullptr) return Fail(EULER_GPU_ENOGRAPH, "sample_neighbor_alias: null graph");
  if (n < 0 || count < 0 || k < 0 || k > kMaxListedTypes)
    return Fail(EULER_GPU_EINVAL, "sample_neighbor_alias: bad n/count/k (k <= 32)");
  if (layout != EULER_GPU_LAYOUT_CORE && layout != EULER_GPU_LAYOUT_TF)
    return Fail(EULER_GPU_EINVAL, "sample_neighbor_alias: bad layout");
  if (n == 0 || count == 0) return EULER_GPU_OK;
  if (!roots || !out_id || !out_w || !out_t) return Fail(EULER_GPU_EINVAL, "sample_neighbor_alias: null buffer");
  if (k > 0 && !edge_types) return Fail(EULER_GPU_EINVAL, "sample_neighbor_alias: null edge_types");
  if (n > INT64_MAX / count) return Fail(EULER_GPU_EINVAL, "sample_neighbor_alias: n * count overflows");
  NbAliasArgs a{};
  {
    const int rc = EnsureNbAlias(g, stream, &a.tab);
    if (rc != EULER_GPU_OK) return rc;
  }
  DeviceGuard dg(g->device);
  a.g = g->view;
  a.seed = seed; a.call_id = call_id;
  a.roots = roots; a.root_mask = root_mask;
  a.root_group = root_group > 0 ? root_group : 1;
  a.out_id = out_id; a.out_w = out_w; a.out_t = out_t; a.out_row_mask = out_row_mask;
  a.n = n; a.default_node = default_node;
  a.k = k; a.count = count;
  for (int i = 0; i < k; ++i) a.et[i] = edge_types[i];
  const int block = 256;
  // an alias draw costs the same for every row, so there is no tail of slow workgroups to even out:
  // GridFor's cap (16 workgroups per CU), grid-stride beyond it
  const int grid = GridFor(n * (int64_t)count, block);
  const int64_t stride = (int64_t)grid * block;
  const int64_t stride_rows = stride / count;
  const int32_t stride_slots = (int32_t)(stride - stride_rows * count);
  auto kern = layout == EULER_GPU_LAYOUT_TF ? SampleNeighborAliasKernel<true> : SampleNeighborAliasKernel<false>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, stream, a, stride_rows, stride_slots);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_graph_build_neighbor_alias(euler_gpu_graph* g, void* stream) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "build_neighbor_alias: null graph");
  const NbAliasEntry* tab = nullptr;
  return EnsureNbAlias(g, (hipStream_t)stream, &tab);
}

int euler_gpu_graph_neighbor_alias_info(const euler_gpu_graph* g, int64_t* bytes_host, int64_t* entries_host) {
  if (!g || !bytes_host || !entries_host) return Fail(EULER_GPU_EINVAL, "neighbor_alias_info: null argument");
  const bool built = g->nb_alias.load(std::memory_order_acquire) != nullptr;
  *bytes_host = built ? g->nb_alias_bytes : 0;
  *entries_host = built ? g->view.n_edges : 0;
  return EULER_GPU_OK;
}

int euler_gpu_graph_export_neighbor_alias(const euler_gpu_graph* g, const uint64_t* ids_host, int64_t n,
                                          int64_t* row_ptr_host, uint64_t* id_self_host,
                                          uint64_t* id_alias_host, float* prob_host, float* w_self_host,
                                          float* w_alias_host) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "export_neighbor_alias: null graph");
  if (n < 0 || !row_ptr_host || (n > 0 && !ids_host)) return Fail(EULER_GPU_EINVAL, "export_neighbor_alias: bad args");
  const NbAliasEntry* tab = g->nb_alias.load(std::memory_order_acquire);
  if (tab == nullptr) return Fail(EULER_GPU_EINVAL, "export_neighbor_alias: the tables are not built");
  DeviceGuard dg(g->device);
  row_ptr_host[0] = 0;
  if (n == 0) return EULER_GPU_OK;
  DevBuf ids_buf, meta_buf;
  EG_HIP(ids_buf.alloc((size_t)n * 8));
  EG_HIP(meta_buf.alloc((size_t)n * 16));
  int64_t* deg_dev = meta_buf.as<int64_t>();
  EG_HIP(hipMemcpy(ids_buf.as<void>(), ids_host, (size_t)n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(NbAliasExportMetaKernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, g->view,
                     ids_buf.as<uint64_t>(), n, deg_dev, deg_dev + n);
  EG_HIP(hipGetLastError());
  std::vector<int64_t> meta((size_t)n * 2);
  EG_HIP(hipMemcpy(meta.data(), deg_dev, (size_t)n * 16, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; ++i) row_ptr_host[i + 1] = row_ptr_host[i] + meta[(size_t)i];
  if (!id_self_host) return EULER_GPU_OK;         // the sizes only
  if (!id_alias_host || !prob_host || !w_self_host || !w_alias_host)
    return Fail(EULER_GPU_EINVAL, "export_neighbor_alias: null output");
  std::vector<NbAliasEntry> row;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t deg = meta[(size_t)i], off = meta[(size_t)(n + i)];
    if (deg == 0) continue;
    row.resize((size_t)deg);
    EG_HIP(hipMemcpy(row.data(), tab + off, (size_t)deg * sizeof(NbAliasEntry), hipMemcpyDeviceToHost));
    for (int64_t x = 0; x < deg; ++x) {
      const int64_t o = row_ptr_host[i] + x;
      id_self_host[o] = row[(size_t)x].id_self;
      id_alias_host[o] = row[(size_t)x].id_alias;
      prob_host[o] = row[(size_t)x].prob;
      w_self_host[o] = row[(size_t)x].w_self;
      w_alias_host[o] = row[(size_t)x].w_alias;
    }
  }
  return EULER_GPU_OK;
}

int euler_gpu_sample_neighbor_alias(const euler_gpu_graph* g, void* stream, uint64_t seed, uint32_t call_id,
                                    const uint64_t* roots_dev, int64_t n, const uint8_t* root_mask_dev,
                                    int32_t root_group, const int32_t* edge_types_host, int32_t k,
                                    int32_t count, int32_t layout, int64_t default_node,
                                    uint64_t* out_id_dev, float* out_w_dev, int32_t* out_t_dev,
                                    uint8_t* out_row_mask_dev) {
  return LaunchAlias(g, (hipStream_t)stream, seed, call_id, roots_dev, n, root_mask_dev, root_group,
                     edge_types_host, k, count, layout, default_node, out_id_dev, out_w_dev, out_t_dev,
                     out_row_mask_dev);
}

size_t euler_gpu_sample_fanout_alias_workspace(int64_t n, const int32_t* counts_host, int32_t layers) {
  return euler_gpu_sample_fanout_workspace(n, counts_host, layers);
}

int euler_gpu_sample_fanout_alias(const euler_gpu_graph* g, void* stream, uint64_t seed, uint32_t call_id,
                                  const uint64_t* roots_dev, int64_t n, const int32_t* edge_types_host,
                                  int32_t k, const int32_t* counts_host, int32_t layers,
                                  int64_t default_node, uint64_t* const* out_id_dev,
                                  float* const* out_w_dev, int32_t* const* out_t_dev, void* workspace_dev) {
  if (layers < 0 || n < 0 || (layers > 0 && (!counts_host || !out_id_dev || !out_w_dev || !out_t_dev)))
    return Fail(EULER_GPU_EINVAL, "sample_fanout_alias: bad arguments");
  if (layers > 0 && n > 0 && !workspace_dev) return Fail(EULER_GPU_EINVAL, "sample_fanout_alias: workspace required");
  if (g == nullptr) return Fail(EULER_GPU_ENOGRAPH, "sample_fanout_alias: null graph");
  // `layers` launches of the one kernel in one enqueue, no host wait between them: hop h draws with
  // call_id + h on hop h - 1's TF-layout ids, and the rows under a default hop h - 1 row sample as
  // node id 0 through that hop's row mask (one mask byte per root of every hop in the workspace)
  const uint64_t* roots = roots_dev;
  const uint8_t* mask = nullptr;
  int32_t group = 1;
  int64_t m = n;
  uint8_t* ws = (uint8_t*)workspace_dev;
  for (int32_t h = 0; h < layers; ++h) {
    if (counts_host[h] < 0 || (counts_host[h] > 0 && m > INT64_MAX / counts_host[h]))
      return Fail(EULER_GPU_EINVAL, "sample_fanout_alias: bad counts");
    uint8_t* row_mask = ws;
    ws += ((size_t)m + 15) & ~(size_t)15;
    const int rc = LaunchAlias(g, (hipStream_t)stream, seed, call_id + (uint32_t)h, roots, m, mask, group,
                               edge_types_host + (size_t)h * k, k, counts_host[h], EULER_GPU_LAYOUT_TF,
                               default_node, out_id_dev[h], out_w_dev[h], out_t_dev[h], row_mask);
    if (rc != EULER_GPU_OK) return rc;
    roots = out_id_dev[h];
    mask = row_mask;
    group = counts_host[h];
    m *= counts_host[h];
  }
  return EULER_GPU_OK;
}

}  // extern "C"
