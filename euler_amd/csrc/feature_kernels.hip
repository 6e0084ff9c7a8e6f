// Sparse (uint64) node features for gfx950 with their C-ABI entry point:
// TF GetSparseFeature (tf_euler/kernels/get_sparse_feature_op.cc:52-131) over
// Node::GetUint64Feature (core/graph/node.cc:330-372).  The dense (float)
// feature kernel lives in mp_kernels.hip.
#include <hip/hip_runtime.h>

#include "device_fns.h"
#include "device_mem.h"
#include "sparse_embed.h"

namespace euler_gpu {

namespace {

struct SparseFeatArgs {
  GraphView g;
  const int64_t* ufeat_ptr;
  const int32_t* ufeat_idx;
  const uint64_t* ufeat_val;
  const uint64_t* nodes;
  int64_t n;
  int32_t n_u64;
  int32_t fid;
};

// Values of slot `fid` of the node (GET_NODE_FEATURE, node.cc:330-351): an
// unknown node or slot has none.
__device__ __forceinline__ int32_t SlotRange(const SparseFeatArgs& a, uint64_t id,
                                             const uint64_t** first) {
  *first = nullptr;
  if (a.fid < 0 || a.fid >= a.n_u64) return 0;
  const int64_t row = FindRow(a.g, id);
  if (row < 0) return 0;
  const int32_t* idx = a.ufeat_idx + row * (int64_t)a.n_u64;
  const int32_t pre = a.fid == 0 ? 0 : idx[a.fid - 1];
  const int32_t now = idx[a.fid];
  *first = a.ufeat_val + a.ufeat_ptr[row] + pre;
  return now - pre;
}

// counts[i] = entries node i contributes: its values, or the one default entry
__global__ __launch_bounds__(256) void SparseFeatCountKernel(
    const SparseFeatArgs a, int64_t* __restrict__ counts,
    unsigned long long* __restrict__ max_len) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int32_t local_max = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    const uint64_t* first;
    int32_t len = SlotRange(a, a.nodes[i], &first);
    if (len < 1) len = 1;
    counts[i] = len;
    local_max = max(local_max, len);
  }
  // one atomic per wave
  for (int off = 32; off > 0; off >>= 1) local_max = max(local_max, __shfl_xor(local_max, off));
  if ((threadIdx.x & 63) == 0 && local_max > 0) atomicMax(max_len, (unsigned long long)local_max);
}

// The GQL `values(...)` form (core/kernels/get_feature_op.cc:34-70, "fea:2i" /
// "fea:2i+1"): counts without the default entry, idx pairs, packed values.
__global__ __launch_bounds__(256) void SparseFeatCoreCountKernel(
    const SparseFeatArgs a, int64_t* __restrict__ counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    const uint64_t* first;
    counts[i] = SlotRange(a, a.nodes[i], &first);
  }
}

__global__ __launch_bounds__(256) void SparseFeatCoreFillKernel(
    const SparseFeatArgs a, const int32_t* __restrict__ idx, uint64_t* __restrict__ values) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave; i < a.n; i += n_waves) {
    const uint64_t* first;
    const int32_t len = SlotRange(a, a.nodes[i], &first);
    const int64_t o = idx[2 * i];
    for (int32_t k = lane; k < len; k += 64) values[o + k] = first[k];
  }
}

__global__ void SparseFeatOffsetsToIdxKernel(const int64_t* __restrict__ off, int64_t n,
                                             int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    idx[2 * i] = (int32_t)off[i];
    idx[2 * i + 1] = (int32_t)off[i + 1];
  }
}

// One wave per node: lanes over its values (lists are short; the row offsets
// make the writes of consecutive nodes contiguous).
__global__ __launch_bounds__(256) void SparseFeatFillKernel(
    const SparseFeatArgs a, const int64_t* __restrict__ off, int64_t default_value,
    int64_t* __restrict__ indices, int64_t* __restrict__ values) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave; i < a.n; i += n_waves) {
    const uint64_t* first;
    const int32_t len = SlotRange(a, a.nodes[i], &first);
    const int64_t o = off[i];
    if (len < 1) {
      if (lane == 0) {
        indices[2 * o] = i;
        indices[2 * o + 1] = 0;
        values[o] = default_value;
      }
      continue;
    }
    for (int32_t k = lane; k < len; k += 64) {
      indices[2 * (o + k)] = i;
      indices[2 * (o + k) + 1] = k;
      values[o + k] = (int64_t)first[k];
    }
  }
}


// ---- fused embedding lookup (sparse_embed.h) ------------------------------------------------
// A group of G lanes per node, 64 / G nodes per wave: lane l of the group owns chunk l (+ G, ...)
// of the row - 16 bytes on the vector path, one element on the scalar one.  The group's first lane
// resolves the node and broadcasts (offset, length); the entry ids are read G at a time, one per
// lane, and handed round with __shfl inside SeFold.
struct SparseEmbedArgs {
  const void* table;
  uint64_t n_rows;
  uint64_t default_value;
  void* out;
  int32_t* counts;
  int32_t dim;
  int32_t combiner;
  int32_t group;
  int32_t has_default;
};

template <int DT, bool VEC> struct SeRow;
template <> struct SeRow<kF32, true> {
  using Raw = float4;
  static constexpr int N = 4;
  static __device__ __forceinline__ void Widen(const Raw& v, float f[4]) {
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  }
};
template <> struct SeRow<kF32, false> {
  using Raw = float;
  static constexpr int N = 1;
  static __device__ __forceinline__ void Widen(const Raw& v, float f[1]) { f[0] = v; }
};
template <int DT> struct SeRow<DT, true> {
  using Raw = uint4;
  static constexpr int N = 8;
  static __device__ __forceinline__ void Widen(const Raw& v, float f[8]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    Widen8<DT>(w, f);
  }
};
template <int DT> struct SeRow<DT, false> {
  using Raw = uint16_t;
  static constexpr int N = 1;
  static __device__ __forceinline__ void Widen(const Raw& v, float f[1]) { f[0] = HalfCvt<DT>::Widen(v); }
};

template <int DT, bool VEC>
struct SeDeviceOps {
  using Row = SeRow<DT, VEC>;
  using Raw = typename Row::Raw;
  const Raw* table;        // the table in units of one chunk
  int64_t row_chunks;      // chunks per row
  int64_t chunk;           // this lane's chunk of the row
  unsigned long long cur;  // this lane's entry of the G being folded
  int32_t group;
  bool active;             // chunk < row_chunks
  __device__ __forceinline__ uint64_t Entry(int32_t j) const { return __shfl(cur, j, group); }
  __device__ __forceinline__ Raw Load(int64_t row) const {
    return table[row * row_chunks + (active ? chunk : 0)];     // (an idle lane: chunk 0, dropped)
  }
  __device__ __forceinline__ void Widen(const Raw& v, float* f) const { Row::Widen(v, f); }
};

template <int ODT, int N>
__device__ __forceinline__ void SeStore(void* out, int64_t at, const float acc[N]) {
  if constexpr (ODT == kF32) {
    float* o = reinterpret_cast<float*>(out) + at;
    if constexpr (N == 1) {
      o[0] = acc[0];
    } else {
#pragma unroll
      for (int k = 0; k < N; k += 4)
        *reinterpret_cast<float4*>(o + k) = make_float4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]);
    }
  } else {
    uint16_t* o = reinterpret_cast<uint16_t*>(out) + at;
    if constexpr (N == 1) {
      o[0] = HalfCvt<ODT>::Narrow(acc[0]);
    } else {
      static_assert(N == 8, "a 16-byte chunk of 16-bit elements");
      uint32_t w[4];
      Narrow8<ODT>(acc, w);
      *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

template <int DT, int ODT, bool VEC>
__global__ __launch_bounds__(256) void SparseEmbedKernel(const SparseFeatArgs a,
                                                         const SparseEmbedArgs e) {
  using Ops = SeDeviceOps<DT, VEC>;
  constexpr int N = Ops::Row::N;
  const int32_t G = e.group;
  const int32_t gl = threadIdx.x & (G - 1);
  const int64_t slot = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int64_t n_slots = ((int64_t)gridDim.x * blockDim.x) / G;
  Ops o;
  o.table = reinterpret_cast<const typename Ops::Raw*>(e.table);
  o.row_chunks = e.dim / N;
  o.group = G;
  for (int64_t i = slot; i < a.n; i += n_slots) {
    int32_t len = 0;
    long long off = 0;
    if (gl == 0) {
      const uint64_t* first;
      len = SlotRange(a, a.nodes[i], &first);
      if (len > 0) off = first - a.ufeat_val;
    }
    len = __shfl(len, 0, G);
    off = __shfl(off, 0, G);
    const uint64_t* first = a.ufeat_val + off;
    const bool use_default = len < 1 && e.has_default;
    int32_t cnt = 0;
    for (int64_t c0 = 0; c0 < o.row_chunks; c0 += G) {
      o.chunk = c0 + gl;
      o.active = o.chunk < o.row_chunks;
      float acc[N];
#pragma unroll
      for (int k = 0; k < N; ++k) acc[k] = 0.f;
      cnt = 0;
      if (use_default) {
        o.cur = e.default_value;
        SeFold<N, kSeUnroll>(o, 1, e.n_rows, acc, &cnt);
      } else {
        for (int32_t e0 = 0; e0 < len; e0 += G) {
          o.cur = e0 + gl < len ? first[e0 + gl] : 0ull;
          SeFold<N, kSeUnroll>(o, min(G, len - e0), e.n_rows, acc, &cnt);
        }
      }
      SeFinish<N>(acc, cnt, e.combiner);
      if (o.active) SeStore<ODT, N>(e.out, (i * o.row_chunks + o.chunk) * N, acc);
    }
    if (gl == 0 && e.counts) e.counts[i] = cnt;
  }
}

template <int DT, int ODT>
void LaunchSparseEmbed(hipStream_t st, const SparseFeatArgs& a, SparseEmbedArgs e, bool vec) {
  const int block = 256;
  const int n_vec = DT == kF32 ? 4 : 8;
  e.group = SeGroupLanes(vec ? e.dim / n_vec : e.dim);
  const dim3 grid(GridFor(a.n * e.group, block));
  if (vec)
    hipLaunchKernelGGL((SparseEmbedKernel<DT, ODT, true>), grid, dim3(block), 0, st, a, e);
  else
    hipLaunchKernelGGL((SparseEmbedKernel<DT, ODT, false>), grid, dim3(block), 0, st, a, e);
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int32_t euler_gpu_graph_num_u64_features(const euler_gpu_graph* g) {
  return g ? g->n_u64 : -1;
}

int euler_gpu_get_sparse_feature(const euler_gpu_graph* g, void* stream,
                                 const uint64_t* nodes_dev, int64_t n, int32_t fid,
                                 int64_t default_value, int64_t* row_off_dev,
                                 int64_t* nnz_host, int64_t* max_len_host,
                                 int64_t* indices_dev, int64_t* values_dev) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "get_sparse_feature: null graph");
  if (n < 0) return Fail(EULER_GPU_EINVAL, "get_sparse_feature: n < 0");
  if (n == 0) {
    if (nnz_host) *nnz_host = 0;
    if (max_len_host) *max_len_host = 0;
    return EULER_GPU_OK;
  }
  if (!nodes_dev || !row_off_dev)
    return Fail(EULER_GPU_EINVAL, "get_sparse_feature: null buffer");
  hipStream_t st = (hipStream_t)stream;
  SparseFeatArgs a{};
  a.g = g->view;
  a.ufeat_ptr = g->ufeat_ptr; a.ufeat_idx = g->ufeat_idx; a.ufeat_val = g->ufeat_val;
  a.nodes = nodes_dev; a.n = n; a.n_u64 = g->n_u64; a.fid = fid;
  const int block = 256;
  if (indices_dev == nullptr) {
    StreamBuf counts_buf(st);
    EG_HIP(counts_buf.alloc((size_t)(n + 2) * sizeof(int64_t)));
    int64_t* counts = counts_buf.as<int64_t>();
    unsigned long long* max_len = reinterpret_cast<unsigned long long*>(counts + n + 1);
    EG_HIP(hipMemsetAsync(counts + n, 0, 2 * sizeof(int64_t), st));
    hipLaunchKernelGGL(SparseFeatCountKernel, dim3(GridFor(n, block)), dim3(block), 0, st, a,
                       counts, max_len);
    int rc = ExclusiveScanI64(st, counts, row_off_dev, n + 1);
    if (rc != EULER_GPU_OK) return rc;
    int64_t total = 0;
    unsigned long long ml = 0;
    EG_HIP(hipMemcpyAsync(&total, row_off_dev + n, 8, hipMemcpyDeviceToHost, st));
    EG_HIP(hipMemcpyAsync(&ml, max_len, 8, hipMemcpyDeviceToHost, st));
    EG_HIP(hipStreamSynchronize(st));
    if (nnz_host) *nnz_host = total;
    if (max_len_host) *max_len_host = (int64_t)ml;
    return EULER_GPU_OK;
  }
  if (!values_dev) return Fail(EULER_GPU_EINVAL, "get_sparse_feature: null values");
  hipLaunchKernelGGL(SparseFeatFillKernel, dim3(GridFor(n * 64, block)), dim3(block), 0, st,
                     a, row_off_dev, default_value, indices_dev, values_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_get_sparse_feature_core(const euler_gpu_graph* g, void* stream,
                                      const uint64_t* nodes_dev, int64_t n, int32_t fid,
                                      int32_t* idx_dev, int64_t* total_host,
                                      uint64_t* values_dev) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "get_sparse_feature_core: null graph");
  if (n < 0) return Fail(EULER_GPU_EINVAL, "get_sparse_feature_core: n < 0");
  if (n == 0) { if (total_host) *total_host = 0; return EULER_GPU_OK; }
  if (!nodes_dev || !idx_dev)
    return Fail(EULER_GPU_EINVAL, "get_sparse_feature_core: null buffer");
  hipStream_t st = (hipStream_t)stream;
  SparseFeatArgs a{};
  a.g = g->view;
  a.ufeat_ptr = g->ufeat_ptr; a.ufeat_idx = g->ufeat_idx; a.ufeat_val = g->ufeat_val;
  a.nodes = nodes_dev; a.n = n; a.n_u64 = g->n_u64; a.fid = fid;
  const int block = 256;
  if (values_dev == nullptr) {
    StreamBuf counts_buf(st);
    EG_HIP(counts_buf.alloc((size_t)(2 * n + 2) * sizeof(int64_t)));
    int64_t* counts = counts_buf.as<int64_t>();
    int64_t* off = counts + n + 1;
    EG_HIP(hipMemsetAsync(counts + n, 0, sizeof(int64_t), st));
    hipLaunchKernelGGL(SparseFeatCoreCountKernel, dim3(GridFor(n, block)), dim3(block), 0, st,
                       a, counts);
    int rc = ExclusiveScanI64(st, counts, off, n + 1);
    if (rc != EULER_GPU_OK) return rc;
    hipLaunchKernelGGL(SparseFeatOffsetsToIdxKernel, dim3((unsigned)((n + block - 1) / block)),
                       dim3(block), 0, st, off, n, idx_dev);
    int64_t total = 0;
    EG_HIP(hipMemcpyAsync(&total, off + n, 8, hipMemcpyDeviceToHost, st));
    EG_HIP(hipStreamSynchronize(st));
    if (total_host) *total_host = total;
    return EULER_GPU_OK;
  }
  hipLaunchKernelGGL(SparseFeatCoreFillKernel, dim3(GridFor(n * 64, block)), dim3(block), 0, st,
                     a, idx_dev, values_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

int euler_gpu_sparse_feature_embedding(const euler_gpu_graph* g, void* stream,
                                       const uint64_t* nodes_dev, int64_t n, int32_t fid,
                                       int32_t has_default, int64_t default_value,
                                       const void* table_dev, int32_t table_dtype, int64_t n_rows,
                                       int32_t dim, int32_t combiner, void* out_dev,
                                       int32_t out_dtype, int32_t* counts_dev) {
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "sparse_feature_embedding: null graph");
  if (n < 0) return Fail(EULER_GPU_EINVAL, "sparse_feature_embedding: n < 0");
  if (dim < 1) return Fail(EULER_GPU_EINVAL, "sparse_feature_embedding: dim < 1");
  if (n_rows < 1 || n_rows >= ((int64_t)1 << 31))
    return Fail(EULER_GPU_EINVAL, "sparse_feature_embedding: n_rows outside [1, 2^31)");
  if (table_dtype != kF32 && table_dtype != kBF16 && table_dtype != kF16)
    return Fail(EULER_GPU_EINVAL, "sparse_feature_embedding: unknown table dtype");
  if (out_dtype != kF32 && out_dtype != table_dtype)
    return Fail(EULER_GPU_EINVAL, "sparse_feature_embedding: out dtype is fp32 or the table's");
  if (combiner != kSeSum && combiner != kSeMean && combiner != kSeSqrtn)
    return Fail(EULER_GPU_EINVAL, "sparse_feature_embedding: unknown combiner");
  if (n == 0) return EULER_GPU_OK;
  if (!nodes_dev || !table_dev || !out_dev)
    return Fail(EULER_GPU_EINVAL, "sparse_feature_embedding: null buffer");
  hipStream_t st = (hipStream_t)stream;
  SparseFeatArgs a{};
  a.g = g->view;
  a.ufeat_ptr = g->ufeat_ptr; a.ufeat_idx = g->ufeat_idx; a.ufeat_val = g->ufeat_val;
  a.nodes = nodes_dev; a.n = n; a.n_u64 = g->n_u64; a.fid = fid;
  SparseEmbedArgs e{};
  e.table = table_dev; e.n_rows = (uint64_t)n_rows; e.default_value = (uint64_t)default_value;
  e.out = out_dev; e.counts = counts_dev; e.dim = dim; e.combiner = combiner;
  e.has_default = has_default != 0;
  // the 16-byte path: whole chunks per row, table and output on 16-byte boundaries (the row
  // strides then are multiples of 16 too); everything else takes one element per lane
  const int n_vec = table_dtype == kF32 ? 4 : 8;
  const bool vec = dim % n_vec == 0 && (reinterpret_cast<uintptr_t>(table_dev) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(out_dev) & 15) == 0;
  if (table_dtype == kF32) LaunchSparseEmbed<kF32, kF32>(st, a, e, vec);
  else if (table_dtype == kBF16 && out_dtype == kF32) LaunchSparseEmbed<kBF16, kF32>(st, a, e, vec);
  else if (table_dtype == kBF16) LaunchSparseEmbed<kBF16, kBF16>(st, a, e, vec);
  else if (out_dtype == kF32) LaunchSparseEmbed<kF16, kF32>(st, a, e, vec);
  else LaunchSparseEmbed<kF16, kF16>(st, a, e, vec);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

}  // extern "C"
