// Full-neighbour aggregation read straight from the graph's rows, for gfx950 (mp_rows.h states the
// contract and the arithmetic):
//  - euler_gpu_neighbor_reduce: queried node i reduces the table rows of its stored neighbours - the
//    entries of its row's listed edge-type groups, as euler_gpu_get_full_neighbor enumerates them
//    (core/graph/node.cc:175-197) - with no weight, the edge weights (the differences of the row's
//    running sums) or the GCN normalisation, optionally its own row appended and a root term added
//    in the same pass.  The ids and the running sums are read where the graph keeps them: no list
//    of the edges is written and read back, no host wait, no 2^31 ceiling on the listed total.
//  - euler_gpu_neighbor_degree: the listed degree of every queried node (FullNbCount's sum), as
//    int32 or as norm = 1 / sqrt(deg) (GcnNormOf), without a host wait.
// The kernels assign lanes exactly as the weighted segment reduces do (RowLaneShape: a wave-slot
// per queried node; a column per lane, or N adjacent columns per lane with one 16-byte access a
// row); a slot finds its row (FindRow, LoadRowMeta) and runs RowReduce under RowOps.  A hub is one
// slot's loop: the order of a column's sum is the enumerated one, never split across waves.
#include <hip/hip_runtime.h>

#include <string>

#include "common.h"
#include "device_fns.h"
#include "half_cvt.h"
#include "mp_loaders.h"
#include "mp_rows.h"
#include "mp_segments.h"

namespace euler_gpu {
namespace {

static_assert(sizeof(RowTypeList::et) / sizeof(int32_t) == kMaxListedTypes, "RowTypeList holds kMaxListedTypes");

struct NbrCall {
  GraphView g;
  const uint64_t* nodes;
  int32_t n;
  int32_t self_loop;
  RowTypeList L;
  const void* x;
  uint32_t rows;
  int64_t d;
  const float* norm_dst;     // kind 2: [n]
  const float* norm_src;     // kind 2: [rows]
  GcnRoot R;
  void* out;
};

// the row of a queried node as RowOps / RowReduce read it; type_end == nullptr: no row
struct NodeRow {
  const int32_t* type_end;
  const uint32_t* nbr_lo;
  const float* prefix_w;
};

__device__ __forceinline__ NodeRow FindNodeRow(const GraphView& g, uint64_t id) {
  const int64_t row = FindRow(g, id);
  if (row < 0) return NodeRow{nullptr, nullptr, nullptr};
  const RowMeta m = LoadRowMeta(g, row);
  return NodeRow{m.type_end, reinterpret_cast<const uint32_t*>(g.nbr + m.row_ptr), g.prefix_w + m.row_ptr};
}

// blockDim = (64, 4): a wave-slot per queried node, one column per lane (any d, any alignment)
template <int MODE, int KIND, int DT, bool OUT16>
__global__ __launch_bounds__(256) void NeighborReduceKernel(const NbrCall a) {
  using Loader = typename ElemLoader<DT>::type;
  using Elem = typename Loader::Raw;
  const int lane = threadIdx.x;
  const int64_t d = a.d;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; r < a.n;
       r += (int64_t)gridDim.x * blockDim.y) {
    const uint64_t id = a.nodes[r];
    const NodeRow nr = FindNodeRow(a.g, id);
    const float nd = KIND == kRowWeightNorm ? a.norm_dst[r] : 0.f;
    for (int64_t c = lane; c < d; c += 64) {
      const RowOps<KIND, Loader> ops{Loader{static_cast<const Elem*>(a.x), d, c}, nr.nbr_lo, nr.prefix_w,
                                     a.norm_src, a.rows, nd, (uint32_t)id};
      float acc[1];
      RowReduce<MODE, 1>(ops, a.L, nr.type_end, a.self_loop != 0, acc);
      if (a.R.p != nullptr) {
        const float root[1] = {RootElem<DT>(a.R, r * d + c)};
        GcnRootEpilogue<1>(acc, root, a.R.agg_scale, a.R.root_scale);
      }
      StoreOne<DT, OUT16>(a.out, r * d + c, acc[0]);
    }
  }
}

// the N-column loader of a storage type: four fp32 columns, eight 16-bit ones
template <int DT> struct VecLoader { using type = LoadH16x8<DT>; static constexpr int N = 8; };
template <> struct VecLoader<kF32> { using type = LoadF32x4; static constexpr int N = 4; };

// d % N == 0 with dv = d / N a divisor of 64: dv lanes a node, 64 / dv nodes a wave, 16-byte
// loads and stores (x, root and out on 16-byte boundaries)
template <int MODE, int KIND, int DT, bool OUT16>
__global__ __launch_bounds__(256) void NeighborReduceVecKernel(const NbrCall a, const int32_t dv) {
  using Loader = typename VecLoader<DT>::type;
  using Raw = typename Loader::Raw;
  constexpr int N = VecLoader<DT>::N;
  const int32_t per_wave = 64 / dv;
  const int32_t sub = threadIdx.x / dv, cl = threadIdx.x - sub * dv;
  const int64_t per_block = (int64_t)blockDim.y * per_wave;
  for (int64_t r = (int64_t)blockIdx.x * per_block + threadIdx.y * per_wave + sub; r < a.n;
       r += (int64_t)gridDim.x * per_block) {
    const uint64_t id = a.nodes[r];
    const NodeRow nr = FindNodeRow(a.g, id);
    const float nd = KIND == kRowWeightNorm ? a.norm_dst[r] : 0.f;
    const RowOps<KIND, Loader> ops{Loader{static_cast<const Raw*>(a.x), dv, cl}, nr.nbr_lo, nr.prefix_w,
                                   a.norm_src, a.rows, nd, (uint32_t)id};
    float acc[N];
    RowReduce<MODE, N>(ops, a.L, nr.type_end, a.self_loop != 0, acc);
    const int64_t slot = r * dv + cl;
    if constexpr (DT == kF32) {
      if (a.R.p != nullptr) {
        const float4 v = static_cast<const float4*>(a.R.p)[slot];
        const float root[4] = {v.x, v.y, v.z, v.w};
        GcnRootEpilogue<4>(acc, root, a.R.agg_scale, a.R.root_scale);
      }
      static_cast<float4*>(a.out)[slot] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
      if (a.R.p != nullptr) {
        float root[8];
        RootElems8<DT>(a.R, slot, root);
        GcnRootEpilogue<8>(acc, root, a.R.agg_scale, a.R.root_scale);
      }
      StoreEight<DT, OUT16>(a.out, slot, acc);
    }
  }
}

template <int MODE, int KIND, int DT, bool OUT16>
int Launch(hipStream_t st, const NbrCall& c) {
  // RowLaneShape with one more condition of the vector form: the root rows on 16-byte boundaries
  // too (a misaligned root asks with dh = 1, which no lane of n > 1 columns divides)
  const bool root_aligned = (uintptr_t)c.R.p % 16 == 0;
  const LaneShape s = RowLaneShape(c.n, c.d, VecLoader<DT>::N, root_aligned ? 0 : 1, c.x, c.out);
  if (s.vec)
    hipLaunchKernelGGL((NeighborReduceVecKernel<MODE, KIND, DT, OUT16>), dim3(s.blocks), dim3(64, 4), 0, st, c,
                       (int32_t)s.dv);
  else
    hipLaunchKernelGGL((NeighborReduceKernel<MODE, KIND, DT, OUT16>), dim3(s.blocks), dim3(64, 4), 0, st, c);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int MODE, int KIND>
int LaunchDtype(hipStream_t st, const NbrCall& c, int32_t dtype, bool out16) {
  if (dtype == EULER_GPU_F32) return Launch<MODE, KIND, kF32, false>(st, c);
  if (dtype == EULER_GPU_BF16)
    return out16 ? Launch<MODE, KIND, kBF16, true>(st, c) : Launch<MODE, KIND, kBF16, false>(st, c);
  return out16 ? Launch<MODE, KIND, kF16, true>(st, c) : Launch<MODE, KIND, kF16, false>(st, c);
}

template <int MODE>
int LaunchKind(hipStream_t st, const NbrCall& c, int32_t kind, int32_t dtype, bool out16) {
  if (kind == kRowWeightNone) return LaunchDtype<MODE, kRowWeightNone>(st, c, dtype, out16);
  if (kind == kRowWeightEdge) return LaunchDtype<MODE, kRowWeightEdge>(st, c, dtype, out16);
  return LaunchDtype<MODE, kRowWeightNorm>(st, c, dtype, out16);
}

// ---- degrees and norms ----------------------------------------------------------------------------
// A thread per queried node.  A degree past int32 (a type listed many times over a huge row) is
// stored as INT32_MAX.
__global__ __launch_bounds__(256) void NeighborDegreeKernel(const GraphView g, const uint64_t* __restrict__ nodes,
                                                            int64_t n, const RowTypeList L, int32_t self_loop,
                                                            int32_t as_norm, void* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t row = FindRow(g, nodes[i]);
    const int64_t deg64 = RowListedDegree(L, row < 0 ? nullptr : LoadRowMeta(g, row).type_end, self_loop != 0);
    const int32_t deg = deg64 > 0x7fffffffLL ? 0x7fffffff : (int32_t)deg64;
    if (as_norm) static_cast<float*>(out)[i] = GcnNormOf(deg);
    else static_cast<int32_t*>(out)[i] = deg;
  }
}

RowTypeList TypeList(const euler_gpu_graph* g, const int32_t* edge_types_host, int32_t k) {
  RowTypeList L{};
  L.k = k;
  L.T = g->view.T;
  for (int32_t i = 0; i < k; ++i) L.et[i] = edge_types_host[i];
  return L;
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_neighbor_reduce(const euler_gpu_graph* g, void* stream, int32_t mode, const uint64_t* nodes_dev,
                              int64_t n, const int32_t* edge_types_host, int32_t k, int32_t weight_kind,
                              int32_t self_loop, const void* table_dev, int32_t table_dtype, int64_t table_rows,
                              int64_t d, const float* norm_dst_dev, const float* norm_src_dev, const void* root_dev,
                              int32_t root_dtype, float root_a, float root_b, void* out_dev, int32_t out_dtype) {
  const auto fail = [](const std::string& why) { return Fail(EULER_GPU_EINVAL, "neighbor_reduce: " + why); };
  // the ladder, in the order of CheckMpReduce: host arithmetic only in front of the first HIP call
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "neighbor_reduce: null graph");
  if (!KnownDtype(table_dtype)) return fail("unknown dtype " + std::to_string(table_dtype) + kDtypeCodes);
  if (out_dtype != EULER_GPU_F32 && out_dtype != table_dtype)
    return fail("out_dtype " + std::to_string(out_dtype) + " is neither fp32 nor the input's dtype");
  if (root_dev && root_dtype != EULER_GPU_F32 && root_dtype != table_dtype)
    return fail("root_dtype " + std::to_string(root_dtype) + " is neither fp32 nor the input's dtype");
  if (mode < 0 || mode > 2) return fail("mode is 0 add, 1 max, 2 mean");
  if (weight_kind < 0 || weight_kind > 2) return fail("weight_kind is 0 none, 1 edge, 2 norm");
  if (n < 0 || d < 0 || k < 0) return fail("bad shape");
  if (n == 0 || d == 0) return EULER_GPU_OK;
  if (!nodes_dev || !table_dev || !out_dev || (k > 0 && !edge_types_host)) return fail("null buffer");
  if (k > kMaxListedTypes) return fail("more than 32 listed edge types");
  // the index is the low 32-bit word of the id: the table must be addressable by it, and have a
  // last row for an id past it to read
  if (table_rows < 1) return fail("the table must have at least one row");
  if (table_rows >= (1LL << 31)) return fail("the table must have fewer than 2^31 rows");
  if (n >= (1LL << 31)) return fail("n >= 2^31");
  const bool norm = weight_kind == kRowWeightNorm;
  if (norm != (norm_dst_dev != nullptr) || norm != (norm_src_dev != nullptr))
    return fail("norm_dst and norm_src come with weight_kind 2, and only with it");
  // (root_a / root_b are read only when root_dev is set)
  const uintptr_t elem = table_dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)nodes_dev % 8 != 0 || (uintptr_t)table_dev % elem != 0 ||
      (uintptr_t)out_dev % (out_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (root_dev && (uintptr_t)root_dev % (root_dtype == EULER_GPU_F32 ? 4 : 2) != 0) ||
      (uintptr_t)norm_dst_dev % 4 != 0 || (uintptr_t)norm_src_dev % 4 != 0)
    return fail("a buffer is not aligned to its type");

  hipStream_t st = (hipStream_t)stream;
  const NbrCall c{g->view, nodes_dev, (int32_t)n, self_loop != 0 ? 1 : 0, TypeList(g, edge_types_host, k),
                  table_dev, (uint32_t)table_rows, d, norm_dst_dev, norm_src_dev,
                  GcnRoot{root_dev, root_dtype == EULER_GPU_F32, root_a, root_b}, out_dev};
  const bool out16 = out_dtype != EULER_GPU_F32;
  if (mode == 0) return LaunchKind<0>(st, c, weight_kind, table_dtype, out16);
  if (mode == 1) return LaunchKind<1>(st, c, weight_kind, table_dtype, out16);
  return LaunchKind<2>(st, c, weight_kind, table_dtype, out16);
}

int euler_gpu_neighbor_degree(const euler_gpu_graph* g, void* stream, const uint64_t* nodes_dev, int64_t n,
                              const int32_t* edge_types_host, int32_t k, int32_t self_loop, int32_t as_norm,
                              void* out_dev) {
  const auto fail = [](const char* why) { return Fail(EULER_GPU_EINVAL, std::string("neighbor_degree: ") + why); };
  if (!g) return Fail(EULER_GPU_ENOGRAPH, "neighbor_degree: null graph");
  if (n < 0 || k < 0) return fail("bad shape");
  if (n == 0) return EULER_GPU_OK;
  if (!nodes_dev || !out_dev || (k > 0 && !edge_types_host)) return fail("null buffer");
  if (k > kMaxListedTypes) return fail("more than 32 listed edge types");
  if (n >= (1LL << 31)) return fail("n >= 2^31");
  if ((uintptr_t)nodes_dev % 8 != 0 || (uintptr_t)out_dev % 4 != 0) return fail("a buffer is not aligned to its type");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(NeighborDegreeKernel, dim3(GridFor(n, 256)), dim3(256), 0, st, g->view, nodes_dev, n,
                     TypeList(g, edge_types_host, k), self_loop != 0 ? 1 : 0, as_norm != 0 ? 1 : 0, out_dev);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

}  // extern "C"
