// GCN-normalised aggregation for gfx950 (mp_gcn.h states the arithmetic):
//  - euler_gpu_gcn_norm: the two degree tables of a block as norm = 1 / sqrt(deg).  Degrees are
//    integers, so they are a histogram: int32 atomics into zeroed stream-ordered scratch - no
//    grouping of the keys, no sort, no host wait, no float atomics, and the same bits on every run
//    (integer sums do not depend on their order) - then one small kernel that writes both tables.
//  - euler_gpu_gather_reduce_norm_t: the weighted segment reduce of mp_kernels.hip /
//    mp_half_kernels.hip whose weight is not an [e] array but fl(norm_dst[r] * norm_src[g(p)]),
//    formed from the two tables where it is used, with an optional root term in the same pass.
//    The kernels assign lanes exactly as the weighted kernels do (a column per lane, or N adjacent
//    columns per lane with one 16-byte access a row); the arithmetic of a destination is
//    WeightedReduceRow under GcnNormOps.
#include <hip/hip_runtime.h>

#include <string>

#include "device_mem.h"
#include "half_cvt.h"
#include "mp_gcn.h"
#include "mp_loaders.h"
#include "mp_segments.h"

namespace euler_gpu {
namespace {

// ---- degrees and norm tables --------------------------------------------------------------------
// An edge counts iff BOTH keys are in range: an edge the reduce leaves out (destination key
// outside the block, or a gather index outside the table) changes nobody's degree.
__global__ __launch_bounds__(256) void GcnDegreeKernel(const int32_t* __restrict__ dst,
                                                       const int32_t* __restrict__ src, int64_t e,
                                                       uint32_t size_dst, uint32_t size_src,
                                                       int32_t* __restrict__ deg_dst,
                                                       int32_t* __restrict__ deg_src) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < e; i += stride) {
    const uint32_t a = (uint32_t)dst[i], b = (uint32_t)src[i];      // (negative keys: >= 2^31)
    if (a < size_dst && b < size_src) {
      atomicAdd(&deg_dst[a], 1);
      atomicAdd(&deg_src[b], 1);
    }
  }
}

// deg is [size_dst + size_src]: the destination side, then the source side
__global__ __launch_bounds__(256) void GcnNormKernel(const int32_t* __restrict__ deg, int64_t size_dst,
                                                     int64_t size_src, float* __restrict__ norm_dst,
                                                     float* __restrict__ norm_src) {
  const int64_t n = size_dst + size_src;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float v = GcnNormOf(deg[i]);
    if (i < size_dst) norm_dst[i] = v;
    else norm_src[i - size_dst] = v;
  }
}

// ---- the node-scaled reduce -----------------------------------------------------------------------
// (mp_loaders.h: what one lane loads of a row, the root term and the stores)
struct GcnTables {
  const float* norm_dst;     // [size]
  const float* norm_src;     // [rows]
  uint32_t rows;
};

// blockDim = (64, 4): a wave-slot per output row, one column per lane (any d, any alignment)
template <int MODE, int DT, bool OUT16>
__global__ __launch_bounds__(256) void GcnReduceKernel(const void* __restrict__ x, const SegSpec seg,
                                                       const MpwIndex ix, const GcnTables T, int64_t d,
                                                       const GcnRoot R, void* __restrict__ out) {
  using Loader = typename ElemLoader<DT>::type;
  using Elem = typename Loader::Raw;
  const int lane = threadIdx.x;
  const int32_t size = seg.size;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; r < size;
       r += (int64_t)gridDim.x * blockDim.y) {
    int64_t b, en;
    SegBounds(seg, r, &b, &en);
    const float nd = T.norm_dst[r];
    for (int64_t c = lane; c < d; c += 64) {
      const GcnNormOps<Loader> ops{Loader{static_cast<const Elem*>(x), d, c}, ix, T.norm_src, T.rows, nd};
      float acc[1];
      WeightedReduceRow<MODE, 1>(ops, b, en, acc);
      if (R.p != nullptr) {
        const float root[1] = {RootElem<DT>(R, r * d + c)};
        GcnRootEpilogue<1>(acc, root, R.agg_scale, R.root_scale);
      }
      StoreOne<DT, OUT16>(out, r * d + c, acc[0]);
    }
  }
}

// fp32, d % 4 == 0 with d4 = d / 4 a divisor of 64: d4 lanes a row, 64 / d4 rows a wave, 16-byte
// loads and stores (x, root and out on 16-byte boundaries)
template <int MODE>
__global__ __launch_bounds__(256) void GcnReduceVec4Kernel(const float* __restrict__ x, const SegSpec seg,
                                                           const MpwIndex ix, const GcnTables T, int32_t d4,
                                                           const GcnRoot R, float* __restrict__ out) {
  const int32_t size = seg.size;
  const int32_t rows_per_wave = 64 / d4;
  const int32_t sub = threadIdx.x / d4, cl = threadIdx.x - sub * d4;
  const int64_t rows_per_block = (int64_t)blockDim.y * rows_per_wave;
  for (int64_t r = (int64_t)blockIdx.x * rows_per_block + threadIdx.y * rows_per_wave + sub;
       r < size; r += (int64_t)gridDim.x * rows_per_block) {
    int64_t b, en;
    SegBounds(seg, r, &b, &en);
    const GcnNormOps<LoadF32x4> ops{LoadF32x4{reinterpret_cast<const float4*>(x), d4, cl}, ix, T.norm_src,
                                    T.rows, T.norm_dst[r]};
    float acc[4];
    WeightedReduceRow<MODE, 4>(ops, b, en, acc);
    if (R.p != nullptr) {
      const float4 v = static_cast<const float4*>(R.p)[r * d4 + cl];
      const float root[4] = {v.x, v.y, v.z, v.w};
      GcnRootEpilogue<4>(acc, root, R.agg_scale, R.root_scale);
    }
    reinterpret_cast<float4*>(out)[r * d4 + cl] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  }
}

// 16-bit rows, d % 8 == 0 with d8 = d / 8 a divisor of 64: a lane owns eight adjacent columns
template <int MODE, int DT, bool OUT16>
__global__ __launch_bounds__(256) void GcnReduceVec8Kernel(const uint4* __restrict__ x8, const SegSpec seg,
                                                           const MpwIndex ix, const GcnTables T, int32_t d8,
                                                           const GcnRoot R, void* __restrict__ out) {
  const int32_t size = seg.size;
  const int32_t rows_per_wave = 64 / d8;
  const int32_t sub = threadIdx.x / d8, cl = threadIdx.x - sub * d8;
  const int64_t rows_per_block = (int64_t)blockDim.y * rows_per_wave;
  for (int64_t r = (int64_t)blockIdx.x * rows_per_block + threadIdx.y * rows_per_wave + sub;
       r < size; r += (int64_t)gridDim.x * rows_per_block) {
    int64_t b, en;
    SegBounds(seg, r, &b, &en);
    const GcnNormOps<LoadH16x8<DT>> ops{LoadH16x8<DT>{x8, d8, cl}, ix, T.norm_src, T.rows, T.norm_dst[r]};
    float acc[8];
    WeightedReduceRow<MODE, 8>(ops, b, en, acc);
    const int64_t slot = r * d8 + cl;
    if (R.p != nullptr) {
      float root[8];
      RootElems8<DT>(R, slot, root);
      GcnRootEpilogue<8>(acc, root, R.agg_scale, R.root_scale);
    }
    StoreEight<DT, OUT16>(out, slot, acc);
  }
}

struct GcnCall {
  const void* x; int64_t d; void* out;
  SegSpec seg; MpwIndex ix; GcnTables T; GcnRoot R;
};

// RowLaneShape with one more condition of the vector form: the root rows on 16-byte boundaries too.
// (A misaligned root asks with dh = 1, which no lane of n > 1 columns divides: the element form.)
LaneShape GcnLaneShape(const GcnCall& c, int n) {
  const bool root_aligned = (uintptr_t)c.R.p % 16 == 0;
  return RowLaneShape(c.seg.size, c.d, n, root_aligned ? 0 : 1, c.x, c.out);
}

template <int MODE>
int LaunchF32(hipStream_t st, const GcnCall& c) {
  const LaneShape s = GcnLaneShape(c, 4);
  if (s.vec)
    hipLaunchKernelGGL(GcnReduceVec4Kernel<MODE>, dim3(s.blocks), dim3(64, 4), 0, st,
                       static_cast<const float*>(c.x), c.seg, c.ix, c.T, (int32_t)s.dv, c.R,
                       static_cast<float*>(c.out));
  else
    hipLaunchKernelGGL((GcnReduceKernel<MODE, kF32, false>), dim3(s.blocks), dim3(64, 4), 0, st, c.x, c.seg,
                       c.ix, c.T, c.d, c.R, c.out);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int MODE, int DT, bool OUT16>
int LaunchH16(hipStream_t st, const GcnCall& c) {
  const LaneShape s = GcnLaneShape(c, 8);
  if (s.vec)
    hipLaunchKernelGGL((GcnReduceVec8Kernel<MODE, DT, OUT16>), dim3(s.blocks), dim3(64, 4), 0, st,
                       static_cast<const uint4*>(c.x), c.seg, c.ix, c.T, (int32_t)s.dv, c.R, c.out);
  else
    hipLaunchKernelGGL((GcnReduceKernel<MODE, DT, OUT16>), dim3(s.blocks), dim3(64, 4), 0, st, c.x, c.seg,
                       c.ix, c.T, c.d, c.R, c.out);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int MODE>
int LaunchMode(hipStream_t st, const GcnCall& c, int32_t in_dtype, bool out16) {
  if (in_dtype == EULER_GPU_F32) return LaunchF32<MODE>(st, c);
  if (in_dtype == EULER_GPU_BF16)
    return out16 ? LaunchH16<MODE, kBF16, true>(st, c) : LaunchH16<MODE, kBF16, false>(st, c);
  return out16 ? LaunchH16<MODE, kF16, true>(st, c) : LaunchH16<MODE, kF16, false>(st, c);
}

// a failing exit after work was enqueued: the stream is drained before the scratch goes back
int Drained(hipStream_t st, int rc) {
  if (rc != EULER_GPU_OK) (void)hipStreamSynchronize(st);
  return rc;
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_gcn_norm(void* stream, const int32_t* dst_keys_dev, const int32_t* src_keys_dev, int64_t e,
                       int32_t size_dst, int32_t size_src, float* norm_dst_out_dev, float* norm_src_out_dev) {
  const auto fail = [](const char* why) { return Fail(EULER_GPU_EINVAL, std::string("gcn_norm: ") + why); };
  if (e < 0 || size_dst < 0 || size_src < 0) return fail("bad shape");
  if (size_dst == 0 && size_src == 0) return EULER_GPU_OK;
  if ((size_dst > 0 && !norm_dst_out_dev) || (size_src > 0 && !norm_src_out_dev) ||
      (e > 0 && (!dst_keys_dev || !src_keys_dev)))
    return fail("null buffer");
  if (e >= (1LL << 31)) return fail("e >= 2^31");
  if ((uintptr_t)dst_keys_dev % 4 != 0 || (uintptr_t)src_keys_dev % 4 != 0 ||
      (uintptr_t)norm_dst_out_dev % 4 != 0 || (uintptr_t)norm_src_out_dev % 4 != 0)
    return fail("keys and tables must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)size_dst + size_src;
  StreamBuf deg(st);                    // [size_dst + size_src] int32 counters
  EG_HIP(deg.alloc((size_t)n * 4));
  EG_HIP(hipMemsetAsync(deg.as(), 0, (size_t)n * 4, st));
  if (e > 0 && size_dst > 0 && size_src > 0) {
    hipLaunchKernelGGL(GcnDegreeKernel, dim3(GridFor(e, 256)), dim3(256), 0, st, dst_keys_dev, src_keys_dev, e,
                       (uint32_t)size_dst, (uint32_t)size_src, deg.as<int32_t>(), deg.as<int32_t>() + size_dst);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess)
      return Drained(st, Fail(EULER_GPU_EHIP, std::string("gcn_norm: ") + hipGetErrorString(err)));
  }
  // the only kernel that writes the outputs: both tables, or neither
  hipLaunchKernelGGL(GcnNormKernel, dim3(GridFor(n, 256)), dim3(256), 0, st, deg.as<int32_t>(), (int64_t)size_dst,
                     (int64_t)size_src, norm_dst_out_dev, norm_src_out_dev);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess)
    return Drained(st, Fail(EULER_GPU_EHIP, std::string("gcn_norm: ") + hipGetErrorString(err)));
  return EULER_GPU_OK;
}

int euler_gpu_gather_reduce_norm_t(void* stream, int32_t mode, const void* x_dev, int32_t in_dtype, int64_t rows,
                                   const int32_t* gather_indices_dev, const int32_t* indices_dev,
                                   const int64_t* seg_ptr_dev, int64_t count, int64_t e, int64_t d, int32_t size,
                                   const float* norm_dst_dev, const float* norm_src_dev, const void* root_dev,
                                   int32_t root_dtype, float agg_scale, float root_scale, void* out_dev,
                                   int32_t out_dtype) {
  const auto fail = [](const std::string& why) { return Fail(EULER_GPU_EINVAL, "gather_reduce_norm: " + why); };
  // the ladder, in the order of CheckMpReduce
  if (!KnownDtype(in_dtype)) return fail("unknown dtype " + std::to_string(in_dtype) + kDtypeCodes);
  if (out_dtype != EULER_GPU_F32 && out_dtype != in_dtype)
    return fail("out_dtype " + std::to_string(out_dtype) + " is neither fp32 nor the input's dtype");
  if (root_dev && root_dtype != EULER_GPU_F32 && root_dtype != in_dtype)
    return fail("root_dtype " + std::to_string(root_dtype) + " is neither fp32 nor the input's dtype");
  if (mode == 1) return fail("max is not supported (mode is 0 add, 2 mean)");
  if (mode != 0 && mode != 2) return fail("mode is 0 add, 2 mean");
  if (e < 0 || d < 0 || size < 0 || rows < 0 || count < 0) return fail("bad shape");
  hipStream_t st = (hipStream_t)stream;
  SegDest dst(st, indices_dev, seg_ptr_dev, count, e, size);
  // (a block without edges may come with no form at all: the keys of an empty tensor are null)
  if (const char* why = dst.FormError(SegDest::kNoFormWhenEmpty)) return fail(why);
  if (size == 0 || d == 0) return EULER_GPU_OK;
  // what the kernels read: out and norm_dst[r] for every destination, whatever its segment; x, the gather
  // indices and norm_src only where an update can contribute (e > 0 and rows > 0: an empty table has no
  // row to read, and its tensors come as null)
  const bool live = e > 0 && rows > 0;
  if (!out_dev || !norm_dst_dev || (live && (!x_dev || !gather_indices_dev || !norm_src_dev)))
    return fail("null buffer");
  if (const char* why = dst.LengthError()) return fail(why);
  if (rows >= (1LL << 31)) return fail("the table must have fewer than 2^31 rows");
  // a destination could collect 2^24 or more updates: its f32 count would no longer be its length
  // (keys or seg_ptr: no segment is longer than e)
  if (mode == 2 && count == 0 && e >= (1LL << 24)) return fail("mean needs e < 2^24");
  if (mode == 2 && count >= (1LL << 24)) return fail("mean needs segments shorter than 2^24");
  const uintptr_t elem = in_dtype == EULER_GPU_F32 ? 4 : 2;
  if ((uintptr_t)x_dev % elem != 0 || (uintptr_t)out_dev % (out_dtype == EULER_GPU_F32 ? 4 : 2) != 0 ||
      (uintptr_t)root_dev % (root_dtype == EULER_GPU_F32 ? 4 : 2) != 0)
    return fail("x, root and out must be aligned to their type");
  if ((uintptr_t)norm_dst_dev % 4 != 0 || (uintptr_t)norm_src_dev % 4 != 0 ||
      (uintptr_t)gather_indices_dev % 4 != 0 || (uintptr_t)indices_dev % 4 != 0 || (uintptr_t)seg_ptr_dev % 8 != 0)
    return fail("norm tables and indices must be aligned to their type");

  // !live: no update can contribute, every destination reduces an empty segment (add and mean give 0)
  SegSpec seg{nullptr, nullptr, 0, 0, size};
  if (live) {
    const int rc = dst.Resolve();
    if (rc != EULER_GPU_OK) return Drained(st, rc);
    seg = dst.seg();
  }
  const GcnCall c{x_dev, d, out_dev, seg,
                  MpwIndex{dst.perm(), gather_indices_dev, 1, rows > 0 ? (uint32_t)(rows - 1) : 0u},
                  GcnTables{norm_dst_dev, norm_src_dev, (uint32_t)rows},
                  GcnRoot{root_dev, root_dtype == EULER_GPU_F32, agg_scale, root_scale}};
  const bool out16 = out_dtype != EULER_GPU_F32;
  return Drained(st, mode == 0 ? LaunchMode<0>(st, c, in_dtype, out16) : LaunchMode<2>(st, c, in_dtype, out16));
}

}  // extern "C"
