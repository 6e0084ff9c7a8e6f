// Per-relation aggregation for gfx950 (RGCN's RelationConv, relation_conv.py:53-70, by linearity:
// mean_e W[t_e] x_e = (sum_t W_t * sum_{e: t_e = t} x_e) / deg): the reduce of gathered rows per
// (destination, relation) into out [size, R, d], which one dense GEMM then multiplies - and its
// C-ABI entry point.  The arithmetic of a destination (validity, the four modes, the order of the
// folds, the batches of loads) is RelationReduceDest of mp_relation.h; the kernels here only
// decide which lane holds what, exactly as the segment reduces of mp_kernels.hip and
// mp_half_kernels.hip do:
//
//  - RelationReduceVecKernel: d / 4 lanes (fp32) or d / 8 lanes (bf16 / fp16) own one destination,
//    each N = 4 / 8 adjacent columns through 16-byte loads, 64 / lanes destinations a wave.  For
//    16-byte aligned tables with d % N == 0 and d / N a divisor of 64.
//  - RelationReduceKernel: a wave-slot per destination, one column per lane (any d, any alignment).
//
// Both keep `float acc[N]` of ONE bucket per lane and store a bucket when its relation is done:
// no LDS, no atomics, no scratch, R buckets written once each (the empty ones included).  Lanes of
// one destination read the same index words (one address: a broadcast); in the 16-byte-lane kernel
// they share the type column through a ballot (RelGroupScan).  The grid strides over the
// destinations with the block cap of the sibling reduces.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_fns.h"
#include "device_mem.h"
#include "half_cvt.h"
#include "mp_relation.h"
#include "mp_segments.h"

namespace euler_gpu {
namespace {

struct RelArgs {
  const void* params;
  SegSpec seg;
  MpwIndex ix;
  const int32_t* type;      // [e], by input position
  int32_t num_relations;
  int64_t e;
  int64_t d;
  void* out;                // [size, R, d]
  int32_t* counts;          // [size, R] or nullptr
};

template <typename Ops> struct RelGroupScan;

// where a lane stands in the group of lanes that owns its destination (the 16-byte-lane kernel)
struct RelGroup {
  int32_t lanes;            // dv: lanes a destination
  int32_t lane;             // this lane's place among them
  int32_t shift;            // of the group's first lane in the wave
  int32_t my_type;          // the type of update b + lane, when the segment fits in one look
  bool one_look;            // segment length <= lanes: my_type holds the whole type column
};

template <int DT, int N>
struct RelOps {
  using Elem = std::conditional_t<DT == kF32, float, uint16_t>;
  using Raw = std::conditional_t<N == 1, Elem, std::conditional_t<N == 4, float4, uint4>>;
#if defined(EULER_GPU_REL_LINEAR_SCAN)
  using Scan = RelLinearScan<RelOps<DT, N>>;            // (an experiment's build)
#else
  using Scan = std::conditional_t<N == 1, RelLinearScan<RelOps<DT, N>>, RelGroupScan<RelOps<DT, N>>>;
#endif
  MpwIndex ix;
  const int32_t* type;
  const Raw* tab; int64_t stride; int64_t c;            // in units of Raw
  RelGroup g;
  __device__ __forceinline__ int64_t Pos(int64_t p) const { return ix.Pos(p); }
  __device__ __forceinline__ int32_t Type(int64_t pos) const { return type[pos]; }
  __device__ __forceinline__ int64_t Row(int64_t pos) const { return ix.Row(pos); }
  __device__ __forceinline__ Raw Load(int64_t row) const { return tab[row * stride + c]; }
  __device__ __forceinline__ void Widen(const Raw& v, float f[N]) const {
    if constexpr (N == 4) {
      f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    } else if constexpr (N == 8) {
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      Widen8<DT>(w, f);
    } else if constexpr (DT == kF32) {
      f[0] = v;
    } else {
      f[0] = HalfCvt<DT>::Widen(v);
    }
  }
};

// The scan of the 16-byte-lane kernel.  The lanes of a destination run in lockstep, so they share
// the type column: lane j looks at update base + j (one load instruction for `lanes` updates, or
// none when the segment fits in one look and the types are already in a register), a ballot tells
// every lane which of them have relation t, and Next() takes the set bits in order - the positions
// and the order of RelLinearScan, for a handful of integer instructions per update instead of a
// load and a compare per update and relation (measured: DESIGN 4.13).  Groups of one wave scan
// different destinations; a ballot counts the active lanes only and each group reads its own bits.
template <typename Ops>
struct RelGroupScan {
  const Ops& o;
  int64_t base, en;
  int32_t t;
  uint64_t mask;            // bit j: update base + j has relation t
  static __device__ __forceinline__ uint64_t Mine(const Ops& o, bool flag) {
    const uint64_t m = __ballot(flag) >> o.g.shift;
    return o.g.lanes == 64 ? m : m & ((1ull << o.g.lanes) - 1);
  }
  static __device__ __forceinline__ int32_t TypeAt(const Ops& o, int64_t base, int64_t en) {
    if (o.g.one_look) return o.g.my_type;
    const int64_t p = base + o.g.lane;
    return p < en ? o.Type(o.Pos(p)) : -1;
  }
  __device__ __forceinline__ RelGroupScan(const Ops& ops, int64_t b, int64_t end, int32_t rel)
      : o(ops), base(b), en(end), t(rel), mask(0) {
    if (b < end) mask = Mine(o, TypeAt(o, base, en) == t);
  }
  __device__ __forceinline__ bool Next(int64_t* pos) {
    while (mask == 0) {
      base += o.g.lanes;
      if (base >= en) return false;
      mask = Mine(o, TypeAt(o, base, en) == t);
    }
    const int32_t bit = __ffsll((unsigned long long)mask) - 1;
    mask &= mask - 1;
    *pos = o.Pos(base + bit);
    return true;
  }
  static __device__ __forceinline__ int32_t CountValid(const Ops& o, int64_t b, int64_t en, int32_t num_relations) {
    int32_t n = 0;
    for (int64_t base = b; base < en; base += o.g.lanes)
      n += __popcll(Mine(o, (uint32_t)TypeAt(o, base, en) < (uint32_t)num_relations));
    return n;
  }
};

// the N columns of bucket (r, t): one rounding at the store when the output is 16-bit
template <int DT, bool OUT16, int N>
struct RelSink {
  void* out; int32_t* counts;
  int64_t bucket0;                  // r * R
  int64_t stride; int64_t c;        // in units of N columns
  bool lead;                        // the lane that writes the destination's counts
  __device__ __forceinline__ void Store(int32_t t, const float acc[N], int32_t cnt) const {
    const int64_t slot = (bucket0 + t) * stride + c;
    if constexpr (N == 4) {
      static_cast<float4*>(out)[slot] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else if constexpr (N == 8) {
      if constexpr (OUT16) {
        uint32_t w[4];
        Narrow8<DT>(acc, w);
        static_cast<uint4*>(out)[slot] = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
        float4* o = static_cast<float4*>(out) + slot * 2;
        o[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        o[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
      }
    } else if constexpr (OUT16) {
      static_cast<uint16_t*>(out)[slot] = HalfCvt<DT>::Narrow(acc[0]);
    } else {
      static_cast<float*>(out)[slot] = acc[0];
    }
    if (lead && counts != nullptr) counts[bucket0 + t] = cnt;
  }
};

// (seg_ptr comes from the caller: positions are clamped to [0, e])
__device__ __forceinline__ void ClampedBounds(const RelArgs& A, int64_t r, int64_t* b, int64_t* en) {
  SegBounds(A.seg, r, b, en);
  *b = *b < 0 ? 0 : (*b > A.e ? A.e : *b);
  *en = *en < *b ? *b : (*en > A.e ? A.e : *en);
}

// blockDim = (64, 4): a wave-slot per destination, one column per lane
template <int MODE, int DT, bool OUT16>
__global__ __launch_bounds__(256) void RelationReduceKernel(const RelArgs A) {
  using Ops = RelOps<DT, 1>;
  const int32_t size = A.seg.size;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; r < size;
       r += (int64_t)gridDim.x * blockDim.y) {
    int64_t b, en;
    ClampedBounds(A, r, &b, &en);
    for (int64_t c = threadIdx.x; c < A.d; c += 64) {
      const Ops ops{A.ix, A.type, static_cast<const typename Ops::Raw*>(A.params), A.d, c, RelGroup{}};
      RelSink<DT, OUT16, 1> sink{A.out, A.counts, r * A.num_relations, A.d, c, c == 0};
      RelationReduceDest<MODE, 1>(ops, b, en, A.num_relations, sink);
    }
  }
}

// dv = d / N lanes a destination (N = 4 fp32, 8 16-bit), 64 / dv destinations a wave
template <int MODE, int DT, bool OUT16, int N>
__global__ __launch_bounds__(256) void RelationReduceVecKernel(const RelArgs A, const int32_t dv) {
  using Ops = RelOps<DT, N>;
  const int32_t size = A.seg.size;
  const int32_t rows_per_wave = 64 / dv;
  const int32_t sub = threadIdx.x / dv, cl = threadIdx.x - sub * dv;
  const int64_t rows_per_block = (int64_t)blockDim.y * rows_per_wave;
  Ops ops{A.ix, A.type, static_cast<const typename Ops::Raw*>(A.params), dv, cl, RelGroup{dv, cl, sub * dv, -1, false}};
  for (int64_t r = (int64_t)blockIdx.x * rows_per_block + threadIdx.y * rows_per_wave + sub;
       r < size; r += (int64_t)gridDim.x * rows_per_block) {
    int64_t b, en;
    ClampedBounds(A, r, &b, &en);
    // a segment no longer than the group (a sampled block's `count`): its types are read ONCE,
    // one per lane, and stay in a register for all R relations
    ops.g.one_look = en - b <= dv;
    if (ops.g.one_look) ops.g.my_type = b + cl < en ? ops.Type(ops.Pos(b + cl)) : -1;
    RelSink<DT, OUT16, N> sink{A.out, A.counts, r * A.num_relations, dv, cl, cl == 0};
    RelationReduceDest<MODE, N>(ops, b, en, A.num_relations, sink);
  }
}

template <int MODE, int DT, bool OUT16>
int LaunchRelation(hipStream_t st, const RelArgs& A) {
  constexpr int N = DT == kF32 ? 4 : 8;
  const LaneShape s = RowLaneShape(A.seg.size, A.d, N, 0, A.params, A.out);
  if (s.vec) {
    hipLaunchKernelGGL((RelationReduceVecKernel<MODE, DT, OUT16, N>), dim3(s.blocks), dim3(64, 4), 0, st, A,
                       (int32_t)s.dv);
  } else {
    hipLaunchKernelGGL((RelationReduceKernel<MODE, DT, OUT16>), dim3(s.blocks), dim3(64, 4), 0, st, A);
  }
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int MODE>
int DispatchRelation(hipStream_t st, int32_t in_dtype, int32_t out_dtype, const RelArgs& A) {
  if (in_dtype == EULER_GPU_F32) return LaunchRelation<MODE, kF32, false>(st, A);
  if (in_dtype == EULER_GPU_BF16)
    return out_dtype == EULER_GPU_F32 ? LaunchRelation<MODE, kBF16, false>(st, A)
                                      : LaunchRelation<MODE, kBF16, true>(st, A);
  return out_dtype == EULER_GPU_F32 ? LaunchRelation<MODE, kF16, false>(st, A)
                                    : LaunchRelation<MODE, kF16, true>(st, A);
}

int RelFail(const std::string& why) { return Fail(EULER_GPU_EINVAL, "relation_reduce: " + why); }

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" int euler_gpu_relation_reduce(void* stream, int32_t mode, const void* params_dev, int32_t in_dtype,
                                         int64_t params_rows, const void* gather_dev, int32_t gather_is_ids,
                                         const int32_t* edge_type_dev, int32_t num_relations,
                                         const int32_t* indices_dev, const int64_t* seg_ptr_dev, int64_t count,
                                         int64_t e, int64_t d, int32_t size, void* out_dev, int32_t out_dtype,
                                         int32_t* counts_dev) {
  if (mode < 0 || mode > 3) return RelFail("mode is 0 add, 1 max, 2 mean over the destination, 3 mean over the bucket");
  if (num_relations < 1) return RelFail("num_relations < 1");
  if (e < 0 || d < 0 || size < 0 || count < 0 || params_rows < 0) return RelFail("bad shape");
  if (!KnownDtype(in_dtype)) return RelFail(std::string("unknown dtype") + kDtypeCodes);
  if (out_dtype != EULER_GPU_F32 && out_dtype != in_dtype) return RelFail("out_dtype is fp32 or in_dtype");
  SegDest dst((hipStream_t)stream, indices_dev, seg_ptr_dev, count, e, size);
  if (const char* why = dst.FormError()) return RelFail(why);
  if (const char* why = dst.LengthError()) return RelFail(why);
  if ((int64_t)size * num_relations >= (1LL << 31)) return RelFail("size * num_relations >= 2^31");
  if (mode >= 2 && (e >= (1LL << 24) || count >= (1LL << 24)))
    return RelFail("a mean needs fewer than 2^24 updates (its counts are exact fp32)");
  if (size == 0 || d == 0) return EULER_GPU_OK;
  if (!out_dev) return RelFail("null buffer");
  if (e > 0) {
    if (!params_dev || !edge_type_dev) return RelFail("null buffer");
    if (params_rows < 1 || (gather_dev == nullptr && params_rows < e))
      return RelFail("the table has fewer rows than the updates read");
  }
  const int rc = dst.Resolve();
  if (rc != EULER_GPU_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  // every index is clamped to the table's last row (int64 ids: the low word, as
  // euler_gpu_gather_segment_reduce_ids): no update reads outside the table
  const uint32_t row_max = (uint32_t)std::min<int64_t>(params_rows > 0 ? params_rows - 1 : 0, 0x7FFFFFFF);
  const MpwIndex ix{dst.perm(), static_cast<const int32_t*>(gather_dev), gather_is_ids ? 2 : 1, row_max};
  const RelArgs A{params_dev, dst.seg(), ix, edge_type_dev, num_relations, e, d, out_dev, counts_dev};
  if (mode == 0) return DispatchRelation<kRelAdd>(st, in_dtype, out_dtype, A);
  if (mode == 1) return DispatchRelation<kRelMax>(st, in_dtype, out_dtype, A);
  if (mode == 2) return DispatchRelation<kRelMeanDst>(st, in_dtype, out_dtype, A);
  return DispatchRelation<kRelMeanRel>(st, in_dtype, out_dtype, A);
}
