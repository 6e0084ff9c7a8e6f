// The segment reduces of mp_kernels.hip (fp32) and mp_half_kernels.hip (bf16 / fp16 storage), shared
// by both and by the ops built on them (edge_softmax, segment_attention, relation_reduce,
// gather_reduce_norm):
//  - device: where the updates of a destination are (SegSpec / SegBounds);
//  - host: the launch shape of a reduce with a wave-slot per destination row (RowLaneShape); the
//    destinations of a call (SegDest): the rule on its three forms, the grouping of scatter keys and
//    the SegSpec, for every op above; and the ONE path of the sixteen scatter_* / gather_scatter* /
//    gather_segment_reduce* entries: each fills an MpReduceCall and calls RunMpReduce, which checks
//    it (CheckMpReduce: the only argument ladder), resolves its SegDest, builds the MpwIndex once and
//    picks the launcher by (weighted, dtype, mode).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_mem.h"

namespace euler_gpu {

__device__ __forceinline__ int64_t LowerBound(const int32_t* a, int64_t n,
                                              int32_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Segment [b, en) of destination r in the grouped key array.  Sampled blocks
// scatter `count` updates to every destination in order (keys = 0,0,..,1,1,..): the
// proportional guess r * e / size is then exact and costs two loads; anything else
// falls back to the bisection.
__device__ __forceinline__ int64_t SegStart(const int32_t* keys, int64_t e, int32_t size,
                                            int64_t r) {
  // r == size: the end of the LAST destination's segment - the first key >= size, not e:
  // out-of-range scatter indices (undefined behaviour in the reference,
  // tf_euler/kernels/scatter_op.cc:27-105) are left out instead of being folded into
  // row size - 1
  if (r >= size) return (e > 0 && keys[e - 1] >= size) ? LowerBound(keys, e, size) : e;
  const int64_t g = r * e / size;
  if ((g == 0 || keys[g - 1] < (int32_t)r) && (g == e || keys[g] >= (int32_t)r)) return g;
  return LowerBound(keys, e, (int32_t)r);
}

// Where destination r's updates are: a grouped key array (scatter: bisected / guessed),
// explicit offsets (segment reduce), or `count` updates per destination.
struct SegSpec {
  const int32_t* keys;
  const int64_t* ptr;      // [size + 1] when keys == nullptr (nullptr: uniform `count`)
  int64_t count;
  int64_t e;
  int32_t size;
};

__device__ __forceinline__ void SegBounds(const SegSpec& s, int64_t r, int64_t* b, int64_t* en) {
  if (s.keys != nullptr) {
    *b = SegStart(s.keys, s.e, s.size, r);
    *en = SegStart(s.keys, s.e, s.size, r + 1);
  } else if (s.ptr != nullptr) {
    *b = s.ptr[r];
    *en = s.ptr[r + 1];
  } else {
    *b = r * s.count;
    *en = *b + s.count;
  }
}

// The launch shape of a reduce with blockDim = (64, 4) and a wave-slot per destination row.  The
// vector form - a lane owns N adjacent columns (one 16-byte access), dv = d / N lanes a row,
// 64 / dv rows a wave - serves d % N == 0 with dv a divisor of 64, rows on 16-byte boundaries and,
// for the weighted kernels, N | dh so that a lane's columns share a head (dh = 0: no heads); every
// other d takes the element form, a column per lane.  At most 256 * 32 blocks: the rows are strided.
struct LaneShape {
  bool vec;
  int64_t dv;        // lanes of a row in the vector form
  unsigned blocks;
};

inline LaneShape RowLaneShape(int32_t size, int64_t d, int n, int64_t dh, const void* params,
                              const void* out) {
  const int64_t dv = d / n;
  const bool vec = d % n == 0 && dv <= 64 && 64 % dv == 0 && dh % n == 0 &&
                   ((uintptr_t)params % 16 == 0) && ((uintptr_t)out % 16 == 0);
  const int64_t rows_per_block = vec ? 4 * (64 / dv) : 4;
  int64_t blocks = ((int64_t)size + rows_per_block - 1) / rows_per_block;
  if (blocks > 256 * 32) blocks = 256 * 32;
  return LaneShape{vec, dv, (unsigned)blocks};
}

struct MpwIndex;      // mp_weighted.h

#pragma GCC visibility push(hidden)      // from here on: helpers of the host code, not names of the library
// The destinations of one call as an entry point receives them - `indices` (a scatter key per update),
// `seg_ptr` ([size + 1] offsets) or `count` (updates per destination) - from the rule on which forms
// may come together to the SegSpec the kernels read.  An entry declares one where its `scratch` used to
// be: it owns the grouped keys of the unsorted path, so it lives as long as the launches that read them.
class SegDest {
 public:
  enum Forms {
    kOneForm,           // exactly one of the three
    kNoFormWhenEmpty,   // ... or none when e == 0: the keys of an empty tensor are null (gather_reduce_norm)
  };
  SegDest(hipStream_t st, const int32_t* indices, const int64_t* seg_ptr, int64_t count, int64_t e, int32_t size)
      : st_(st), scratch_(st), indices_(indices), seg_{indices, seg_ptr, count, e, size} {}
  // The two shared rules of a ladder, host arithmetic only: nullptr, or what the entry's message says
  // after its own name.  Two calls, because every ladder has its empty case (and some their null
  // checks) between them.
  const char* FormError(Forms allowed = kOneForm) const {
    const int forms = (indices_ != nullptr) + (seg_.ptr != nullptr) + (seg_.count > 0);
    if (forms != 1 && !(forms == 0 && allowed == kNoFormWhenEmpty && seg_.e == 0))
      return "pass exactly one of indices, seg_ptr and count";
    if (seg_.count > 0 && seg_.e != (int64_t)seg_.size * seg_.count) return "e is not size * count";
    return nullptr;
  }
  // (the sort of the keys and the positions of the updates are 32-bit)
  const char* LengthError() const { return seg_.e >= (1LL << 31) ? "e >= 2^31" : nullptr; }
  // mp_kernels.hip: groups the keys of the `indices` form (GroupScatterKeys: one look when they are
  // sorted already, one host wait); nothing to do for the other two.  Before it, seg() has the keys as
  // they came and perm() is null.
  int Resolve();
  const SegSpec& seg() const { return seg_; }
  const uint32_t* perm() const { return perm_; }   // the original position of the p-th grouped update, or null

 private:
  hipStream_t st_;
  StreamBuf scratch_;
  const int32_t* indices_;
  SegSpec seg_;
  const uint32_t* perm_ = nullptr;
};

// One call of a scatter_* / gather_scatter* / gather_segment_reduce* entry, as its adapter in
// mp_kernels.hip / mp_half_kernels.hip states it: {name, mode, params, d, size, out}, then what the
// entry has beyond an fp32 reduce of consecutive rows.
enum MpGather {
  kNoGatherArg,     // scatter_*: update p is row p
  kGatherOrNull,    // int32 indices; nullptr: update p is row p
  kGatherNeeded,    // int32 indices, nullptr refused
  kGatherIds,       // int64 ids read in place (index = low word, clamped to the last row), nullptr refused
};

struct MpReduceCall {
  const char* name;          // of the entry, as its messages begin
  int32_t mode;              // 0 add, 1 max, 2 mean
  const void* params;        // the table, or the updates themselves
  int64_t d;
  int32_t size;
  void* out;
  bool typed = false;        // a `_t` entry: dtype codes, and weights whose alignment is not their C type's
  int32_t in_dtype = EULER_GPU_F32, out_dtype = EULER_GPU_F32, w_dtype = EULER_GPU_F32;
  MpGather gather_kind = kNoGatherArg;
  const void* gather = nullptr;
  int64_t params_rows = 0;   // kGatherIds: rows of the table
  bool keyed = false;        // destinations by scatter key (keys, e); else by seg_ptr, or `count` each
  const int32_t* keys = nullptr;
  int64_t e = 0;
  const int64_t* seg_ptr = nullptr;
  int64_t count = 0;
  bool weighted = false;
  const void* w = nullptr;   // [E, heads]
  int32_t heads = 1;
  const float* fp8_scale = nullptr;   // fp8: params is the q [rows, d] of an Fp8Rows table, this its [d] scales
  bool fp8 = false;                   // (an internal storage kind: no dtype code of the C ABI names it)

  MpReduceCall& Typed(int32_t in, int32_t out_dt) { typed = true; in_dtype = in; out_dtype = out_dt; return *this; }
  // an fp8_* entry: out_dtype (and w_dtype) any of the three codes
  MpReduceCall& Fp8(const float* scale, int32_t out_dt) { fp8 = true; fp8_scale = scale; out_dtype = out_dt; return *this; }
  MpReduceCall& Gather(MpGather kind, const void* g, int64_t rows = 0) {
    gather_kind = kind; gather = g; params_rows = rows; return *this;
  }
  MpReduceCall& Keys(const int32_t* k, int64_t n) { keyed = true; keys = k; e = n; return *this; }
  MpReduceCall& Segments(const int64_t* ptr, int64_t n) { seg_ptr = ptr; count = n; return *this; }
  MpReduceCall& Weights(const void* w_dev, int32_t h, int32_t dt = EULER_GPU_F32) {
    weighted = true; w = w_dev; heads = h; w_dtype = dt; return *this;
  }
};

// mp_kernels.hip: the argument ladder, in its one order: dtype codes and weight alignment; mode,
// heads, heads | d; negative shape; size == 0 || d == 0 (*nothing_to_do: OK, nothing is touched - the
// callers hand over null for empty tensors, so the null check comes after); null buffers; e >= 2^31;
// the 2^24 limits of a mean; the 2^31 rows of an id-addressed table; 2-byte alignment of 16-bit
// data (fp8: the output's alignment to its type).  Host arithmetic and Fail() only: no HIP call.
int CheckMpReduce(const MpReduceCall& c, bool* nothing_to_do);
int RunMpReduce(hipStream_t st, const MpReduceCall& c);
// mp_half_kernels.hip: the launchers over bf16 / fp16 rows (c checked, seg and ix built)
int ReduceHalf(hipStream_t st, const MpReduceCall& c, const SegSpec& seg, const MpwIndex& ix);
int WeightedReduceHalf(hipStream_t st, const MpReduceCall& c, const SegSpec& seg, const MpwIndex& ix);
#pragma GCC visibility pop

}  // namespace euler_gpu
