// Where the updates of a destination are, for the segment reduces of mp_kernels.hip (fp32) and
// mp_half_kernels.hip (bf16 / fp16 storage): device functions shared by both.
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

#pragma GCC visibility push(hidden)
// mp_kernels.hip: groups the e scatter keys by destination for the reduces.  Keys that are already
// non-decreasing (one look, one host wait) are used as they are: *keys = idx, *perm = nullptr.
// Otherwise a stable sort of (key, position) into `scratch`: *keys = the grouped keys, (*perm)[p] =
// the original position of the p-th grouped update.
int GroupScatterKeys(hipStream_t st, const int32_t* idx, int64_t e, StreamBuf* scratch,
                     const int32_t** keys, const uint32_t** perm);
// mp_kernels.hip: the argument checks every weighted entry shares (mode 0..2, heads >= 1, heads | d)
int CheckWeightedShape(const char* what, int32_t mode, int64_t d, int32_t heads);
#pragma GCC visibility pop

}  // namespace euler_gpu
