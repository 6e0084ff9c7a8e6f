// The device pieces that the in-place stores (embed_store_kernels.hip) and the sparse-row
// optimiser steps (sparse_optim_kernels.hip) share: chunk loads and stores, the (key, position)
// kernel, the stable radix sort that groups the occurrences, and the eight-ahead walk over a
// segment.  embed_store.h states what a key, a segment and an owner are.
//
// Everything sits in an anonymous namespace: each of the two translation units gets its own copy
// of the kernel and of the host functions, as it had when they lived in embed_store_kernels.hip.
// The argument structs of the two files differ, so EsAhead and GroupOccurrences take theirs as a
// template parameter; they use its ids, e, rows, row_index, m, keys and perm.
#pragma once

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "device_fns.h"
#include "device_mem.h"
#include "embed_store.h"

namespace euler_gpu {
namespace {

constexpr int kBytes[3] = {4, 2, 2};

// V adjacent elements as their bits: 16-byte (8-byte) accesses where the type and V allow
template <int DT, int V>
__device__ __forceinline__ void EsLoad(const void* base, int64_t at, uint32_t r[V]) {
  if constexpr (DT == kF32) {
    const uint32_t* p = static_cast<const uint32_t*>(base) + at;
    if constexpr (V == 1) {
      r[0] = *p;
    } else {
#pragma unroll
      for (int q = 0; q < V / 4; ++q) {
        const uint4 v = reinterpret_cast<const uint4*>(p)[q];
        r[4 * q] = v.x; r[4 * q + 1] = v.y; r[4 * q + 2] = v.z; r[4 * q + 3] = v.w;
      }
    }
  } else {
    const uint16_t* p = static_cast<const uint16_t*>(base) + at;
    if constexpr (V == 1) {
      r[0] = *p;
    } else if constexpr (V == 4) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      r[0] = v.x & 0xffffu; r[1] = v.x >> 16; r[2] = v.y & 0xffffu; r[3] = v.y >> 16;
    } else {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) { r[2 * q] = w[q] & 0xffffu; r[2 * q + 1] = w[q] >> 16; }
    }
  }
}

template <int DT, int V>
__device__ __forceinline__ void EsStore(void* base, int64_t at, const uint32_t r[V]) {
  if constexpr (DT == kF32) {
    uint32_t* p = static_cast<uint32_t*>(base) + at;
    if constexpr (V == 1) {
      *p = r[0];
    } else {
#pragma unroll
      for (int q = 0; q < V / 4; ++q)
        reinterpret_cast<uint4*>(p)[q] = make_uint4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
    }
  } else {
    uint16_t* p = static_cast<uint16_t*>(base) + at;
    if constexpr (V == 1) {
      *p = (uint16_t)r[0];
    } else if constexpr (V == 4) {
      *reinterpret_cast<uint2*>(p) = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
    } else {
      *reinterpret_cast<uint4*>(p) =
          make_uint4(r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16));
    }
  }
}

__global__ __launch_bounds__(256) void EsKeysKernel(const int64_t* __restrict__ ids, int64_t e, int64_t rows,
                                                    const int32_t* __restrict__ row_index, int64_t m,
                                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ pos) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < e; p += stride) {
    keys[p] = EsKey(ids[p], rows, EsSourceLive(p, row_index, m));
    pos[p] = (uint32_t)p;
  }
}

// K sorted entries from q on: which of them belong to the segment of `key` (ok), and their
// positions.  An entry past the segment stands in as entry i (the head), which is always valid.
template <int K, typename Args>
__device__ __forceinline__ void EsAhead(const Args& a, uint64_t key, int64_t i, int64_t q, bool ok[K],
                                        int64_t pos[K]) {
#pragma unroll
  for (int x = 0; x < K; ++x) ok[x] = q + x < a.e && a.keys[q + x < a.e ? q + x : i] == key;
#pragma unroll
  for (int x = 0; x < K; ++x) pos[x] = a.perm[ok[x] ? q + x : i];
}

// (key, position) of every occurrence, stably sorted by key, into `pairs` (released by its owner)
template <typename Args>
int GroupOccurrences(hipStream_t st, Args* a, StreamBuf* pairs) {
  const size_t n = (size_t)a->e;
  EG_HIP(pairs->alloc(n * (8 + 8 + 4 + 4) + 64));
  uint64_t* keys_in = pairs->as<uint64_t>();
  uint64_t* keys_out = keys_in + n;
  uint32_t* pos_in = reinterpret_cast<uint32_t*>(keys_out + n);
  uint32_t* pos_out = pos_in + n;
  int64_t blocks = ((int64_t)n + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(EsKeysKernel, dim3((unsigned)blocks), dim3(256), 0, st, a->ids, a->e, a->rows, a->row_index,
                     a->m, keys_in, pos_in);
  EG_HIP(hipGetLastError());
  const int bits = EsKeyBits(a->rows);
  size_t tmp_bytes = 0;
  EG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys_in, keys_out, pos_in, pos_out, (int)n, 0, bits,
                                            st));
  StreamBuf tmp(st);          // (the library's scratch goes back before the store kernel runs)
  EG_HIP(tmp.alloc(tmp_bytes + 16));
  EG_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.as(), tmp_bytes, keys_in, keys_out, pos_in, pos_out, (int)n, 0, bits,
                                            st));
  a->keys = keys_out;
  a->perm = pos_out;
  return EULER_GPU_OK;
}

}  // namespace
}  // namespace euler_gpu
