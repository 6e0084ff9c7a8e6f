// The owners of device memory in the host code of libeuler_gpu.so.  Each wraps exactly one HIP
// call pair - no pool, no cache, no size classes:
//   DevBuf     a per-call temporary from hipMalloc, returned with hipFree
//   StreamBuf  a per-call temporary from hipMallocAsync, returned with hipFreeAsync on its stream
//   AllocList  the blocks of one build, returned on failure, handed to the graph on success
// An entry point declares a guard where it allocates and has no raw allocate / free pair: every
// return, an EG_HIP in the middle included, then gives the block back.
#pragma once

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "common.h"

namespace euler_gpu {
#pragma GCC visibility push(hidden)      // helpers of the host code, not names of the library

// Makes `dev` the current device for a scope.
struct DeviceGuard {
  int prev = 0;
  explicit DeviceGuard(int dev) { (void)hipGetDevice(&prev); (void)hipSetDevice(dev); }
  ~DeviceGuard() { (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// The launch error, then a device-wide wait: for builds, which run on the null stream.
inline int CheckLaunch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return Fail(EULER_GPU_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  const hipError_t s = hipDeviceSynchronize();
  if (s != hipSuccess) return Fail(EULER_GPU_EHIP, std::string(what) + ": " + hipGetErrorString(s));
  return EULER_GPU_OK;
}

class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  hipError_t alloc(size_t bytes) { reset(); return hipMalloc(&p_, bytes); }
  // (a status is dropped: a free can only fail after an error the caller's checks report)
  void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
  template <typename T = void> T* as() const { return static_cast<T*>(p_); }

 private:
  void* p_ = nullptr;
};

class StreamBuf {
 public:
  explicit StreamBuf(hipStream_t st) : st_(st) {}
  StreamBuf(const StreamBuf&) = delete;
  StreamBuf& operator=(const StreamBuf&) = delete;
  ~StreamBuf() { reset(); }
  hipError_t alloc(size_t bytes) { reset(); return hipMallocAsync(&p_, bytes, st_); }
  void reset() { if (p_) (void)hipFreeAsync(p_, st_); p_ = nullptr; }
  template <typename T = void> T* as() const { return static_cast<T*>(p_); }

 private:
  void* p_ = nullptr;
  hipStream_t st_;
};

// (pointer, bytes) of every block a graph, an edge store or a label index owns
using OwnedBlocks = std::vector<std::pair<void*, int64_t>>;

struct AllocList {
  OwnedBlocks list;
  int rc = EULER_GPU_OK;
  const char* prefix;           // of the error messages: "", "edge store: ", "graph labels: "
  explicit AllocList(const char* message_prefix) : prefix(message_prefix) {}
  template <typename T>
  T* Alloc(size_t count) {
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
      rc = Fail(EULER_GPU_ENOMEM, std::string(prefix) + "hipMalloc(" + std::to_string(bytes) +
                                      "): " + hipGetErrorString(e));
      return nullptr;
    }
    list.emplace_back(p, (int64_t)bytes);
    return (T*)p;
  }
  template <typename T>
  T* Upload(const T* host, size_t count) {
    T* d = Alloc<T>(count);
    if (d && count > 0) {
      const hipError_t e = hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        rc = Fail(EULER_GPU_EHIP, std::string(prefix) + "hipMemcpy H2D: " + hipGetErrorString(e));
        return nullptr;
      }
    }
    return d;
  }
  void Release() {
    for (auto& p : list) (void)hipFree(p.first);
    list.clear();
  }
  // Appends the blocks to an owner's list; returns their bytes (the owner's byte count grows by it).
  int64_t HandOver(OwnedBlocks* owner) {
    int64_t bytes = 0;
    for (auto& p : list) { owner->push_back(p); bytes += p.second; }
    list.clear();
    return bytes;
  }
};

// Returns an owner's blocks; returns their bytes (the owner's byte count shrinks by it).
inline int64_t FreeBlocks(OwnedBlocks* owner) {
  int64_t bytes = 0;
  for (auto& p : *owner) { (void)hipFree(p.first); bytes += p.second; }
  owner->clear();
  return bytes;
}

// graph_build.hip: a finished build's blocks become the graph's (and count in its bytes), under the
// lock the index builds commit under - for builds that run outside graph_build.hip.
void AdoptBlocks(euler_gpu_graph* g, AllocList* blocks);

#pragma GCC visibility pop
}  // namespace euler_gpu
