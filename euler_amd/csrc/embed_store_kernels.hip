// In-place embedding stores on gfx950 - update / add / take of embed_store.h, which states the
// contract - with their C-ABI entry points.
//
// A call is: one kernel that writes (key, position) per occurrence, one stable radix sort of those
// pairs over the bits `rows` needs (rocPRIM via hipCUB - the one library primitive used here),
// and one kernel in which every segment of equal keys has ONE owner.  A wave looks at 64 adjacent
// sorted entries at a time (one coalesced load of the keys, one ballot of the entries that start
// a task); the tasks of a window go round robin to the wave's 64 / L groups of L lanes, L = the
// power of two >= d / V, so narrow rows fill the wave.  The owner reads the table row once, walks
// its segment in position order - keys, positions and source rows are loaded eight entries ahead
// of the add chain, which is sequential by definition - and writes the row once.  No lane of any
// other task reads or writes that table row.  Nothing here waits on the host: the three entries
// only enqueue, scratch comes from StreamBuf and goes back in stream order on every exit, and
// every check precedes the first write to the table.  take without clear needs no grouping: it is
// a plain lookup per occurrence.  The chunk loads and stores, the key kernel, the sort and the
// eight-ahead walk live in embed_group.h, which the sparse-row optimiser steps share.
#include "embed_group.h"

namespace euler_gpu {
namespace {

struct EsArgs {
  void* table; int64_t rows, d;
  const int64_t* ids; int64_t e;
  const void* values; int64_t m; const int32_t* row_index; int64_t count;     // update / add
  void* out; int32_t clear;                                                    // take
  const uint64_t* keys; const uint32_t* perm;                                  // the sorted pairs
  int32_t log_l;
};

// The task that sorted entry i starts (update: ends), run by the L lanes of a group; l = the
// lane's number in its group.  DV: the dtype of values (update, add) or of out (take).
template <int OP, int DT, int DV, int V>
__device__ __forceinline__ void EsTask(const EsArgs& a, int64_t i, int32_t l, int32_t lanes, int32_t chunks) {
  if constexpr (OP == kEsTake) {
    const int64_t id = a.ids[i];
    const bool in = EsInRange(id, a.rows);
    for (int32_t j = l; j < chunks; j += lanes) {
      uint32_t r[V];
      if (in) EsLoad<DT, V>(a.table, id * a.d + (int64_t)j * V, r);
#pragma unroll
      for (int k = 0; k < V; ++k) r[k] = in ? EsConvert<DT, DV>(r[k]) : 0u;
      EsStore<DV, V>(a.out, i * a.d + (int64_t)j * V, r);
    }
  } else if constexpr (OP == kEsUpdate) {
    const int64_t id = (int64_t)a.keys[i];
    const int64_t src = EsSourceRow(a.perm[i], a.row_index, a.count);
    for (int32_t j = l; j < chunks; j += lanes) {
      uint32_t r[V];
      EsLoad<DV, V>(a.values, src * a.d + (int64_t)j * V, r);
#pragma unroll
      for (int k = 0; k < V; ++k) r[k] = EsConvert<DV, DT>(r[k]);
      EsStore<DT, V>(a.table, id * a.d + (int64_t)j * V, r);
    }
  } else if constexpr (OP == kEsAdd) {
    const uint64_t key = a.keys[i];
    for (int32_t j = l; j < chunks; j += lanes) {
      const int64_t at = (int64_t)key * a.d + (int64_t)j * V;
      uint32_t r[V];
      float acc[V];
      EsLoad<DT, V>(a.table, at, r);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = EsWiden<DT>(r[k]);
      // the adds stay in position order; only the loads of eight entries are issued together
      for (int64_t q = i;; q += 8) {
        bool ok[8];
        int64_t pos[8];
        uint32_t v[8][V];
        EsAhead<8>(a, key, i, q, ok, pos);
#pragma unroll
        for (int x = 0; x < 8; ++x)
          EsLoad<DV, V>(a.values, EsSourceRow(pos[x], a.row_index, a.count) * a.d + (int64_t)j * V, v[x]);
#pragma unroll
        for (int x = 0; x < 8; ++x) {
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] = ok[x] ? EsAddStep<DV>(acc[k], v[x][k]) : acc[k];
        }
        if (!ok[7]) break;
      }
#pragma unroll
      for (int k = 0; k < V; ++k) r[k] = EsNarrow<DT>(acc[k]);
      EsStore<DT, V>(a.table, at, r);
    }
  } else {                                        // kEsTakeClear
    const uint64_t key = a.keys[i];
    const bool in = key < (uint64_t)a.rows;
    for (int32_t j = l; j < chunks; j += lanes) {
      const int64_t at = (int64_t)key * a.d + (int64_t)j * V;
      uint32_t r[V], z[V];
#pragma unroll
      for (int k = 0; k < V; ++k) z[k] = 0u;
      if (!in) {                                  // a removed id reads as a row of +0
        EsStore<DV, V>(a.out, (int64_t)a.perm[i] * a.d + (int64_t)j * V, z);
        continue;
      }
      EsLoad<DT, V>(a.table, at, r);
#pragma unroll
      for (int k = 0; k < V; ++k) r[k] = EsConvert<DT, DV>(r[k]);
      // the old row to every occurrence of the segment
      for (int64_t q = i;; q += 8) {
        bool ok[8];
        int64_t pos[8];
        EsAhead<8>(a, key, i, q, ok, pos);
#pragma unroll
        for (int x = 0; x < 8; ++x)
          if (ok[x]) EsStore<DV, V>(a.out, pos[x] * a.d + (int64_t)j * V, r);
        if (!ok[7]) break;
      }
      if (a.clear) EsStore<DT, V>(a.table, at, z);
    }
  }
}

template <int OP, int DT, int DV, int V>
__global__ __launch_bounds__(256) void EsStoreKernel(const EsArgs a) {
  const int32_t lanes = 1 << a.log_l, groups = 64 >> a.log_l;
  const int32_t lane = threadIdx.x & 63;
  const int32_t g = lane >> a.log_l, l = lane & (lanes - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int32_t chunks = (int32_t)(a.d / V);
  for (int64_t base = wave * 64; base < a.e; base += waves * 64) {       // (the same trips for a whole wave)
    const int64_t i = base + lane;
    bool task = i < a.e;
    if constexpr (OP != kEsTake) {
      if (task) {
        const bool live = a.keys[i] < (uint64_t)a.rows;
        if constexpr (OP == kEsUpdate) task = live && EsIsTail(a.keys, i, a.e);
        else if constexpr (OP == kEsAdd) task = live && EsIsHead(a.keys, i);
        else task = !live || EsIsHead(a.keys, i);         // a removed id: every occurrence on its own
      }
    }
    uint64_t todo = __ballot(task);
    // group g takes the tasks g, g + groups, ... of the window
    for (int32_t x = 0; x < g && todo; ++x) todo &= todo - 1;
    while (todo) {
      EsTask<OP, DT, DV, V>(a, base + __builtin_ctzll(todo), l, lanes, chunks);
      for (int32_t x = 0; x < groups && todo; ++x) todo &= todo - 1;
    }
  }
}

template <int OP, int DT, int DV>
int LaunchStore(hipStream_t st, EsArgs a, const void* other) {
  const int32_t v = EsChunkWidth(a.d, (uintptr_t)a.table, kBytes[DT], (uintptr_t)other, kBytes[DV]);
  a.log_l = EsLogLanes(a.d / v);
  const int64_t waves = (a.e + 63) / 64;
  int64_t blocks = (waves + 3) / 4;
  if (blocks > 256 * 32) blocks = 256 * 32;
  const dim3 grid((unsigned)blocks), block(256);
  if (v == 8) hipLaunchKernelGGL((EsStoreKernel<OP, DT, DV, 8>), grid, block, 0, st, a);
  else if (v == 4) hipLaunchKernelGGL((EsStoreKernel<OP, DT, DV, 4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((EsStoreKernel<OP, DT, DV, 1>), grid, block, 0, st, a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int OP, int DT>
int DispatchOther(hipStream_t st, const EsArgs& a, const void* other, int32_t other_dtype) {
  if (other_dtype == EULER_GPU_F32) return LaunchStore<OP, DT, kF32>(st, a, other);
  return LaunchStore<OP, DT, DT>(st, a, other);
}

template <int OP>
int DispatchTable(hipStream_t st, const EsArgs& a, int32_t table_dtype, const void* other, int32_t other_dtype) {
  if (table_dtype == EULER_GPU_F32) return LaunchStore<OP, kF32, kF32>(st, a, other);
  if (table_dtype == EULER_GPU_BF16) return DispatchOther<OP, kBF16>(st, a, other, other_dtype);
  return DispatchOther<OP, kF16>(st, a, other, other_dtype);
}

// The checks the three entries share: the table, the ids and the other data buffer (values / out).
// -> EULER_GPU_OK with *run = false when there is nothing to do.
int CheckStoreArgs(const std::string& what, const EsArgs& a, int32_t table_dtype, const void* other,
                   int32_t other_dtype, bool* run) {
  *run = false;
  if (!KnownDtype(table_dtype) || !KnownDtype(other_dtype))
    return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (other_dtype != EULER_GPU_F32 && other_dtype != table_dtype)
    return Fail(EULER_GPU_EINVAL, what + ": values / out are fp32 or of the table's dtype");
  if (a.rows < 1) return Fail(EULER_GPU_EINVAL, what + ": a table with fewer than 1 row");
  if (a.e < 0 || a.d < 0) return Fail(EULER_GPU_EINVAL, what + ": e or d < 0");
  if (a.e >= (1LL << 31) || a.d >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, what + ": e or d >= 2^31");
  if (a.e == 0 || a.d == 0) return EULER_GPU_OK;
  if (!a.table || !a.ids || !other) return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  if ((uintptr_t)a.table % kBytes[table_dtype] != 0 || (uintptr_t)other % kBytes[other_dtype] != 0 ||
      (uintptr_t)a.ids % 8 != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  *run = true;
  return EULER_GPU_OK;
}

template <int OP>
int StoreWrite(const char* name, void* stream, void* table_dev, int32_t table_dtype, int64_t rows, int64_t d,
               const int64_t* ids_dev, int64_t e, const void* values_dev, int32_t values_dtype, int64_t m,
               const int32_t* row_index_dev, int64_t count) {
  const std::string what(name);
  EsArgs a{};
  a.table = table_dev; a.rows = rows; a.d = d; a.ids = ids_dev; a.e = e;
  a.values = values_dev; a.m = m; a.row_index = row_index_dev; a.count = count;
  if (row_index_dev && count != 0) return Fail(EULER_GPU_EINVAL, what + ": row_index and count both given");
  if (count < 0) return Fail(EULER_GPU_EINVAL, what + ": count < 0");
  if (m < 0) return Fail(EULER_GPU_EINVAL, what + ": m < 0");
  if (e >= 0 && count > 0 && (e % count != 0 || m != e / count))
    return Fail(EULER_GPU_EINVAL, what + ": count needs e % count == 0 and m == e / count");
  if (!row_index_dev && count == 0 && m != e) return Fail(EULER_GPU_EINVAL, what + ": values are [e, d]: m != e");
  if (row_index_dev && (uintptr_t)row_index_dev % 4 != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  bool run;
  const int rc = CheckStoreArgs(what, a, table_dtype, values_dev, values_dtype, &run);
  if (rc != EULER_GPU_OK || !run) return rc;
  hipStream_t st = (hipStream_t)stream;
  StreamBuf pairs(st);
  const int rg = GroupOccurrences(st, &a, &pairs);
  if (rg != EULER_GPU_OK) return rg;
  return DispatchTable<OP>(st, a, table_dtype, values_dev, values_dtype);
}

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" {

int euler_gpu_store_update(void* stream, void* table_dev, int32_t table_dtype, int64_t rows, int64_t d,
                           const int64_t* ids_dev, int64_t e, const void* values_dev, int32_t values_dtype,
                           int64_t m, const int32_t* row_index_dev, int64_t count) {
  return StoreWrite<kEsUpdate>("store_update", stream, table_dev, table_dtype, rows, d, ids_dev, e, values_dev,
                               values_dtype, m, row_index_dev, count);
}

int euler_gpu_store_add(void* stream, void* table_dev, int32_t table_dtype, int64_t rows, int64_t d,
                        const int64_t* ids_dev, int64_t e, const void* values_dev, int32_t values_dtype,
                        int64_t m, const int32_t* row_index_dev, int64_t count) {
  return StoreWrite<kEsAdd>("store_add", stream, table_dev, table_dtype, rows, d, ids_dev, e, values_dev,
                            values_dtype, m, row_index_dev, count);
}

int euler_gpu_store_take(void* stream, void* table_dev, int32_t table_dtype, int64_t rows, int64_t d,
                         const int64_t* ids_dev, int64_t e, int32_t clear, void* out_dev, int32_t out_dtype) {
  EsArgs a{};
  a.table = table_dev; a.rows = rows; a.d = d; a.ids = ids_dev; a.e = e;
  a.out = out_dev; a.clear = clear;
  bool run;
  const int rc = CheckStoreArgs("store_take", a, table_dtype, out_dev, out_dtype, &run);
  if (rc != EULER_GPU_OK || !run) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!clear) return DispatchTable<kEsTake>(st, a, table_dtype, out_dev, out_dtype);
  StreamBuf pairs(st);
  const int rg = GroupOccurrences(st, &a, &pairs);
  if (rg != EULER_GPU_OK) return rg;
  return DispatchTable<kEsTakeClear>(st, a, table_dtype, out_dev, out_dtype);
}

}  // extern "C"
