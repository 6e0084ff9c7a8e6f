// Fused sparse-row optimiser steps on gfx950 - sgd / momentum / adagrad / adam of sparse_optim.h,
// which states the contract - with their C-ABI entry point.
//
// A call is the three launches of an in-place store (embed_group.h): the (key, position) kernel,
// the stable radix sort of those pairs, and one kernel in which every segment of equal keys has
// ONE owner group of L lanes.  Per chunk of V columns the owner sums the gradient rows of its
// segment in position order - the loads of eight entries are issued together, the adds stay a
// chain -, then loads the chunk of the parameter row and of its state rows, applies the step and
// stores them: a distinct row costs one read and one write of p and of each state row, and no
// [distinct, d] temporary exists.  No lane of any other task reads or writes those rows.  Nothing
// here waits on the host, scratch comes from StreamBuf and goes back in stream order on every
// exit, and every check precedes the first write.
#include <cmath>

#include "embed_group.h"
#include "sparse_optim.h"

namespace euler_gpu {
namespace {

struct SoArgs {
  void* table; int64_t rows, d;
  float* state0; float* state1;
  const int64_t* ids; int64_t e;
  const void* grad; int64_t m; const int32_t* row_index; int64_t count;
  const uint64_t* keys; const uint32_t* perm;                                  // the sorted pairs
  SoScalars c;
  int32_t log_l;
};

// The task that sorted entry i starts, run by the L lanes of a group; l = the lane's number in
// its group.  DT: the table's dtype, DV: the gradient's.
template <int KIND, int DT, int DV, int V>
__device__ __forceinline__ void SoTask(const SoArgs& a, int64_t i, int32_t l, int32_t lanes, int32_t chunks) {
  const uint64_t key = a.keys[i];
  for (int32_t j = l; j < chunks; j += lanes) {
    const int64_t at = (int64_t)key * a.d + (int64_t)j * V;
    float g[V];
#pragma unroll
    for (int k = 0; k < V; ++k) g[k] = 0.f;
    // the adds stay in position order; only the loads of eight entries are issued together
    for (int64_t q = i;; q += 8) {
      bool ok[8];
      int64_t pos[8];
      uint32_t v[8][V];
      EsAhead<8>(a, key, i, q, ok, pos);
#pragma unroll
      for (int x = 0; x < 8; ++x)
        EsLoad<DV, V>(a.grad, EsSourceRow(pos[x], a.row_index, a.count) * a.d + (int64_t)j * V, v[x]);
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        const bool first = x == 0 && q == i;            // (the head: ok[0] holds there)
#pragma unroll
        for (int k = 0; k < V; ++k) g[k] = ok[x] ? SoGradStep<DV>(first, g[k], v[x][k]) : g[k];
      }
      if (!ok[7]) break;
    }
    uint32_t r[V], r0[V], r1[V];
    float p[V], s0[V], s1[V];
    EsLoad<DT, V>(a.table, at, r);
    if constexpr (KIND != kSoSgd) EsLoad<kF32, V>(a.state0, at, r0);
    if constexpr (KIND == kSoAdam) EsLoad<kF32, V>(a.state1, at, r1);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      p[k] = EsWiden<DT>(r[k]);
      s0[k] = KIND != kSoSgd ? BitsF32(r0[k]) : 0.f;
      s1[k] = KIND == kSoAdam ? BitsF32(r1[k]) : 0.f;
      SoStep<KIND>(a.c, g[k], &p[k], &s0[k], &s1[k]);
      r[k] = EsNarrow<DT>(p[k]);
      r0[k] = F32Bits(s0[k]);
      r1[k] = F32Bits(s1[k]);
    }
    EsStore<DT, V>(a.table, at, r);
    if constexpr (KIND != kSoSgd) EsStore<kF32, V>(a.state0, at, r0);
    if constexpr (KIND == kSoAdam) EsStore<kF32, V>(a.state1, at, r1);
  }
}

// The grid-stride loop and the ballot-based task hand-out of EsStoreKernel: a wave looks at 64
// adjacent sorted entries, the live heads among them go round robin to its 64 / L groups.
template <int KIND, int DT, int DV, int V>
__global__ __launch_bounds__(256) void SoStepKernel(const SoArgs a) {
  const int32_t lanes = 1 << a.log_l, groups = 64 >> a.log_l;
  const int32_t lane = threadIdx.x & 63;
  const int32_t g = lane >> a.log_l, l = lane & (lanes - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int32_t chunks = (int32_t)(a.d / V);
  for (int64_t base = wave * 64; base < a.e; base += waves * 64) {       // (the same trips for a whole wave)
    const int64_t i = base + lane;
    const bool task = i < a.e && a.keys[i] < (uint64_t)a.rows && EsIsHead(a.keys, i);
    uint64_t todo = __ballot(task);
    // group g takes the tasks g, g + groups, ... of the window
    for (int32_t x = 0; x < g && todo; ++x) todo &= todo - 1;
    while (todo) {
      SoTask<KIND, DT, DV, V>(a, base + __builtin_ctzll(todo), l, lanes, chunks);
      for (int32_t x = 0; x < groups && todo; ++x) todo &= todo - 1;
    }
  }
}

template <int KIND, int DT, int DV>
int LaunchStep(hipStream_t st, SoArgs a) {
  const int32_t v = SoChunkWidth(a.d, (uintptr_t)a.table, kBytes[DT], (uintptr_t)a.grad, kBytes[DV],
                                 (uintptr_t)a.state0, (uintptr_t)a.state1);
  a.log_l = EsLogLanes(a.d / v);
  const int64_t waves = (a.e + 63) / 64;
  int64_t blocks = (waves + 3) / 4;
  if (blocks > 256 * 32) blocks = 256 * 32;
  const dim3 grid((unsigned)blocks), block(256);
  if (v == 8) hipLaunchKernelGGL((SoStepKernel<KIND, DT, DV, 8>), grid, block, 0, st, a);
  else if (v == 4) hipLaunchKernelGGL((SoStepKernel<KIND, DT, DV, 4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((SoStepKernel<KIND, DT, DV, 1>), grid, block, 0, st, a);
  EG_HIP(hipGetLastError());
  return EULER_GPU_OK;
}

template <int KIND, int DT>
int DispatchGrad(hipStream_t st, const SoArgs& a, int32_t grad_dtype) {
  if (grad_dtype == EULER_GPU_F32) return LaunchStep<KIND, DT, kF32>(st, a);
  return LaunchStep<KIND, DT, DT>(st, a);
}

template <int KIND>
int DispatchTable(hipStream_t st, const SoArgs& a, int32_t table_dtype, int32_t grad_dtype) {
  if (table_dtype == EULER_GPU_F32) return LaunchStep<KIND, kF32, kF32>(st, a);
  if (table_dtype == EULER_GPU_BF16) return DispatchGrad<KIND, kBF16>(st, a, grad_dtype);
  return DispatchGrad<KIND, kF16>(st, a, grad_dtype);
}

bool SoScalarOk(float x) { return std::isfinite(x) && x >= 0.f; }

}  // namespace
}  // namespace euler_gpu

using namespace euler_gpu;

extern "C" int euler_gpu_sparse_optim_step(void* stream, int32_t kind, void* table_dev, int32_t table_dtype,
                                           int64_t rows, int64_t d, float* state0_dev, float* state1_dev,
                                           const int64_t* ids_dev, int64_t e, const void* grad_dev,
                                           int32_t grad_dtype, int64_t m, const int32_t* row_index_dev,
                                           int64_t count, float lr, float mu, float eps, float om1, float om2,
                                           float step_size) {
  const std::string what("sparse_optim_step");
  if (kind < kSoSgd || kind > kSoAdam)
    return Fail(EULER_GPU_EINVAL, what + ": unknown kind (0 sgd, 1 momentum, 2 adagrad, 3 adam)");
  if (!KnownDtype(table_dtype) || !KnownDtype(grad_dtype))
    return Fail(EULER_GPU_EINVAL, what + ": unknown dtype" + kDtypeCodes);
  if (grad_dtype != EULER_GPU_F32 && grad_dtype != table_dtype)
    return Fail(EULER_GPU_EINVAL, what + ": grad is fp32 or of the table's dtype");
  if (!SoScalarOk(lr) || !SoScalarOk(mu) || !SoScalarOk(eps) || !SoScalarOk(om1) || !SoScalarOk(om2) ||
      !SoScalarOk(step_size))
    return Fail(EULER_GPU_EINVAL, what + ": a scalar is negative or not finite");
  const int32_t n_state = SoStateCount(kind);
  if ((n_state >= 1) != (state0_dev != nullptr) || (n_state == 2) != (state1_dev != nullptr))
    return Fail(EULER_GPU_EINVAL, what + ": the state buffers do not match the kind (sgd none, momentum and "
                                         "adagrad one, adam two)");
  if (rows < 1) return Fail(EULER_GPU_EINVAL, what + ": a table with fewer than 1 row");
  if (e < 0 || d < 0) return Fail(EULER_GPU_EINVAL, what + ": e or d < 0");
  if (e >= (1LL << 31) || d >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, what + ": e or d >= 2^31");
  if (row_index_dev && count != 0) return Fail(EULER_GPU_EINVAL, what + ": row_index and count both given");
  if (count < 0) return Fail(EULER_GPU_EINVAL, what + ": count < 0");
  if (m < 0) return Fail(EULER_GPU_EINVAL, what + ": m < 0");
  if (count > 0 && (e % count != 0 || m != e / count))
    return Fail(EULER_GPU_EINVAL, what + ": count needs e % count == 0 and m == e / count");
  if (!row_index_dev && count == 0 && m != e) return Fail(EULER_GPU_EINVAL, what + ": grad is [e, d]: m != e");
  if ((uintptr_t)row_index_dev % 4 != 0 || (uintptr_t)state0_dev % 4 != 0 || (uintptr_t)state1_dev % 4 != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  if (e == 0 || d == 0) return EULER_GPU_OK;
  if (row_index_dev && m == 0) return EULER_GPU_OK;  // no source row: every occurrence is removed
  if (!table_dev || !ids_dev || !grad_dev) return Fail(EULER_GPU_EINVAL, what + ": null buffer");
  if ((uintptr_t)table_dev % kBytes[table_dtype] != 0 || (uintptr_t)grad_dev % kBytes[grad_dtype] != 0 ||
      (uintptr_t)ids_dev % 8 != 0)
    return Fail(EULER_GPU_EINVAL, what + ": a buffer is not aligned to its type");
  SoArgs a{};
  a.table = table_dev; a.rows = rows; a.d = d; a.state0 = state0_dev; a.state1 = state1_dev;
  a.ids = ids_dev; a.e = e; a.grad = grad_dev; a.m = m; a.row_index = row_index_dev; a.count = count;
  a.c = SoScalars{lr, mu, eps, om1, om2, step_size};
  hipStream_t st = (hipStream_t)stream;
  StreamBuf pairs(st);
  const int rg = GroupOccurrences(st, &a, &pairs);
  if (rg != EULER_GPU_OK) return rg;
  switch (kind) {
    case kSoSgd: return DispatchTable<kSoSgd>(st, a, table_dtype, grad_dtype);
    case kSoMomentum: return DispatchTable<kSoMomentum>(st, a, table_dtype, grad_dtype);
    case kSoAdagrad: return DispatchTable<kSoAdagrad>(st, a, table_dtype, grad_dtype);
    default: return DispatchTable<kSoAdam>(st, a, table_dtype, grad_dtype);
  }
}
