// Host build of the shared pieces of the fused sparse-row optimiser steps
// (euler_amd/csrc/sparse_optim.h) for tests/test_sparse_optim_host.py: the keys and the range
// rule, the occurrence-to-source-row mapping, head selection over the stably sorted
// (key, position) array, the gradient chain, the four steps and the single rounding - driven over
// whole calls on plain host arrays, one column at a time.  Built with -ffp-contract=off.
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "sparse_optim.h"

using namespace euler_gpu;

namespace {

struct Call {
  void* table; int64_t rows, d;
  float* state0; float* state1;
  const int64_t* ids; int64_t e;
  const void* grad; int64_t m; const int32_t* row_index; int64_t count;
  SoScalars c;
};

template <int DT>
uint32_t Get(const void* base, int64_t at) {
  if (DT == kF32) return static_cast<const uint32_t*>(base)[at];
  return static_cast<const uint16_t*>(base)[at];
}
template <int DT>
void Put(void* base, int64_t at, uint32_t raw) {
  if (DT == kF32) static_cast<uint32_t*>(base)[at] = raw;
  else static_cast<uint16_t*>(base)[at] = (uint16_t)raw;
}

template <int KIND, int DT, int DV>
void Run(const Call& c) {
  // the stable sort of (key, position): what the radix sort of the device leaves
  std::vector<uint64_t> k((size_t)c.e), keys((size_t)c.e);
  for (int64_t p = 0; p < c.e; ++p) k[p] = EsKey(c.ids[p], c.rows, EsSourceLive(p, c.row_index, c.m));
  std::vector<uint32_t> perm((size_t)c.e);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
  for (int64_t i = 0; i < c.e; ++i) keys[i] = k[perm[i]];
  for (int64_t i = 0; i < c.e; ++i) {
    if (keys[i] >= (uint64_t)c.rows || !EsIsHead(keys.data(), i)) continue;
    for (int64_t col = 0; col < c.d; ++col) {
      const int64_t at = (int64_t)keys[i] * c.d + col;
      float g = 0.f;
      for (int64_t q = i; q < c.e && keys[q] == keys[i]; ++q)
        g = SoGradStep<DV>(q == i, g, Get<DV>(c.grad, EsSourceRow(perm[q], c.row_index, c.count) * c.d + col));
      float p = EsWiden<DT>(Get<DT>(c.table, at));
      float s0 = KIND != kSoSgd ? c.state0[at] : 0.f, s1 = KIND == kSoAdam ? c.state1[at] : 0.f;
      SoStep<KIND>(c.c, g, &p, &s0, &s1);
      Put<DT>(c.table, at, EsNarrow<DT>(p));
      if (KIND != kSoSgd) c.state0[at] = s0;
      if (KIND == kSoAdam) c.state1[at] = s1;
    }
  }
}

template <int KIND, int DT>
void RunGrad(const Call& c, int32_t grad_dt) {
  if (grad_dt == kF32) Run<KIND, DT, kF32>(c);
  else Run<KIND, DT, DT>(c);
}

template <int KIND>
void RunTable(const Call& c, int32_t table_dt, int32_t grad_dt) {
  if (table_dt == kF32) Run<KIND, kF32, kF32>(c);
  else if (table_dt == kBF16) RunGrad<KIND, kBF16>(c, grad_dt);
  else RunGrad<KIND, kF16>(c, grad_dt);
}

}  // namespace

extern "C" int so_state_count(int32_t kind) { return SoStateCount(kind); }

extern "C" int so_chunk_width(int64_t d, uint64_t table, int table_bytes, uint64_t grad, int grad_bytes,
                              uint64_t state0, uint64_t state1) {
  return SoChunkWidth(d, (uintptr_t)table, table_bytes, (uintptr_t)grad, grad_bytes, (uintptr_t)state0,
                      (uintptr_t)state1);
}

// One whole call on host arrays; the arguments of euler_gpu_sparse_optim_step without the stream.
// dtype codes 0 fp32, 1 bf16, 2 fp16 (16-bit data: uint16).
extern "C" int so_call(int32_t kind, void* table, int32_t table_dt, int64_t rows, int64_t d, float* state0,
                       float* state1, const int64_t* ids, int64_t e, const void* grad, int32_t grad_dt, int64_t m,
                       const int32_t* row_index, int64_t count, float lr, float mu, float eps, float om1, float om2,
                       float step_size) {
  if (kind < 0 || kind > 3 || table_dt < 0 || table_dt > 2 || (grad_dt != kF32 && grad_dt != table_dt)) return -1;
  if (rows < 1 || e < 0 || d < 0 || (row_index && count != 0) || count < 0) return -1;
  if (count > 0 && (e % count != 0 || m != e / count)) return -1;
  if (!row_index && count == 0 && m != e) return -1;
  if ((SoStateCount(kind) >= 1) != (state0 != nullptr) || (SoStateCount(kind) == 2) != (state1 != nullptr)) return -1;
  Call c{table, rows, d, state0, state1, ids, e, grad, m, row_index, count, SoScalars{lr, mu, eps, om1, om2, step_size}};
  if (kind == kSoSgd) RunTable<kSoSgd>(c, table_dt, grad_dt);
  else if (kind == kSoMomentum) RunTable<kSoMomentum>(c, table_dt, grad_dt);
  else if (kind == kSoAdagrad) RunTable<kSoAdagrad>(c, table_dt, grad_dt);
  else RunTable<kSoAdam>(c, table_dt, grad_dt);
  return 0;
}
