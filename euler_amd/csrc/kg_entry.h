// The host front of the triple-scoring entries (kg_score_kernels.hip, kg_proj_kernels.hip,
// kg_matrix_kernels.hip): the kernel arguments the three families share, the one argument ladder
// in front of their six entries, the dtype fan-out and the launch shape of a task of L lanes.
// Host code only.  What a family adds - its own fields, its entries' tails, its kernels - stays
// in its file.
#pragma once

#include <stdint.h>

#include <string>
#include <type_traits>

#include "common.h"
#include "half_cvt.h"
#include "kg_matrix.h"
#include "kg_proj.h"
#include "kg_score.h"

namespace euler_gpu {

// What every family's kernels take; KgArgs, KgProjArgs and KgmArgs are this plus their own fields.
struct KgTripleArgs {
  int32_t kind, corrupt, log_l;
  const void* ent; int64_t ent_rows;
  const void* rel; int64_t rel_rows;
  const int64_t* src; const int64_t* rel_id; const int64_t* dst; const int64_t* neg;
  int64_t b, k;
  float* pos_out; float* neg_out;                 // forward
  const float* g_pos; const float* g_neg;         // gradient
  float* g_src; float* g_rel; float* g_dst; float* g_neg_rows;
  int32_t out_vec;                                // the lane-written gradient buffers start on 16 bytes
};

// The shared part from an entry's parameters: a forward entry passes its two outputs, a gradient
// entry null for them and its six gradient buffers.
inline KgTripleArgs KgShared(int32_t kind, int32_t corrupt, const void* ent, int64_t ent_rows, const void* rel,
                             int64_t rel_rows, const int64_t* src, const int64_t* rel_id, const int64_t* dst,
                             const int64_t* neg, int64_t b, int64_t k, float* pos_out, float* neg_out,
                             const float* g_pos = nullptr, const float* g_neg = nullptr, float* g_src = nullptr,
                             float* g_rel = nullptr, float* g_dst = nullptr, float* g_neg_rows = nullptr) {
  return KgTripleArgs{kind, corrupt, /*log_l=*/0, ent, ent_rows, rel, rel_rows, src, rel_id, dst, neg, b, k,
                      pos_out, neg_out, g_pos, g_neg, g_src, g_rel, g_dst, g_neg_rows, /*out_vec=*/0};
}

inline bool KgAligned(const void* p, int32_t dtype) { return (uintptr_t)p % (dtype == EULER_GPU_F32 ? 4 : 2) == 0; }

// What a family adds to the ladder.  score: d.  proj: d, proj and its two aux tables.  matrix:
// d = de, dr, the matrix with its dtype, and `order`.
enum KgFamily { kKgScoreFamily, kKgProjFamily, kKgMatrixFamily };
struct KgCall {
  const char* what;                               // the entry's name in the messages
  KgFamily family;
  int32_t ent_dtype, rel_dtype;
  int64_t d;
  int32_t proj = 0;
  const void* ent_aux = nullptr; const void* rel_aux = nullptr;
  int64_t dr = 0;
  const void* matrix = nullptr; int32_t matrix_dtype = EULER_GPU_F32;
  const void* order = nullptr;
};

// The checks all six entries share, in one order.  -> EULER_GPU_OK with *run = false when there
// is nothing to do.  An entry's own buffers (outputs, gradients, segments) are its tail's.
inline int CheckKgCall(const KgCall& c, const KgTripleArgs& a, bool* run) {
  *run = false;
  const std::string w(c.what);
  const bool proj = c.family == kKgProjFamily, matrix = c.family == kKgMatrixFamily;
  if (proj && (c.proj < 1 || c.proj > 2)) return Fail(EULER_GPU_EINVAL, w + ": proj outside 1..2 (1 hyperplane, 2 transfer)");
  if (c.family == kKgScoreFamily) {
    if (a.kind < 0 || a.kind > 2) return Fail(EULER_GPU_EINVAL, w + ": kind outside 0..2");
  } else if (a.kind < 0 || a.kind > 1) {
    return Fail(EULER_GPU_EINVAL, w + ": kind outside 0..1 (distmult takes no projection)");
  }
  if (a.corrupt < 0 || a.corrupt > 2) return Fail(EULER_GPU_EINVAL, w + ": corrupt outside 0..2");
  if (!KnownDtype(c.ent_dtype) || !KnownDtype(c.rel_dtype) || !KnownDtype(c.matrix_dtype))
    return Fail(EULER_GPU_EINVAL, w + ": unknown dtype" + kDtypeCodes);
  if (a.k < 0 || a.b < 0 || c.d < 0 || c.dr < 0)
    return Fail(EULER_GPU_EINVAL, w + (matrix ? ": b, k, de or dr < 0" : ": b, k or d < 0"));
  if (a.ent_rows < 1 || a.rel_rows < 1) return Fail(EULER_GPU_EINVAL, w + ": a table with fewer than 1 row");
  if (matrix) {
    if (c.d > kKgMatrixMaxDim || c.dr > kKgMatrixMaxDim) return Fail(EULER_GPU_EINVAL, w + ": de or dr above 512");
    if (a.ent_rows >= (1LL << 31)) return Fail(EULER_GPU_EINVAL, w + ": ent_rows >= 2^31");
  } else if (c.d >= (1LL << 31)) {
    return Fail(EULER_GPU_EINVAL, w + ": d >= 2^31");
  }
  if (a.b >= (1LL << 31) || a.k >= (1LL << 31) || a.b * (a.k > 1 ? a.k : 1) * 2 >= (1LL << 31))
    return Fail(EULER_GPU_EINVAL, w + ": b * max(k, 1) * 2 >= 2^31");
  if (proj && c.proj == kKgProjHyper && c.ent_aux) return Fail(EULER_GPU_EINVAL, w + ": proj 1 takes no ent_aux table");
  if (a.b == 0 || c.d == 0 || (matrix && c.dr == 0)) return EULER_GPU_OK;
  if (!a.ent || !a.rel || !a.src || !a.rel_id || !a.dst || (matrix && (!c.matrix || !c.order)))
    return Fail(EULER_GPU_EINVAL, w + ": null buffer");
  if (proj && (!c.rel_aux || (c.proj == kKgProjTransfer && !c.ent_aux)))
    return Fail(EULER_GPU_EINVAL, w + ": a missing aux table (proj 1: hyper; proj 2: ent_transfer and rel_transfer)");
  if (a.k > 0 && !a.neg) return Fail(EULER_GPU_EINVAL, w + ": k > 0 without negatives");
  if (!KgAligned(a.ent, c.ent_dtype) || !KgAligned(c.ent_aux, c.ent_dtype) || !KgAligned(a.rel, c.rel_dtype) ||
      !KgAligned(c.rel_aux, c.rel_dtype) || !KgAligned(c.matrix, c.matrix_dtype))
    return Fail(EULER_GPU_EINVAL, w + ": a table is not aligned to its type");
  *run = true;
  return EULER_GPU_OK;
}

// A run-time dtype code as a compile-time constant: f(std::integral_constant<int, kF32>) ...
template <typename F>
int KgWithDtype(int32_t dtype, F&& f) {
  if (dtype == EULER_GPU_F32) return f(std::integral_constant<int, kF32>{});
  if (dtype == EULER_GPU_BF16) return f(std::integral_constant<int, kBF16>{});
  return f(std::integral_constant<int, kF16>{});
}

// f(DE, DR) for the dtypes of the entity and the relation tables
template <typename F>
int KgDispatchTables(int32_t ent_dtype, int32_t rel_dtype, F&& f) {
  return KgWithDtype(ent_dtype, [&](auto de) { return KgWithDtype(rel_dtype, [&](auto dr) { return f(de, dr); }); });
}

// The launch of b tasks of L lanes, 64 / L tasks a wave and four waves a workgroup.  reg: a lane
// owns at most one chunk.
struct KgLaunchShape {
  int32_t log_l;
  bool reg;
  unsigned grid;
};
inline KgLaunchShape KgTaskLaunch(int64_t b, int64_t chunks) {
  const int32_t log_l = KgLogLanes(chunks);
  const int64_t tasks_per_wave = 64 >> log_l;
  const int64_t waves = (b + tasks_per_wave - 1) / tasks_per_wave;
  int64_t blocks = (waves + 3) / 4;
  if (blocks > 256 * 32) blocks = 256 * 32;
  return KgLaunchShape{log_l, chunks <= 64, (unsigned)blocks};
}

}  // namespace euler_gpu
