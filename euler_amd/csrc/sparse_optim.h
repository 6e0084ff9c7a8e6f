// Fused sparse-row optimiser steps - sgd, momentum, adagrad, adam: the four optimisers the
// reference offers every model (tf_euler/python/utils/optimizers.py), applied to the rows of an
// embedding table that a list of ids names, from the gradient rows of the OCCURRENCES of those ids.
// THE CONTRACT is stated here once; the pieces below are shared by the kernel of
// sparse_optim_kernels.hip and by tests/csrc/sparse_optim_check.cc, which compiles this file with
// the host compiler.
//
// table  [rows, d], contiguous, fp32 / bf16 / fp16, rows >= 1; MODIFIED IN PLACE.
// state  zero, one or two [rows, d] fp32 contiguous buffers, MODIFIED IN PLACE:
//        sgd: none; momentum: accum; adagrad: sum; adam: exp_avg and exp_avg_sq.
// ids    signed int64 [e]; RANGE RULE of embed_store.h: an id outside [0, rows) names no row and
//        is left out.
// grad   the gradient row of occurrence p is grad[p], grad[row_index[p]] (int32 [e], grad [m, d];
//        an entry outside [0, m) removes the occurrence) or grad[p / count] - the three source
//        forms of embed_store.h (EsSourceRow / EsSourceLive).  grad is fp32 or the table's dtype.
//
// For every distinct live id r and every column, each fl() ONE correctly rounded fp32 operation
// (device: the __f*_rn forms, the IEEE sqrt and divide; host: plain operators and sqrtf in a
// translation unit built with -ffp-contract=off):
//   g  = widen(element of the FIRST occurrence of r); then for its later occurrences in
//        increasing position: g = fl(g + widen(x)).
//   p  = widen(table[r]); afterwards table[r] = narrow(p'), one rounding.
//   sgd       p' = fl(p - fl(lr * g))
//   momentum  a' = fl(fl(mu * a) + g);  p' = fl(p - fl(lr * a'))
//             (TensorFlow's SparseApplyMomentum: touched rows only, no Nesterov)
//   adagrad   s' = fl(s + fl(g * g));  p' = fl(p - fl(lr * fl(g / fl(fl(sqrt(s')) + eps))))
//             (torch's sparse branch; eps = 0 gives TensorFlow's)
//   adam      m' = fl(m + fl(fl(g - m) * om1))
//             v' = fl(v + fl(fl(fl(g * g) - v) * om2))
//             p' = fl(p - fl(step_size * fl(m' / fl(fl(sqrt(v')) + eps))))
//             (lazy: the formula of torch.optim.SparseAdam)
// SCALARS: lr, mu, eps, om1 = 1 - beta1, om2 = 1 - beta2 and step_size = lr * sqrt(1 - beta2^t) /
// (1 - beta1^t) are computed on the host in double, rounded once to fp32 and passed by value: the
// kernel reads no scalar from device memory and the step count t lives on the host.
// Rows named by no live id keep their bits, in the table and in every state buffer.  e == 0 or
// d == 0: nothing is touched.
//
// HOW: the grouping of embed_store.h - a STABLE sort of (key, position), one owner (L lanes of a
// wave) per segment of equal keys, chunks of V = 8 / 4 / 1 adjacent columns by d % V and the
// alignment of EVERY buffer the call touches, the state included.  There is NO sum across columns
// here: every column is a chain of its own, so V, L and the launch geometry cannot change any bit.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <math.h>
#include <stdint.h>

#include "embed_store.h"

namespace euler_gpu {

constexpr int kSoSgd = 0, kSoMomentum = 1, kSoAdagrad = 2, kSoAdam = 3;

// The number of state buffers of a kind
inline int32_t SoStateCount(int32_t kind) { return kind == kSoSgd ? 0 : kind == kSoAdam ? 2 : 1; }

// The scalars of a call, each one fp32 value the host rounded once from its double
struct SoScalars {
  float lr, mu, eps, om1, om2, step_size;
};

EG_MPW_HD float SoSub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fsub_rn(a, b);
#else
  return a - b;
#endif
}

EG_MPW_HD float SoSqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_sqrtf(x);        // the correctly rounded expansion (never the native form)
#else
  return sqrtf(x);
#endif
}

// The gradient chain: the first occurrence starts it, every later one is EsAddStep
template <int DV>
EG_MPW_HD float SoGradStep(bool first, float g, uint32_t raw) {
  return first ? EsWiden<DV>(raw) : EsAddStep<DV>(g, raw);
}

// One element: the summed gradient g, the parameter *p and its state *s0 / *s1 (those the kind
// has), all fp32; the new values are left in place.
template <int KIND>
EG_MPW_HD void SoStep(const SoScalars& c, float g, float* p, float* s0, float* s1) {
  if constexpr (KIND == kSoSgd) {
    *p = SoSub(*p, MpwMul(c.lr, g));
  } else if constexpr (KIND == kSoMomentum) {
    *s0 = MpwAdd(MpwMul(c.mu, *s0), g);
    *p = SoSub(*p, MpwMul(c.lr, *s0));
  } else if constexpr (KIND == kSoAdagrad) {
    *s0 = MpwAdd(*s0, MpwMul(g, g));
    *p = SoSub(*p, MpwMul(c.lr, MpwDiv(g, MpwAdd(SoSqrt(*s0), c.eps))));
  } else {
    *s0 = MpwAdd(*s0, MpwMul(SoSub(g, *s0), c.om1));
    *s1 = MpwAdd(*s1, MpwMul(SoSub(MpwMul(g, g), *s1), c.om2));
    *p = SoSub(*p, MpwMul(c.step_size, MpwDiv(*s0, MpwAdd(SoSqrt(*s1), c.eps))));
  }
}

// V, given d and every buffer of the call (a state pointer that the kind does not have: 0)
inline int32_t SoChunkWidth(int64_t d, uintptr_t table, int table_bytes, uintptr_t grad, int grad_bytes,
                            uintptr_t state0, uintptr_t state1) {
  const int32_t a = EsChunkWidth(d, table, table_bytes, grad, grad_bytes);
  const int32_t b = EsChunkWidth(d, state0, 4, state1, 4);
  return a < b ? a : b;
}

}  // namespace euler_gpu
