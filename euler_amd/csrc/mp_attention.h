// Fused segment attention (attention_aggregate): the arithmetic of ONE destination - a logit per
// (update, head), the softmax of mp_softmax.h over the destination's updates, and the sum of the
// source rows weighted by it (gat_conv.py:66-72, agnn_conv.py:36-54, attention_pool.py:36-40,
// set2set_pool.py:45-49) - shared by segment_attention_kernels.hip and by
// tests/csrc/segment_attention_check.cc, which compiles this file with the host compiler.  Every
// operation is a correctly rounded fp32 add, multiply or divide (MpwAdd / MpwMul / MpwDiv), an
// integer operation or a comparison: no FMA, no library exp.
//
// THE LOGIT of update p and head h, destination r (qr = q_index[r] or r, g = the gathered row):
//   dot:       fl(scale * DOT_c q[qr][h dh + c] * k[g][h dh + c])
//   additive:  a = fl(q[qr][h] + k[g][h]);  a < 0 ? fl(a * slope) : a          (q absent: q = +0)
// ORDER OF DOT (a function of dh alone - never of E, size, the grid, the storage type, the
// segment form or pointer alignment).  The dh columns are cut into chunks of V adjacent ones,
// V = 4 when dh % 4 == 0, else 1 (AttChunk); L = min(64, the power of two >= dh / V) partial sums
// (AttLanes).  Partial l takes the chunks l, l + L, l + 2 L, ... and adds their products one by one
// in increasing column order, starting from +0 (AttChunkDot); a partial without a chunk is +0.
// The L partials are combined by a butterfly: for off = L / 2, L / 4, ..., 1:  s_l = s_l + s_(l ^ off)
// (every s_l ends with the same bits: the addition commutes).  dh = 1: fl(+0 + q k).
// The same DOT, over the dv columns of a head of v, gives the backward's da = DOT_c G[r] * v[g].
//
// THE SOFTMAX is mp_softmax.h unchanged (SmxShortForward for 1..32 updates, the SmxLane* partials
// and SmxCombine4 beyond): alpha is what edge_softmax returns for these logits.
//
// THE SUM is the ordered fold of WeightedReduceRow: acc = +0, then acc = fl(acc + fl(x * alpha))
// in increasing p (AttFold): out is what gather_segment_reduce("add", v, g, size,
// edge_weight=alpha) returns.
//
// BACKWARD at the destination, given the saved alpha and the incoming G [size, Dv]:
//   da = DOT (above, over dv),  dl = SmxBackward(alpha, da)  (mp_softmax.h),
//   dot:       ds = fl(scale * dl),  dq_dst[r] = the AttFold of k[g] with ds;
//   additive:  ds = a < 0 ? fl(dl * slope) : dl  (a as above),  dq_dst[r][h] = +0 + ds_0 + ds_1 + ...
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "mp_softmax.h"
#include "mp_weighted.h"

namespace euler_gpu {

constexpr int32_t kAttDot = 0, kAttAdditive = 1;

EG_MPW_HD int32_t AttChunk(int64_t dh) { return dh % 4 == 0 ? 4 : 1; }

EG_MPW_HD int32_t AttLanes(int64_t dh) {
  const int64_t chunks = dh / AttChunk(dh);
  int32_t l = 1;
  while (l < 64 && l < chunks) l <<= 1;
  return l;
}

// the products of one chunk, added to the partial s in increasing column order
template <int V>
EG_MPW_HD float AttChunkDot(const float a[V], const float b[V], float s) {
EG_MPW_UNROLL
  for (int c = 0; c < V; ++c) s = MpwAdd(s, MpwMul(a[c], b[c]));
  return s;
}

EG_MPW_HD float AttDotLogit(float dot, float scale) { return MpwMul(scale, dot); }

EG_MPW_HD float AttAdditiveLogit(float q, float k, float slope) {
  const float a = MpwAdd(q, k);
  return a < 0.f ? MpwMul(a, slope) : a;
}

// additive: the gradient through the leaky relu, on the pre-activation a = fl(q + k)
EG_MPW_HD float AttAdditiveGrad(float dl, float q, float k, float slope) {
  return MpwAdd(q, k) < 0.f ? MpwMul(dl, slope) : dl;
}

EG_MPW_HD float AttFold(float acc, float x, float w) { return MpwAdd(acc, MpwMul(x, w)); }

}  // namespace euler_gpu
