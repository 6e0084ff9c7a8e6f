// GCN-normalised aggregation: the symmetric degree normalisation norm_i * norm_j of GCNConv,
// APPNPConv, SGCNConv, TAGConv, ARMAConv and DNAConv (gcn_conv.py:33-51, appnp_conv.py:34-60,
// arma_conv.py:46-78, dna_conv.py:106-170) folded into the weighted reduce of mp_weighted.h.
// Shared by gcn_norm_kernels.hip and by tests/csrc/mp_gcn_check.cc, which compiles it with the
// host compiler.
//
// norm = 1 / sqrt((float)deg): the conversion is exact below 2^24, the square root and the divide
// are two correctly rounded fp32 operations - the bits of numpy's float32(1) / sqrt(float32(deg)).
// deg == 0 gives exactly 0: the reference's deg ** -0.5 is inf there, but such a node has no
// counted edge, so the value is never multiplied into anything, and 0 keeps the tables finite.
//
// Destination r reduces, in input order, fl(x[g(p)][c] * fl(norm_dst[r] * norm_src[g(p)])) over
// the updates p of its segment: the weight is the rounded product of the two table entries, the
// message the rounded product of the row with it, the sum a rounded add - three roundings, in the
// order the composition norm_i * norm_j * x_j forms them, so the bits are those of the weighted
// reduce over the edge weights norm_dst[dst] * norm_src[src].  The arithmetic of a destination is
// WeightedReduceRow itself; GcnNormOps only supplies the weight.
//
// An update whose gather index lies outside [0, rows) contributes nothing: its weight is 0 and
// its row is clamped to the last one.  For a finite table the product is then +-0, and adding
// +-0 to an accumulator that started at +0 leaves every bit alone (x + (+-0) = x, and +0 + -0 =
// +0 under round-to-nearest), so the result has the bits of a reduce without that update; a
// table with inf or NaN in its last row is outside that promise.  The backward pass relies on it:
// it gathers by destination key, and a key outside the block needs no appended zero row.
//
// The optional epilogue adds the destination's own row: fl(fl(agg * a) + fl(root * b)), three
// fp32 roundings before the one rounding of the store - APPNP's (1 - alpha, alpha)
// (appnp_conv.py:57-60), ARMA's (1, 1) (arma_conv.py:72-75), where both products are exact.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <math.h>
#include <stdint.h>

#include "mp_weighted.h"

namespace euler_gpu {

EG_MPW_HD float GcnNormOf(int32_t deg) {
  if (deg <= 0) return 0.f;
  // sqrtf, not __fsqrt_rn: on gfx950 the latter is the bare v_sqrt_f32 (1 ulp), the former the
  // corrected sequence; tests/test_gcn_norm_gpu.py holds this in place
  return MpwDiv(1.0f, sqrtf((float)deg));
}

// Ops of WeightedReduceRow over a Loader {Raw, Load(row), Widen(raw, f)}: the weight of update
// pos is fl(nd * norm_src[g]) for its gather index g, nd = norm_dst[r] of the destination (a
// register); g outside [0, rows): weight 0 (MpwIndex::Row clamps the row: ix.row_max = rows - 1).
template <typename Loader>
struct GcnNormOps {
  using Raw = typename Loader::Raw;
  Loader ld;
  MpwIndex ix;
  const float* norm_src;
  uint32_t rows;
  float nd;
  EG_MPW_HD int64_t Pos(int64_t p) const { return ix.Pos(p); }
  EG_MPW_HD int64_t Row(int64_t pos) const { return ix.Row(pos); }
  EG_MPW_HD float Weight(int64_t pos) const {
    const uint32_t g = (uint32_t)ix.gsrc[pos];
    return g < rows ? MpwMul(nd, norm_src[g]) : 0.f;
  }
  EG_MPW_HD Raw Load(int64_t row) const { return ld.Load(row); }
  EG_MPW_HD void Widen(const Raw& v, float* f) const { ld.Widen(v, f); }
};

// acc[k] = fl(fl(acc[k] * a) + fl(root[k] * b))
template <int N>
EG_MPW_HD void GcnRootEpilogue(float acc[N], const float root[N], float a, float b) {
  for (int k = 0; k < N; ++k) acc[k] = MpwAdd(MpwMul(acc[k], a), MpwMul(root[k], b));
}

}  // namespace euler_gpu
