// The supervised loss head (GraphSAGE, GCN, GAT, ... and the graph classifiers of the reference:
// SuperviseModel.__call__ of tf_euler/python/mp_utils/base.py:24-47 after out_fc, SuperviseSolution
// of solution/base_supervise.py, GraphModel of mp_utils/base_graph.py:24-47, with f1_score /
// acc_score / auc_score of utils/metrics.py:29-48): the arithmetic of ONE ELEMENT (b, c) of the
// [B, C] block of logits, shared by the kernels of supervise_kernels.hip and by
// tests/csrc/supervise_check.cc, which compiles this file with the host compiler.  Every operation
// is a correctly rounded fp32 multiply, add or divide (MpwMul / MpwAdd / MpwDiv), one IEEE float64
// division rounded once to fp32 (the threshold table), a comparison or an integer operation: host
// and device return the same bits by construction.
//
// INPUTS.  Logits x [B, C]: fp32, bf16 or fp16, widened exactly.  Labels z: a tensor [B, C] (fp32,
// bf16 or fp16, widened exactly), or the GRAPH FORM: node ids [B] and a float feature slot fid of
// the graph, read straight from the graph's feature table with the semantics of
// euler_gpu_get_dense_feature_t - an unknown node or slot reads as zeros, a slot shorter than C is
// zero filled, a longer one is truncated, a 16-bit table is widened.  No [B, C] label block
// exists in the graph form.
//
// PROBABILITY.  p = SgSigmoid(x) (skipgram.h).
// LOSS TERM (tf.nn.sigmoid_cross_entropy_with_logits, soft labels allowed):
//   term = (SgRelu(x) - x * z) + Log1pUnit(SgExp(x))
//   - one multiply and two adds, each correctly rounded, in that order (SvTermGeneral).
//   HARD LABELS.  For z == 0 the product is a zero and SgRelu(x) - (+-0) is SgRelu(x); for z == 1
//   SgRelu(x) - x is exactly SgRelu(-x) (x > 0: x - x = +0; x <= 0: +0 - x = -x, and +0 - (+-0) =
//   +0).  So for z in {0, 1} and every finite x the term has the bits of SgTerm(x, z == 1), and
//   SvTerm takes those two identities as written: the same bits for finite x, and at x = +-inf
//   the limit (inf or +0) instead of the NaN of inf * 0 or inf - inf.  An infinite logit with a
//   soft label is outside the contract.
// ROW AND TOTAL.  row_loss[b] = the terms of the row added one by one in the order c = 0 .. C - 1,
//   starting FROM the first term.  The total is skip-gram's rule with P + K = C: kSgPartials
//   partial sums as a function of B alone (SgLanePartial), the same combine tree, one division by
//   float(B * C) (SgFinish(total, B, C, 0)).  B == 0: loss = +0, no division.
// PREDICTED LABEL.  pred = fl32(p + 0.5f) >= 1.0f - the reference's floor(predict + 0.5) in fp32,
//   not x >= 0: for a tiny negative x the sigmoid returns the float just below 0.5, 0.5 - 2^-25,
//   and the sum, 1 - 2^-25, ties to even at 1.0: the prediction is 1.
// COUNTS (int64): tp, fp, fn, correct, total.  tf.metrics casts to bool for tp / fp / fn (label
//   != 0, prediction != 0); accuracy counts z == float(pred), so a soft label is never correct;
//   total = B * C.
// AUC BUCKETS, for T >= 2 thresholds (tf.metrics.auc's table: Python floats rounded once to fp32):
//   thr_0 = fl32(0 - 1e-7), thr_i = fl32(i / (T - 1)) for 0 < i < T - 1 (the float64 quotient
//   rounded to fp32), thr_(T-1) = fl32(1 + 1e-7).
//   bucket(p) = #{i : thr_i < p}  (strict, TF's `greater`), in [0, T]; the table is increasing, so
//   SvBucket starts from floor(p (T - 1)) + 1 and corrects against the neighbouring thresholds.
//   Two int64 histograms [2][T + 1]: row 0 for label != 0, row 1 for label == 0.  p is bucketed
//   ONCE: auc_score of the reference applies sigmoid to what SuperviseModel has already passed
//   through sigmoid, which squeezes every prediction into [0.5, 0.731]; the map is monotone, so
//   only the resolution differs.
// GRADIENT.  diff = p - z, one fp32 subtract (kept by the forward).  gs = g / float(B * C);
//   g_x = gs * diff, rounded once to the logits' dtype.
// NaN logits are outside the contract.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "skipgram.h"

namespace euler_gpu {

constexpr int kSvCounts = 5;          // tp, fp, fn, correct, total

// the term as the formula states it: one multiply, two adds
EG_MPW_HD float SvTermGeneral(float x, float z) {
  return MpwAdd(MpwAdd(SgRelu(x), -MpwMul(x, z)), Log1pUnit(SgExp(x)));
}

// the term: hard labels through the two identities of the header
EG_MPW_HD float SvTerm(float x, float z) {
  if (z == 0.f) return SgTerm(x, false);
  if (z == 1.f) return SgTerm(x, true);
  return SvTermGeneral(x, z);
}

// floor(p + 0.5) != 0
EG_MPW_HD bool SvPredict(float p) { return MpwAdd(p, 0.5f) >= 1.0f; }

// thr_i of a table of t >= 2 thresholds, 0 <= i < t
EG_MPW_HD float SvThreshold(int32_t i, int32_t t) {
  if (i == 0) return (float)(0.0 - 1e-7);
  if (i == t - 1) return (float)(1.0 + 1e-7);
  return (float)((double)i / (double)(t - 1));
}

// #{i : thr_i < p}, in [0, t]
EG_MPW_HD int32_t SvBucket(float p, int32_t t) {
  if (!(p > SvThreshold(0, t))) return 0;
  double q = (double)p * (double)(t - 1);
  if (q > (double)(t - 1)) q = (double)(t - 1);
  if (q < 0.0) q = 0.0;
  int32_t n = (int32_t)q + 1;                       // thresholds 0 .. n - 1 are presumed below p
  if (n > t) n = t;
  while (n < t && SvThreshold(n, t) < p) ++n;
  while (n > 1 && !(SvThreshold(n - 1, t) < p)) --n;
  return n;
}

// what one element contributes
struct SvElem {
  float p, term, diff;
  bool label, pred, correct;
};

EG_MPW_HD SvElem SvElement(float x, float z) {
  SvElem e;
  e.p = SgSigmoid(x);
  e.term = SvTerm(x, z);
  e.diff = MpwAdd(e.p, -z);
  e.label = z != 0.f;
  e.pred = SvPredict(e.p);
  e.correct = z == (e.pred ? 1.0f : 0.0f);
  return e;
}

// the row sum, one term at a time
EG_MPW_HD float SvRowAdd(float sum, float term, bool first) { return first ? term : MpwAdd(sum, term); }

// gs from g, and one element of the gradient (before the rounding to the logits' dtype)
EG_MPW_HD float SvScale(float g, int64_t b, int64_t c) { return MpwDiv(g, SgCount(b, c, 0)); }
EG_MPW_HD float SvGrad(float gs, float diff) { return MpwMul(gs, diff); }

}  // namespace euler_gpu
