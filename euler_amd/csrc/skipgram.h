// The skip-gram loss head of the walk-based models (DeepWalk, node2vec, LINE, unsupervised
// GraphSAGE: tf_euler/python/solution/base_unsupervise.py with PosNegLogits of
// solution/logits.py:30-34, xent_loss of solution/losses.py:27-33 and mrr_score / hitk_score /
// mr_score of utils/metrics.py:51-83): the arithmetic of ONE LANE of one pair row, shared by the
// kernels of skipgram_kernels.hip and by tests/csrc/skipgram_check.cc, which compiles this file
// with the host compiler.  Every operation is a correctly rounded fp32 multiply, add or divide
// (MpwMul / MpwAdd / MpwDiv: the __f*_rn forms on the device, plain operators in a translation
// unit built with -ffp-contract=off on the host), a comparison or an integer operation: host and
// device return the same bits by construction.
//
// INPUTS.  target [Nt, d] and context [Nc, d]: fp32, bf16 or fp16, each its own type, widened
// exactly; the two may be the same table.  src [B], pos [B, P] (P >= 1), neg [B, K] (K >= 0):
// signed int64.  RANGE RULE (that of kg_score.h): an id outside [0, rows) of its table names no
// row.  It is never dereferenced, reads as a row of +0 and its gradient row is written as +0.
// Its term still counts in the loss (its logit is 0: a term of Log1pUnit(1), ln 2).
//
// LOGITS.  With t = target[src[b]] and c_j = context[pos[b][j]] for j < P, context[neg[b][j - P]]
// for P <= j < P + K:   x_j = sum_c t_c * c_{j,c}   (one product, then the sum).  The chunk width
// V, the lane count L, the per-lane order and the butterfly are exactly those kg_score.h states,
// with V = KgChunkWidth(d, target, context): lane l adds the products of its chunks l, l + L, ...
// one by one in increasing column order starting FROM its first product (KgAcc), a lane without
// a chunk holds +0, then for off = L / 2, ..., 1: s = s + s[lane ^ off].
//
// LOSS.  e = ExpNonPositive(-|x|) (mp_softmax.h: +0 below -86), and
//   Log1pUnit(e), e in [0, 1]:  s = e / (2 + e), u = s * s,
//                               q = 1/3 + u (1/5 + u (1/7 + u (1/9 + u (1/11 + u (1/13 + u / 15)))))
//                               (Horner, the constants rounded to fp32), result = 2 s + 2 s * (u * q)
//   (ln(1 + e) = 2 atanh(s); no fitted constant).  Log1pUnit(0) = +0.  For every e that
//   ExpNonPositive returns (0, or >= 2^-124.08) s is a normal number, and the result does not
//   depend on how denormals are handled: where u is below the normal range, 2 s * (u * q) is
//   below a quarter ulp of 2 s whichever way u was rounded.
//   positive j < P:   term_j = max(-x_j, 0) + Log1pUnit(e_j)      (softplus(-x))
//   negative j >= P:  term_j = max( x_j, 0) + Log1pUnit(e_j)      (softplus(x))
//   max(y, 0) is y > 0 ? y : +0.  Largest errors against float64: DESIGN 4.19.
// ROW SUM: row_loss[b] = the terms of the row added one by one, j = 0 .. P + K - 1, starting FROM
// the first term.
// TOTAL: kSgPartials (256) partial sums, a function of B alone and never of the grid.  Partial l
// starts from +0 and adds row_loss[b] for b = l, l + 256, l + 512, ... in increasing b
// (SgLanePartial).  Combine tree (that of mp_softmax.h): the 256 partials are cut into 4 runs of
// 64 adjacent ones; inside a run a butterfly, for off = 32, 16, ..., 1: s_l = s_l + s_(l ^ off);
// then the four run sums as (S0 + S1) + (S2 + S3) (SmxCombine4).  loss = total / float(B * (P + K)),
// one division (the count converted to fp32 by round-to-nearest; it is below 2^31).  B == 0:
// loss = +0, no division.
//
// RANK.  rank[b] (int32) = the number of j among the first P - 1 positives and the K negatives
// with x_j >= x_(P-1), the LAST positive's logit.  This is tf.nn.top_k's lower-index-first tie
// rule on concat([neg, pos]) (metrics.py:51-83): a tie goes against the positive.  K == 0 and
// P == 1 give rank 0.  mrr = mean 1 / (rank + 1), mr = mean rank + 1, hit@k = mean [rank < k].
// NaN logits are outside the contract (a NaN never compares >=, so it is never counted).
//
// GRADIENT, given the scalar g of the loss and the forward's logits (no dot product is taken
// again):  gs = g / float(B * (P + K));  e = ExpNonPositive(-|x_j|);
//   sig = x_j >= 0 ? 1 / (1 + e) : e / (1 + e);
//   c_j = gs * (sig - 1) for a positive, gs * sig for a negative  (exact at the extremes: e = 0
//   gives sig exactly 1 or 0, so c_j is a zero, -gs or gs);
//   G_ctx_j = c_j * t  per column (a row the range rule removed: +0);
//   G_src   = sum_j c_j * ctx_j per column, each contribution one add in the order j = 0 ..
//             P + K - 1 starting from +0 (a src the range rule removed: +0).
// The gradients refer to the raw table rows, in fp32, one row per occurrence; a table's gradient
// is their scatter_add by id.
// No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "kg_score.h"
#include "mp_softmax.h"
#include "mp_weighted.h"

namespace euler_gpu {

constexpr int kSgPartials = 256;       // partial sums of the total: 4 runs of 64

// ln(1 + e) for e in [0, 1]
EG_MPW_HD float Log1pUnit(float e) {
  const float s = MpwDiv(e, MpwAdd(2.0f, e));
  const float u = MpwMul(s, s);
  float q = 0x1.111112p-4f;                       // 1 / 15
  q = MpwAdd(MpwMul(q, u), 0x1.3b13b2p-4f);       // 1 / 13
  q = MpwAdd(MpwMul(q, u), 0x1.745d18p-4f);       // 1 / 11
  q = MpwAdd(MpwMul(q, u), 0x1.c71c72p-4f);       // 1 / 9
  q = MpwAdd(MpwMul(q, u), 0x1.24924ap-3f);       // 1 / 7
  q = MpwAdd(MpwMul(q, u), 0x1.99999ap-3f);       // 1 / 5
  q = MpwAdd(MpwMul(q, u), 0x1.555556p-2f);       // 1 / 3
  const float s2 = MpwAdd(s, s);
  return MpwAdd(s2, MpwMul(s2, MpwMul(u, q)));
}

EG_MPW_HD float SgRelu(float y) { return y > 0.f ? y : 0.f; }

// e of a logit
EG_MPW_HD float SgExp(float x) { return ExpNonPositive(-KgAbs(x)); }

// the loss term of a logit: softplus(-x) of a positive, softplus(x) of a negative
EG_MPW_HD float SgTerm(float x, bool positive) {
  return MpwAdd(SgRelu(positive ? -x : x), Log1pUnit(SgExp(x)));
}

// the logistic function of a logit
EG_MPW_HD float SgSigmoid(float x) {
  const float e = SgExp(x);
  const float den = MpwAdd(1.0f, e);
  return x >= 0.f ? MpwDiv(1.0f, den) : MpwDiv(e, den);
}

// float(B * (P + K))
EG_MPW_HD float SgCount(int64_t b, int64_t p, int64_t k) { return (float)(b * (p + k)); }

// c_j from gs and the logit
EG_MPW_HD float SgCoef(float gs, float x, bool positive) {
  const float sig = SgSigmoid(x);
  return MpwMul(gs, positive ? MpwAdd(sig, -1.0f) : sig);
}

// A Row is what a lane sees of one table row, an Acc a lane's columns of G_src, an Out a lane's
// columns of an output row: Chunk(j, f), Get(j, f) / Put(j, f) over chunks of V columns, as in
// kg_score.h.

// a lane's part of x_j = sum t_c * c_c
template <int V, typename RowT, typename RowC>
EG_MPW_HD float SgLaneDot(const RowT& t, const RowC& c, int32_t l, int32_t lanes, int32_t chunks) {
  float s = 0.f;
  bool first = true;
  for (int32_t j = l; j < chunks; j += lanes) {
    float ft[V], fc[V];
    t.Chunk(j, ft);
    c.Chunk(j, fc);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) KgAcc(MpwMul(ft[k], fc[k]), &s, &first);
  }
  return s;
}

// The row of logits, one at a time in the order the row sum needs: Add(x_j) for j = 0 .. P + K - 1
// after Last(x_(P-1)), the last positive's logit, which the rank compares with.
struct SgRowState {
  float last, sum;
  int32_t rank;
  int64_t j, p;
  EG_MPW_HD void Start(int64_t positives, float x_last) { last = x_last; sum = 0.f; rank = 0; j = 0; p = positives; }
  EG_MPW_HD void Add(float x) {
    const float term = SgTerm(x, j < p);
    sum = j == 0 ? term : MpwAdd(sum, term);
    if (j != p - 1 && x >= last) ++rank;
    ++j;
  }
};

// partial l of the total: +0, then row_loss[l], row_loss[l + 256], ...
EG_MPW_HD float SgLanePartial(const float* row_loss, int64_t l, int64_t b) {
  float s = 0.f;
  for (int64_t i = l; i < b; i += kSgPartials) s = MpwAdd(s, row_loss[i]);
  return s;
}

// the loss from the combined total
EG_MPW_HD float SgFinish(float total, int64_t b, int64_t p, int64_t k) {
  return b == 0 ? 0.f : MpwDiv(total, SgCount(b, p, k));
}

// one context row of the gradient: G_ctx_j = c * t into `gc`, and c * ctx_j added to the lane's G_src
template <int V, typename RowT, typename RowC, typename Acc, typename Out>
EG_MPW_HD void SgLaneGrad(float c, bool ctx_ok, const RowT& t, const RowC& ctx, Acc& gsrc, Out& gc, int32_t l,
                          int32_t lanes, int32_t chunks) {
  for (int32_t j = l; j < chunks; j += lanes) {
    float ft[V], fc[V], ps[V], pc[V];
    t.Chunk(j, ft);
    ctx.Chunk(j, fc);
    gsrc.Get(j, ps);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) {
      ps[k] = MpwAdd(ps[k], MpwMul(c, fc[k]));
      pc[k] = ctx_ok ? MpwMul(c, ft[k]) : 0.f;
    }
    gsrc.Put(j, ps);
    gc.Put(j, pc);
  }
}

// the lane's G_src, complete, stored through `out` (which may be its own storage)
template <int V, typename Acc, typename Out>
EG_MPW_HD void SgLaneSrcGrad(bool src_ok, const Acc& gsrc, Out& out, int32_t l, int32_t lanes, int32_t chunks) {
  for (int32_t j = l; j < chunks; j += lanes) {
    float p[V];
    gsrc.Get(j, p);
EG_MPW_UNROLL
    for (int k = 0; k < V; ++k) if (!src_ok) p[k] = 0.f;
    out.Put(j, p);
  }
}

}  // namespace euler_gpu
