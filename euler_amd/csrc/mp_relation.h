// Per-relation aggregation (RGCN, tf_euler/python/convolution/relation_conv.py): the arithmetic
// of ONE destination - N adjacent columns of its R output rows over the updates of its segment -
// shared by the kernels of relation_kernels.hip and by tests/csrc/mp_relation_check.cc, which
// compiles this file with the host compiler.
//
// Update p of destination r reads row g(p) of the table and has the relation
// t(p) = edge_type[pos(p)], indexed by the update's position in the INPUT (as the weights of
// mp_weighted.h are).  It is VALID when 0 <= t(p) < R; an invalid update (the -1 the samplers
// write beside a default_node fill, a type the caller did not list) belongs to no bucket: it is
// left out of every sum, maximum and count, and its row is never loaded.
// out[r][t][c] folds, in input order, the widened params[g(p)][c] of the valid updates of bucket
// (r, t): MODE 0 add (from 0, correctly rounded fp32 adds), 1 max (from -1e9), 2 the sum divided
// by fl(n_valid(r) + 1e-7f) with n_valid(r) = sum_t cnt(r, t) (relation_conv.py:59: scatter_mean
// over the destination), 3 the sum divided by fl(cnt(r, t) + 1e-7f) (the 1 / c_{i,r} of the RGCN
// paper).  An empty bucket is 0 (add, both means) or -1e9 (max).
//
// The relations are walked in increasing order.  For relation t a scan (Ops::Scan) hands out the
// positions of the bucket's updates in input order: RelLinearScan below re-reads the destination's
// type column from its start, one lane on its own (the host build, the one-column-per-lane
// kernel); the 16-byte-lane kernel shares the column among the lanes of a destination
// (relation_kernels.hip: RelGroupScan; DESIGN 4.13 has the measurement that chose it).  The next
// K = 8 matching positions are gathered, then their K rows are loaded with no branch between the
// loads, then folded in input order; what a bucket has left takes a batch of 4 and then ONE batch
// of the 1 .. 3 updates left (a sampled block has about count / R updates a bucket: taken one at a
// time they would be as many dependent trips to memory).  Every valid update's row is loaded
// exactly once.  No HIP header is needed: a host-only program may include this file on its own.
#pragma once

#include <stdint.h>

#include "mp_weighted.h"

namespace euler_gpu {

constexpr int kRelAdd = 0, kRelMax = 1, kRelMeanDst = 2, kRelMeanRel = 3;

// The next update of relation t at or after grouped position *p (below en): -> its input position
// in *pos, *p behind it.  The types are looked at four at a time - four loads in flight, compared
// in order - so a bucket's scan is en / 4 dependent steps, not en; a look past the segment's end
// re-reads its last update and is ignored.
template <typename Ops>
EG_MPW_HD bool RelNext(const Ops& o, int64_t* p, int64_t en, int32_t t, int64_t* pos) {
  for (int64_t s = *p; s < en; s += 4) {
    int64_t q[4];
    int32_t ty[4];
EG_MPW_UNROLL
    for (int x = 0; x < 4; ++x) q[x] = o.Pos(s + x < en ? s + x : en - 1);
EG_MPW_UNROLL
    for (int x = 0; x < 4; ++x) ty[x] = o.Type(q[x]);
EG_MPW_UNROLL
    for (int x = 0; x < 4; ++x) {
      if (s + x < en && ty[x] == t) {
        *pos = q[x];
        *p = s + x + 1;
        return true;
      }
    }
  }
  *p = en;
  return false;
}

// The scan of one bucket as RelationReduceDest drives it: Next(&pos) hands out the input positions
// of the updates of relation t in input order; CountValid is the destination's n_valid.  This is
// the form every Ops can use (one lane on its own: the host build, the one-column-per-lane
// kernel); the 16-byte-lane kernel has a scan of its own in which the lanes of a destination
// share the type column (relation_kernels.hip: RelGroupScan) - the same positions, the same order.
template <typename Ops>
struct RelLinearScan {
  const Ops& o;
  int64_t p, en;
  int32_t t;
  EG_MPW_HD RelLinearScan(const Ops& ops, int64_t b, int64_t end, int32_t rel) : o(ops), p(b), en(end), t(rel) {}
  EG_MPW_HD bool Next(int64_t* pos) { return RelNext(o, &p, en, t, pos); }
  static EG_MPW_HD int32_t CountValid(const Ops& o, int64_t b, int64_t en, int32_t num_relations) {
    int32_t n = 0;
    for (int64_t p = b; p < en; ++p) n += (uint32_t)o.Type(o.Pos(p)) < (uint32_t)num_relations;
    return n;
  }
};

// K updates at the input positions pos[0..K): row numbers, then all rows, then the ordered fold.
template <int MODE, int N, int K, typename Ops>
EG_MPW_HD void RelBatch(const Ops& o, const int64_t* pos, float acc[N]) {
  int64_t row[K];
  typename Ops::Raw v[K];
EG_MPW_UNROLL
  for (int x = 0; x < K; ++x) row[x] = o.Row(pos[x]);
EG_MPW_UNROLL
  for (int x = 0; x < K; ++x) v[x] = o.Load(row[x]);
EG_MPW_UNROLL
  for (int x = 0; x < K; ++x) {
    float f[N];
    o.Widen(v[x], f);
EG_MPW_UNROLL
    for (int k = 0; k < N; ++k) {
      if (MODE == kRelMax) acc[k] = f[k] > acc[k] ? f[k] : acc[k];
      else acc[k] = MpwAdd(acc[k], f[k]);
    }
  }
}

// The r = 1 .. 3 updates a bucket has left after its batches of 8 and 4: one batch of exactly r
// (EULER_GPU_REL_TAIL_SINGLES, an experiment's build: one at a time, as MpwBatch's tail).
template <int MODE, int N, typename Ops>
EG_MPW_HD void RelTail(const Ops& o, const int64_t* pos, int32_t r, float acc[N]) {
#if defined(EULER_GPU_REL_TAIL_SINGLES)
EG_MPW_UNROLL
  for (int x = 0; x < 3; ++x) {
    if (x < r) RelBatch<MODE, N, 1>(o, pos + x, acc);
  }
#else
  if (r == 3) RelBatch<MODE, N, 3>(o, pos, acc);
  else if (r == 2) RelBatch<MODE, N, 2>(o, pos, acc);
  else if (r == 1) RelBatch<MODE, N, 1>(o, pos, acc);
#endif
}

// The R buckets of the destination whose updates are the grouped positions [b, en).
// Ops supplies: Raw (what one load of the N columns returns), Pos(p) (MpwIndex::Pos), Type(pos),
// Row(pos) (MpwIndex::Row), Load(row), Widen(raw, f[N]) and Scan (RelLinearScan<Ops>, or its own).
// Sink supplies Store(t, acc, cnt), called exactly once per relation, in increasing order, the
// empty buckets included.
template <int MODE, int N, typename Ops, typename Sink>
EG_MPW_HD void RelationReduceDest(const Ops& o, int64_t b, int64_t en, int32_t num_relations, Sink& sink) {
  float dst_denom = 1.f;
  if (MODE == kRelMeanDst)
    dst_denom = MpwAdd((float)Ops::Scan::CountValid(o, b, en, num_relations), 1e-7f);
  for (int32_t t = 0; t < num_relations; ++t) {
    float acc[N];
    const float init = MODE == kRelMax ? (float)-1e9 : 0.f;
EG_MPW_UNROLL
    for (int k = 0; k < N; ++k) acc[k] = init;
    int32_t cnt = 0;
    typename Ops::Scan scan(o, b, en, t);
    for (;;) {
      int64_t pos[8];
      int32_t m = 0;
EG_MPW_UNROLL
      for (int x = 0; x < 8; ++x) {
        if (m == x && scan.Next(&pos[x])) m = x + 1;
      }
      cnt += m;
      if (m == 8) {
        RelBatch<MODE, N, 8>(o, pos, acc);
        continue;
      }
      if (m >= 4) {
        RelBatch<MODE, N, 4>(o, pos, acc);
        RelTail<MODE, N>(o, pos + 4, m - 4, acc);
      } else {
        RelTail<MODE, N>(o, pos, m, acc);
      }
      break;
    }
    if (MODE == kRelMeanDst || MODE == kRelMeanRel) {
      const float denom = MODE == kRelMeanDst ? dst_denom : MpwAdd((float)cnt, 1e-7f);
EG_MPW_UNROLL
      for (int k = 0; k < N; ++k) acc[k] = MpwDiv(acc[k], denom);
    }
    sink.Store(t, acc, cnt);
  }
}

}  // namespace euler_gpu
