// Host build of the per-lane arithmetic and the ordering rules of the table search
// (euler_amd/csrc/table_search.h) for tests/test_table_search_host.py: the same lane functions
// the kernels call, over plain host arrays (already widened to fp32), with the L lanes of a
// (query, row) pair run one after the other and combined by the butterfly the header states, and
// the k best kept in a list that inserts by TsEntryPrecedes - the rows visited forwards or
// backwards, which must not matter.  Built with -ffp-contract=off.
#include <stdint.h>

#include "table_search.h"

using namespace euler_gpu;

namespace {

template <int V>
struct HostRow {
  const float* p;
  void Chunk(int32_t j, float f[V]) const {
    for (int k = 0; k < V; ++k) f[k] = p[(int64_t)j * V + k];
  }
};

// for off = L / 2 .. 1: s = s + s[lane ^ off]; every lane ends with the same bits
template <typename F>
float Sum(int32_t lanes, F lane_part) {
  float s[64], n[64];
  for (int32_t l = 0; l < lanes; ++l) s[l] = lane_part(l);
  for (int32_t off = lanes >> 1; off > 0; off >>= 1) {
    for (int32_t l = 0; l < lanes; ++l) n[l] = MpwAdd(s[l], s[l ^ off]);
    for (int32_t l = 0; l < lanes; ++l) s[l] = n[l];
  }
  return s[0];
}

struct Shape {
  const float* table; int64_t n, d;
  const float* queries; int64_t q;
};

template <int M, int V>
float Inv(const float* row, int64_t d) {
  if (M != kTsCos) return 1.f;
  const int32_t chunks = (int32_t)(d / V), lanes = 1 << KgLogLanes(chunks);
  const HostRow<V> x{row};
  return KgInv(Sum(lanes, [&](int32_t l) { return KgLaneSumSq<V>(x, l, lanes, chunks); }), true);
}

template <int M, int V>
float Score(const Shape& a, int64_t qq, float inv_q, int64_t r) {
  const int32_t chunks = (int32_t)(a.d / V), lanes = 1 << KgLogLanes(chunks);
  const HostRow<V> q{a.queries + qq * a.d}, x{a.table + r * a.d};
  const float s = Sum(lanes, [&](int32_t l) { return TsLaneScore<M, V>(q, x, l, lanes, chunks); });
  return TsFinish(M, s, inv_q, Inv<M, V>(x.p, a.d));
}

template <int M, int V>
void Topk(const Shape& a, int64_t k, const int64_t* exclude, bool backwards, float* scores, int64_t* rows) {
  const bool larger = TsLargerIsBetter(M);
  for (int64_t qq = 0; qq < a.q; ++qq) {
    float es[kTsMaxK];
    int32_t er[kTsMaxK];
    for (int64_t j = 0; j < k; ++j) { es[j] = TsFill(M); er[j] = -1; }
    const float inv_q = Inv<M, V>(a.queries + qq * a.d, a.d);
    const int32_t exc = TsRowOrNone(exclude, qq, a.n);
    for (int64_t i = 0; i < a.n; ++i) {
      const int64_t r = backwards ? a.n - 1 - i : i;
      if (r == exc) continue;
      const float s = Score<M, V>(a, qq, inv_q, r);
      int64_t pos = 0;
      while (pos < k && TsEntryPrecedes(larger, es[pos], er[pos], s, (int32_t)r)) ++pos;
      if (pos >= k) continue;
      for (int64_t j = k - 1; j > pos; --j) { es[j] = es[j - 1]; er[j] = er[j - 1]; }
      es[pos] = s;
      er[pos] = (int32_t)r;
    }
    for (int64_t j = 0; j < k; ++j) { scores[qq * k + j] = es[j]; rows[qq * k + j] = er[j]; }
  }
}

template <int M, int V>
void Rank(const Shape& a, const int64_t* target, const int64_t* exclude, int32_t* rank) {
  const bool larger = TsLargerIsBetter(M);
  for (int64_t qq = 0; qq < a.q; ++qq) {
    const int32_t tgt = TsRowOrNone(target, qq, a.n), exc = TsRowOrNone(exclude, qq, a.n);
    if (tgt < 0) { rank[qq] = -1; continue; }
    const float inv_q = Inv<M, V>(a.queries + qq * a.d, a.d);
    const float st = Score<M, V>(a, qq, inv_q, tgt);
    int32_t c = 0;
    for (int64_t r = 0; r < a.n; ++r)
      if (r != tgt && r != exc && TsCounts(larger, Score<M, V>(a, qq, inv_q, r), st)) ++c;
    rank[qq] = c;
  }
}

template <int M, int V>
void Run(const Shape& a, int64_t k, const int64_t* target, const int64_t* exclude, bool backwards, float* scores,
         int64_t* rows, int32_t* rank) {
  if (rank) Rank<M, V>(a, target, exclude, rank);
  else Topk<M, V>(a, k, exclude, backwards, scores, rows);
}

template <int M>
void RunWidth(int32_t v, const Shape& a, int64_t k, const int64_t* target, const int64_t* exclude, bool backwards,
              float* scores, int64_t* rows, int32_t* rank) {
  if (v == 8) Run<M, 8>(a, k, target, exclude, backwards, scores, rows, rank);
  else if (v == 4) Run<M, 4>(a, k, target, exclude, backwards, scores, rows, rank);
  else Run<M, 1>(a, k, target, exclude, backwards, scores, rows, rank);
}

}  // namespace

extern "C" {

// V of the order for tables of these types at these addresses (the rule the launcher applies)
int ts_chunk_width(int64_t d, uint64_t table, int32_t table_f32, uint64_t queries, int32_t q_f32) {
  return KgChunkWidth(d, (uintptr_t)table, table_f32 != 0, (uintptr_t)queries, q_f32 != 0);
}

// the launch shape, for the tests that state it
int64_t ts_slabs(int64_t n, int64_t tiles) { return TsSlabs(n, tiles); }
int32_t ts_wave_queries(int64_t d, int32_t* staged) {
  bool s;
  const int32_t qw = TsWaveQueriesFor(d, &s);
  *staged = s;
  return qw;
}

// The top-k (rank == nullptr) or the rank of q queries over fp32 host arrays with chunk width v
// (1, 4, 8 with d % v == 0).  backwards: visit the rows from the last to the first.
int ts_search(int32_t v, int32_t metric, const float* table, int64_t n, int64_t d, const float* queries, int64_t q,
              int64_t k, const int64_t* target, const int64_t* exclude, int32_t backwards, float* scores, int64_t* rows,
              int32_t* rank) {
  if (d < 1 || n < 0 || q < 0 || k < 1 || k > kTsMaxK || metric < 0 || metric > 3) return -1;
  if ((v != 1 && v != 4 && v != 8) || d % v != 0) return -1;
  const Shape a{table, n, d, queries, q};
  if (metric == kTsIp) RunWidth<kTsIp>(v, a, k, target, exclude, backwards != 0, scores, rows, rank);
  else if (metric == kTsCos) RunWidth<kTsCos>(v, a, k, target, exclude, backwards != 0, scores, rows, rank);
  else if (metric == kTsL2) RunWidth<kTsL2>(v, a, k, target, exclude, backwards != 0, scores, rows, rank);
  else RunWidth<kTsL1>(v, a, k, target, exclude, backwards != 0, scores, rows, rank);
  return 0;
}

}  // extern "C"
