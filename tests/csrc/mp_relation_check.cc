// Host build of the per-destination arithmetic of the per-relation aggregation
// (euler_amd/csrc/mp_relation.h) for tests/test_relation_reduce_host.py: the same
// RelationReduceDest the kernels call, over plain host arrays.  Built with -ffp-contract=off.
#include <stdint.h>

#include "mp_relation.h"

using namespace euler_gpu;

namespace {

template <int N>
struct HostOps {
  struct Raw { float v[N]; };
  using Scan = RelLinearScan<HostOps<N>>;
  MpwIndex ix;
  const int32_t* type;
  const float* x; int64_t d; int64_t c;
  int64_t* loads;                       // loads[row] += 1 per Load (counted for column 0 only)
  int64_t Pos(int64_t p) const { return ix.Pos(p); }
  int32_t Type(int64_t pos) const { return type[pos]; }
  int64_t Row(int64_t pos) const { return ix.Row(pos); }
  Raw Load(int64_t row) const {
    Raw r;
    for (int k = 0; k < N; ++k) r.v[k] = x[row * d + c + k];
    if (loads && c == 0) ++loads[row];
    return r;
  }
  void Widen(const Raw& r, float f[N]) const { for (int k = 0; k < N; ++k) f[k] = r.v[k]; }
};

template <int N>
struct HostSink {
  float* out; int32_t* counts; int64_t d; int64_t c;
  int32_t* stores;                      // stores[t] += 1 per Store (column 0 only)
  void Store(int32_t t, const float acc[N], int32_t cnt) const {
    for (int k = 0; k < N; ++k) out[t * d + c + k] = acc[k];
    if (c == 0) { counts[t] = cnt; if (stores) ++stores[t]; }
  }
};

template <int MODE, int N>
void Dest(const float* x, int64_t d, const MpwIndex& ix, const int32_t* type, int32_t R, int64_t b,
          int64_t en, float* out, int32_t* counts, int64_t* loads, int32_t* stores) {
  for (int64_t c = 0; c < d; c += N) {
    const HostOps<N> ops{ix, type, x, d, c, loads};
    HostSink<N> sink{out, counts, d, c, stores};
    RelationReduceDest<MODE, N>(ops, b, en, R, sink);
  }
}

template <int N>
int Mode(int mode, const float* x, int64_t d, const MpwIndex& ix, const int32_t* type, int32_t R,
         int64_t b, int64_t en, float* out, int32_t* counts, int64_t* loads, int32_t* stores) {
  if (mode == 0) Dest<0, N>(x, d, ix, type, R, b, en, out, counts, loads, stores);
  else if (mode == 1) Dest<1, N>(x, d, ix, type, R, b, en, out, counts, loads, stores);
  else if (mode == 2) Dest<2, N>(x, d, ix, type, R, b, en, out, counts, loads, stores);
  else if (mode == 3) Dest<3, N>(x, d, ix, type, R, b, en, out, counts, loads, stores);
  else return -1;
  return 0;
}

}  // namespace

// out[R, d] / counts[R] = the buckets of the destination whose updates are the grouped positions
// [b, en).  lane_cols: the columns a lane owns (1, 4 or 8; d % lane_cols == 0).  gather / perm may
// be null; gstride 1 (int32 indices) or 2 (low words of int64 ids).  loads [table rows] and stores
// [R] (either may be null) count the row loads and the bucket stores of column 0.
extern "C" int mpr_reduce_dest(int mode, int lane_cols, const float* x, int64_t d, const int32_t* gather,
                               int32_t gstride, uint32_t row_max, const uint32_t* perm,
                               const int32_t* type, int32_t num_relations, int64_t b, int64_t en,
                               float* out, int32_t* counts, int64_t* loads, int32_t* stores) {
  if (num_relations < 1 || d % lane_cols != 0) return -1;
  const MpwIndex ix{perm, gather, gstride, row_max};
  if (lane_cols == 1) return Mode<1>(mode, x, d, ix, type, num_relations, b, en, out, counts, loads, stores);
  if (lane_cols == 4) return Mode<4>(mode, x, d, ix, type, num_relations, b, en, out, counts, loads, stores);
  if (lane_cols == 8) return Mode<8>(mode, x, d, ix, type, num_relations, b, en, out, counts, loads, stores);
  return -1;
}
