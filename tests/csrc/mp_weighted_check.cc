// Host build of the per-row arithmetic of the edge-weighted reduces
// (euler_amd/csrc/mp_weighted.h) for tests/test_weighted_mp_host.py: the same
// WeightedReduceRow the kernels call, over plain host arrays.  Built with -ffp-contract=off.
#include <stdint.h>

#include "mp_weighted.h"

using namespace euler_gpu;

namespace {

template <int N>
struct HostOps {
  struct Raw { float v[N]; };
  MpwIndex ix;
  const float* x; int64_t d; int64_t c;
  const float* w; int32_t heads; int32_t head;
  int64_t Pos(int64_t p) const { return ix.Pos(p); }
  int64_t Row(int64_t pos) const { return ix.Row(pos); }
  float Weight(int64_t pos) const { return w[pos * heads + head]; }
  Raw Load(int64_t row) const {
    Raw r;
    for (int k = 0; k < N; ++k) r.v[k] = x[row * d + c + k];
    return r;
  }
  void Widen(const Raw& r, float f[N]) const { for (int k = 0; k < N; ++k) f[k] = r.v[k]; }
};

template <int MODE, int N>
void Row(const float* x, int64_t d, const MpwIndex& ix, const float* w, int32_t heads, int64_t b,
         int64_t en, float* out) {
  const int64_t dh = d / heads;
  for (int64_t c = 0; c < d; c += N) {
    const HostOps<N> ops{ix, x, d, c, w, heads, (int32_t)(c / dh)};
    float acc[N];
    WeightedReduceRow<MODE, N>(ops, b, en, acc);
    for (int k = 0; k < N; ++k) out[c + k] = acc[k];
  }
}

template <int N>
int Mode(int mode, const float* x, int64_t d, const MpwIndex& ix, const float* w, int32_t heads,
         int64_t b, int64_t en, float* out) {
  if (mode == 0) Row<0, N>(x, d, ix, w, heads, b, en, out);
  else if (mode == 1) Row<1, N>(x, d, ix, w, heads, b, en, out);
  else if (mode == 2) Row<2, N>(x, d, ix, w, heads, b, en, out);
  else return -1;
  return 0;
}

}  // namespace

// out[0..d) = destination columns over the grouped positions [b, en).  lane_cols: the columns a
// lane owns (1, 4 or 8 - the kernels' three shapes; 4 and 8 need dh % lane_cols == 0).
// gather / perm may be null; gstride 1 (int32 indices) or 2 (low words of int64 ids).
extern "C" int mpw_reduce_row(int mode, int lane_cols, const float* x, int64_t d, const int32_t* gather,
                              int32_t gstride, uint32_t row_max, const uint32_t* perm, const float* w,
                              int32_t heads, int64_t b, int64_t en, float* out) {
  if (heads < 1 || d % heads != 0 || (d / heads) % lane_cols != 0) return -1;
  const MpwIndex ix{perm, gather, gstride, row_max};
  if (lane_cols == 1) return Mode<1>(mode, x, d, ix, w, heads, b, en, out);
  if (lane_cols == 4) return Mode<4>(mode, x, d, ix, w, heads, b, en, out);
  if (lane_cols == 8) return Mode<8>(mode, x, d, ix, w, heads, b, en, out);
  return -1;
}
