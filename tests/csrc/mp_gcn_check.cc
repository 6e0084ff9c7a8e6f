// Host build of the arithmetic of the GCN-normalised aggregation (euler_amd/csrc/mp_gcn.h) for
// tests/test_gcn_norm_host.py: the same GcnNormOf, GcnNormOps (under WeightedReduceRow) and
// GcnRootEpilogue the kernels call, over plain host arrays.  Built with -ffp-contract=off.
#include <stdint.h>

#include "mp_gcn.h"

using namespace euler_gpu;

namespace {

template <int N>
struct HostLoader {
  struct Raw { float v[N]; };
  const float* x; int64_t d; int64_t c;
  Raw Load(int64_t row) const {
    Raw r;
    for (int k = 0; k < N; ++k) r.v[k] = x[row * d + c + k];
    return r;
  }
  void Widen(const Raw& r, float* f) const { for (int k = 0; k < N; ++k) f[k] = r.v[k]; }
};

template <int MODE, int N>
void Row(const float* x, int64_t d, int64_t rows, const MpwIndex& ix, float nd, const float* norm_src,
         int64_t b, int64_t en, const float* root, float a, float rb, float* out) {
  for (int64_t c = 0; c < d; c += N) {
    const GcnNormOps<HostLoader<N>> ops{HostLoader<N>{x, d, c}, ix, norm_src, (uint32_t)rows, nd};
    float acc[N];
    WeightedReduceRow<MODE, N>(ops, b, en, acc);
    if (root) GcnRootEpilogue<N>(acc, root + c, a, rb);
    for (int k = 0; k < N; ++k) out[c + k] = acc[k];
  }
}

}  // namespace

extern "C" {

// norm[i] = GcnNormOf(deg[i])
void gcn_norm_of(const int32_t* deg, int64_t n, float* norm) {
  for (int64_t i = 0; i < n; ++i) norm[i] = GcnNormOf(deg[i]);
}

// degrees as the device counts them: an edge counts iff both keys are in range
void gcn_degrees(const int32_t* dst, const int32_t* src, int64_t e, int32_t size_dst, int32_t size_src,
                 int32_t* deg_dst, int32_t* deg_src) {
  for (int64_t i = 0; i < e; ++i) {
    const uint32_t a = (uint32_t)dst[i], b = (uint32_t)src[i];
    if (a < (uint32_t)size_dst && b < (uint32_t)size_src) { ++deg_dst[a]; ++deg_src[b]; }
  }
}

// out[0..d) = one destination (norm nd) over the grouped positions [b, en).  lane_cols: the columns
// a lane owns (1 or 4; 4 needs d % 4 == 0).  mode 0 add, 2 mean.  perm and root may be null.
int gcn_reduce_row(int mode, int lane_cols, const float* x, int64_t d, int64_t rows, const int32_t* gather,
                   const uint32_t* perm, float nd, const float* norm_src, int64_t b, int64_t en,
                   const float* root, float agg_scale, float root_scale, float* out) {
  if (rows < 1 || d % lane_cols != 0) return -1;
  const MpwIndex ix{perm, gather, 1, (uint32_t)(rows - 1)};
  if (mode == 0 && lane_cols == 1) Row<0, 1>(x, d, rows, ix, nd, norm_src, b, en, root, agg_scale, root_scale, out);
  else if (mode == 0 && lane_cols == 4) Row<0, 4>(x, d, rows, ix, nd, norm_src, b, en, root, agg_scale, root_scale, out);
  else if (mode == 2 && lane_cols == 1) Row<2, 1>(x, d, rows, ix, nd, norm_src, b, en, root, agg_scale, root_scale, out);
  else if (mode == 2 && lane_cols == 4) Row<2, 4>(x, d, rows, ix, nd, norm_src, b, en, root, agg_scale, root_scale, out);
  else return -1;
  return 0;
}

}  // extern "C"
