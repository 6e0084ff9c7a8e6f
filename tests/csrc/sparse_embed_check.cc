// Host build of the embedding-lookup arithmetic (euler_amd/csrc/sparse_embed.h) for
// tests/test_sparse_embedding_host.py: the same SeFold / SeFinish the kernel calls, driven the way
// the kernel drives them - the entries handed over `group` at a time, the row cut into chunks of N
// columns.  Built with -ffp-contract=off.
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "sparse_embed.h"

using namespace euler_gpu;

namespace {

template <int DT, int N>
struct HostOps {
  struct Raw { float f[N]; };
  const uint8_t* table;
  int64_t dim, col;
  const uint64_t* cur;      // the entries being folded
  int32_t have;             // how many of them exist
  uint64_t Entry(int32_t j) const { return j < have ? cur[j] : 0; }
  Raw Load(int64_t row) const {
    Raw r;
    for (int k = 0; k < N; ++k) {
      const int64_t at = row * dim + col + k;
      if (DT == kF32) {
        memcpy(&r.f[k], table + 4 * at, 4);
      } else {
        uint16_t h;
        memcpy(&h, table + 2 * at, 2);
        r.f[k] = DT == kBF16 ? HalfCvt<kBF16>::Widen(h) : HalfCvt<kF16>::Widen(h);
      }
    }
    return r;
  }
  void Widen(const Raw& v, float* f) const { for (int k = 0; k < N; ++k) f[k] = v.f[k]; }
};

void Store(void* out, int32_t out_dtype, int64_t at, float x) {
  if (out_dtype == kF32) {
    memcpy((uint8_t*)out + 4 * at, &x, 4);
  } else {
    const uint16_t h = out_dtype == kBF16 ? HalfCvt<kBF16>::Narrow(x) : HalfCvt<kF16>::Narrow(x);
    memcpy((uint8_t*)out + 2 * at, &h, 2);
  }
}

template <int DT, int N>
int32_t Row(const uint64_t* v, int32_t len, int32_t has_default, uint64_t dv, const void* table,
            int64_t n_rows, int32_t dim, int32_t combiner, int32_t group, void* out,
            int32_t out_dtype) {
  HostOps<DT, N> o;
  o.table = (const uint8_t*)table;
  o.dim = dim;
  int32_t cnt = 0;
  for (int32_t col = 0; col < dim; col += N) {
    o.col = col;
    float acc[N];
    for (int k = 0; k < N; ++k) acc[k] = 0.f;
    cnt = 0;
    if (len < 1 && has_default) {
      o.cur = &dv;
      o.have = 1;
      SeFold<N, kSeUnroll>(o, 1, (uint64_t)n_rows, acc, &cnt);
    } else {
      for (int32_t e0 = 0; e0 < len; e0 += group) {
        o.cur = v + e0;
        o.have = std::min(group, len - e0);
        SeFold<N, kSeUnroll>(o, o.have, (uint64_t)n_rows, acc, &cnt);
      }
    }
    SeFinish<N>(acc, cnt, combiner);
    for (int k = 0; k < N; ++k) Store(out, out_dtype, col + k, acc[k]);
  }
  return cnt;
}

}  // namespace

extern "C" {

int32_t se_unroll() { return kSeUnroll; }
int32_t se_group_lanes(int64_t chunks) { return SeGroupLanes(chunks); }

// One node.  vec != 0: chunks of 4 (fp32) / 8 (16-bit) columns, dim a multiple of that; else one
// column at a time.  Returns the count, -1 for arguments the kernel's entry would refuse.
int32_t se_row(const uint64_t* v, int32_t len, int32_t has_default, uint64_t default_value,
               const void* table, int32_t dtype, int64_t n_rows, int32_t dim, int32_t combiner,
               int32_t group, int32_t vec, void* out, int32_t out_dtype) {
  if (dim < 1 || n_rows < 1 || group < 1 || combiner < 0 || combiner > 2) return -1;
  if (out_dtype != kF32 && out_dtype != dtype) return -1;
  const int n_vec = dtype == kF32 ? 4 : 8;
  if (vec && dim % n_vec) return -1;
#define SE_ROW(DT, N) \
  return Row<DT, N>(v, len, has_default, default_value, table, n_rows, dim, combiner, group, out, out_dtype)
  if (dtype == kF32) { if (vec) SE_ROW(kF32, 4); SE_ROW(kF32, 1); }
  if (dtype == kBF16) { if (vec) SE_ROW(kBF16, 8); SE_ROW(kBF16, 1); }
  if (dtype == kF16) { if (vec) SE_ROW(kF16, 8); SE_ROW(kF16, 1); }
#undef SE_ROW
  return -1;
}

}  // extern "C"
