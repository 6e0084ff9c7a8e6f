// Host build of the arithmetic of the full-neighbour aggregation (euler_amd/csrc/mp_rows.h) for
// tests/test_neighbor_reduce_host.py: the same RowOps, RowReduce, RowListedDegree and
// GcnRootEpilogue the kernels call, over plain host arrays.  Built with -ffp-contract=off, as a
// shared object for the tests and - it has its own main - as a program that checks the row
// function against a plain loop (the form a sanitizer build runs).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mp_rows.h"

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

struct RowArgs {
  const float* x; int64_t d; int64_t rows;
  const uint64_t* nbr; const float* prefix_w; const int32_t* type_end;
  RowTypeList L; bool self_loop; uint64_t self_id; float nd; const float* norm_src;
  const float* root; float a, b;
};

template <int MODE, int KIND, int N>
void Row(const RowArgs& r, float* out) {
  for (int64_t c = 0; c < r.d; c += N) {
    const RowOps<KIND, HostLoader<N>> ops{HostLoader<N>{r.x, r.d, c}, reinterpret_cast<const uint32_t*>(r.nbr),
                                          r.prefix_w, r.norm_src, (uint32_t)r.rows, r.nd, (uint32_t)r.self_id};
    float acc[N];
    RowReduce<MODE, N>(ops, r.L, r.type_end, r.self_loop, acc);
    if (r.root) GcnRootEpilogue<N>(acc, r.root + c, r.a, r.b);
    for (int k = 0; k < N; ++k) out[c + k] = acc[k];
  }
}

template <int MODE, int KIND>
int RowLanes(int lane_cols, const RowArgs& r, float* out) {
  if (lane_cols == 1) Row<MODE, KIND, 1>(r, out);
  else if (lane_cols == 4) Row<MODE, KIND, 4>(r, out);
  else if (lane_cols == 8) Row<MODE, KIND, 8>(r, out);
  else return -1;
  return 0;
}

template <int MODE>
int RowKind(int kind, int lane_cols, const RowArgs& r, float* out) {
  if (kind == 0) return RowLanes<MODE, 0>(lane_cols, r, out);
  if (kind == 1) return RowLanes<MODE, 1>(lane_cols, r, out);
  if (kind == 2) return RowLanes<MODE, 2>(lane_cols, r, out);
  return -1;
}

RowTypeList TypeList(const int32_t* et, int32_t k, int32_t T) {
  RowTypeList L{};
  L.k = k;
  L.T = T;
  for (int32_t i = 0; i < k; ++i) L.et[i] = et[i];
  return L;
}

}  // namespace

extern "C" {

// out[0..d) = one queried node.  nbr / prefix_w: the row's entries; type_end [T] (NULL: the node has
// no row); lane_cols 1, 4 or 8 (d % lane_cols == 0); mode 0 add, 1 max, 2 mean; kind 0 none, 1 edge,
// 2 norm; root may be NULL.
int neighbor_reduce_row(int mode, int kind, int lane_cols, const float* x, int64_t d, int64_t rows,
                        const uint64_t* nbr, const float* prefix_w, const int32_t* type_end, int32_t T,
                        const int32_t* et, int32_t k, int self_loop, uint64_t self_id, float nd,
                        const float* norm_src, const float* root, float a, float b, float* out) {
  if (rows < 1 || d % lane_cols != 0 || k < 0 || k > 32) return -1;
  const RowArgs r{x, d, rows, nbr, prefix_w, type_end, TypeList(et, k, T), self_loop != 0, self_id, nd, norm_src,
                  root, a, b};
  if (mode == 0) return RowKind<0>(kind, lane_cols, r, out);
  if (mode == 1) return RowKind<1>(kind, lane_cols, r, out);
  if (mode == 2) return RowKind<2>(kind, lane_cols, r, out);
  return -1;
}

int64_t neighbor_listed_degree(const int32_t* type_end, int32_t T, const int32_t* et, int32_t k, int self_loop) {
  return RowListedDegree(TypeList(et, k, T), type_end, self_loop != 0);
}

}  // extern "C"

// The program: rows of 0 .. 70 entries in three groups, every mode and kind, against a plain loop.
int main() {
  const int64_t rows = 19, d = 8;
  std::vector<float> x(rows * d), norm_src(rows);
  for (int64_t i = 0; i < rows * d; ++i) x[i] = (float)((i * 37 % 101) - 50) * 0.03125f;
  for (int64_t i = 0; i < rows; ++i) norm_src[i] = 1.0f / (float)(1 + i % 5);
  int bad = 0;
  for (int32_t len = 0; len <= 70; ++len) {
    std::vector<uint64_t> nbr(len + 1);
    std::vector<float> pw(len + 1);
    float run = 0.f;
    for (int32_t p = 0; p < len; ++p) {
      nbr[p] = (uint64_t)((p * 7 + len) % (rows + 2)) | (p % 3 == 0 ? (1ULL << 40) : 0);
      run += 0.25f + (float)(p % 4);
      pw[p] = run;
    }
    const int32_t type_end[3] = {len / 3, len / 3, len};
    const int32_t et[4] = {2, 0, 5, 0};
    for (int mode = 0; mode < 3; ++mode)
      for (int kind = 0; kind < 3; ++kind)
        for (int self = 0; self < 2; ++self) {
          float want[8], got[8];
          // the plain loop
          std::vector<int32_t> pos;
          for (int32_t p = len / 3; p < len; ++p) pos.push_back(p);
          for (int rep = 0; rep < 2; ++rep)
            for (int32_t p = 0; p < len / 3; ++p) pos.push_back(p);
          if (self) pos.push_back(-1);
          for (int c = 0; c < d; ++c) {
            float acc = mode == 1 ? (float)-1e9 : 0.f;
            for (int32_t p : pos) {
              const uint32_t g = p < 0 ? 3u : (uint32_t)nbr[p];
              float w = 1.0f;
              if (kind == 1 && p >= 0) w = pw[p] - (p == 0 ? 0.f : pw[p - 1]);
              if (kind == 2) w = g < rows ? 0.5f * norm_src[g] : 0.f;
              const float m = x[(g < rows - 1 ? g : rows - 1) * d + c] * w;
              if (mode == 1) acc = m > acc ? m : acc; else acc = acc + m;
            }
            if (mode == 2) acc = acc / ((float)pos.size() + 1e-7f);
            want[c] = acc;
          }
          for (int lanes : {1, 4, 8}) {
            if (neighbor_reduce_row(mode, kind, lanes, x.data(), d, rows, nbr.data(), pw.data(), type_end, 3, et, 4,
                                    self, 3, 0.5f, norm_src.data(), nullptr, 1.f, 1.f, got) != 0 ||
                memcmp(want, got, sizeof want) != 0) {
              printf("mismatch: len %d mode %d kind %d self %d lanes %d\n", len, mode, kind, self, lanes);
              ++bad;
            }
          }
          if (neighbor_listed_degree(type_end, 3, et, 4, self) != (int64_t)pos.size()) ++bad;
        }
  }
  printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
