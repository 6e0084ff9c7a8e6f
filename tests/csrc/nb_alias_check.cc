// Host build of the alias neighbour mode (euler_amd/csrc/nb_alias.h, nb_alias_draw.h) for
// tests/test_neighbor_alias_host.py: the same AliasBuild, NbAliasFixup, NbAliasBuildGroup,
// NbAliasRootOf and NbAliasSlot the kernels call, over plain host arrays.  Built with
// -ffp-contract=off, as a shared object for the tests and - it has its own main - as a program that
// reads a graph and a list of calls from files, runs the same functions and writes what they gave
// (the form a sanitizer build runs).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "nb_alias_draw.h"

using namespace euler_gpu;

namespace {

// a GraphView over host arrays: hash id map (the table FindRow probes), nothing else set
struct HostGraph {
  GraphView v;
  std::vector<uint8_t> meta;
  std::vector<uint64_t> slots;
  HostGraph(int64_t n, int32_t T, const uint64_t* row_id, const int64_t* row_ptr, const int32_t* type_end,
            const float* type_prefix, const uint64_t* nbr, const float* prefix_w) {
    memset(&v, 0, sizeof(v));
    v.n_rows = n; v.n_edges = row_ptr[n]; v.T = T; v.meta_stride = 8 + 8 * T;
    meta.resize((size_t)n * v.meta_stride + 16);
    v.has_zero_nbr = 0;
    for (int64_t e = 0; e < v.n_edges; ++e) if (nbr[e] == 0) v.has_zero_nbr = 1;
    for (int64_t r = 0; r < n; ++r) {
      uint8_t* rec = meta.data() + r * v.meta_stride;
      memcpy(rec, &row_ptr[r], 8);
      memcpy(rec + 8, type_end + r * T, 4 * (size_t)T);
      if (type_prefix) memcpy(rec + 8 + 4 * T, type_prefix + r * T, 4 * (size_t)T);
    }
    uint64_t cap = 4;
    while (cap < 2 * (uint64_t)n + 2) cap <<= 1;
    slots.assign(2 * cap, ~0ull);                    // row -1 = empty
    for (int64_t r = 0; r < n && row_id; ++r) {
      uint64_t h = Mix64(row_id[r]) & (cap - 1);
      while ((int64_t)slots[2 * h + 1] >= 0) h = (h + 1) & (cap - 1);
      slots[2 * h] = row_id[r]; slots[2 * h + 1] = (uint64_t)r;
    }
    v.row_meta = meta.data(); v.nbr = nbr; v.prefix_w = prefix_w;
    v.map_mode = 1; v.hash_slots = slots.data(); v.hash_mask = cap - 1; v.monotone = 1;
  }
};

// every (row, group) as NbAliasBuildKernel builds it
void BuildRows(const GraphView& g, NbAliasEntry* tab, int32_t* scratch) {
  for (int64_t i = 0; i < g.n_rows * (int64_t)g.T; ++i) {
    const int64_t row = i / g.T;
    const int32_t t = (int32_t)(i - row * g.T);
    const RowMeta m = LoadRowMeta(g, row);
    const int32_t b = t == 0 ? 0 : m.type_end[t - 1];
    const int32_t d = m.type_end[t] - b;
    if (d <= 0) continue;
    const int64_t first = m.row_ptr + b;
    const float before = b == 0 ? 0.f : g.prefix_w[first - 1];
    (void)NbAliasBuildGroup(tab + first, scratch + first, g.nbr + first, g.prefix_w + first, before, d);
  }
}

void Draw(const GraphView& g, const NbAliasEntry* tab, uint64_t seed, uint32_t call_id, const uint64_t* roots,
          int64_t n, const int32_t* et, int32_t k, int32_t count, int32_t tf, int64_t default_node,
          uint64_t* out_id, float* out_w, int32_t* out_t, uint8_t* out_mask) {
  for (int64_t r = 0; r < n; ++r) {
    const NbAliasRoot root = NbAliasRootOf(g, roots[r], et, k);
    for (int32_t j = 0; j < count; ++j) {
      bool masked;
      NbAliasSlot(g, tab, root, et, k, seed, call_id, roots[r], j, tf != 0, default_node, out_id + r * count + j,
                  out_w + r * count + j, out_t + r * count + j, &masked);
      if (j == 0) out_mask[r] = masked ? 1 : 0;
    }
  }
}

}  // namespace

extern "C" {

// AliasBuild over plain arrays, as the node / edge samplers call it
void nba_alias_init(const float* norm, int64_t n, float* prob, int64_t* alias) {
  std::vector<float> w(norm, norm + n);
  std::vector<int64_t> stack((size_t)n + 1);
  AliasArrays<int64_t> tab{w.data(), prob, alias};
  if (n > 0) AliasBuild(tab, n, stack.data());
}

int64_t nba_fixup(const float* w, float* prob, int64_t* alias, int64_t d) {
  NbAliasFixArrays f{w, prob, alias};
  return NbAliasFixup(f, d);
}

// the tables of a whole graph: tab [E] 32-byte entries
void nba_build(int64_t n, int32_t T, const int64_t* row_ptr, const int32_t* type_end, const uint64_t* nbr,
               const float* prefix_w, void* tab) {
  HostGraph G(n, T, nullptr, row_ptr, type_end, nullptr, nbr, prefix_w);
  std::vector<int32_t> scratch((size_t)row_ptr[n] + 1);
  memset(tab, 0, (size_t)row_ptr[n] * sizeof(NbAliasEntry));
  BuildRows(G.v, (NbAliasEntry*)tab, scratch.data());
}

void nba_draw(int64_t n, int32_t T, const uint64_t* row_id, const int64_t* row_ptr, const int32_t* type_end,
              const float* type_prefix, const uint64_t* nbr, const float* prefix_w, const void* tab, uint64_t seed,
              uint32_t call_id, const uint64_t* roots, int64_t n_roots, const int32_t* et, int32_t k, int32_t count,
              int32_t tf, int64_t default_node, uint64_t* out_id, float* out_w, int32_t* out_t, uint8_t* out_mask) {
  HostGraph G(n, T, row_id, row_ptr, type_end, type_prefix, nbr, prefix_w);
  Draw(G.v, (const NbAliasEntry*)tab, seed, call_id, roots, n_roots, et, k, count, tf, default_node, out_id, out_w,
       out_t, out_mask);
}

}  // extern "C"

// nb_alias_check <in> <out>: <in> = int64 n, T, n_calls | row_id [n] | row_ptr [n + 1] | type_end [n T] i32 |
// type_prefix [n T] f32 | nbr [E] | prefix_w [E] f32 | per call: u64 seed, i64 call_id, k, count, tf, default_node,
// n_roots, i32 et [32], u64 roots [n_roots].  <out> = the E entries, then per call ids | weights | types | masks.
template <typename X>
static bool ReadVec(FILE* f, std::vector<X>* v, size_t n) {
  v->resize(n + 1);
  return n == 0 || fread(v->data(), sizeof(X), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
  int64_t head[3];
  if (fread(head, 8, 3, in) != 3) return 3;
  const int64_t n = head[0], T = head[1], calls = head[2];
  std::vector<uint64_t> row_id, nbr;
  std::vector<int64_t> row_ptr;
  std::vector<int32_t> type_end;
  std::vector<float> type_prefix, prefix_w;
  if (!ReadVec(in, &row_id, (size_t)n) || !ReadVec(in, &row_ptr, (size_t)n + 1) ||
      !ReadVec(in, &type_end, (size_t)(n * T)) || !ReadVec(in, &type_prefix, (size_t)(n * T)))
    return 3;
  const int64_t E = row_ptr[(size_t)n];
  if (!ReadVec(in, &nbr, (size_t)E) || !ReadVec(in, &prefix_w, (size_t)E)) return 3;
  HostGraph G(n, (int32_t)T, row_id.data(), row_ptr.data(), type_end.data(), type_prefix.data(), nbr.data(),
              prefix_w.data());
  std::vector<NbAliasEntry> tab((size_t)E + 1);
  std::vector<int32_t> scratch((size_t)E + 1);
  memset(tab.data(), 0, tab.size() * sizeof(NbAliasEntry));
  BuildRows(G.v, tab.data(), scratch.data());
  fwrite(tab.data(), sizeof(NbAliasEntry), (size_t)E, out);
  for (int64_t c = 0; c < calls; ++c) {
    int64_t h[7];
    int32_t et[32];
    if (fread(h, 8, 7, in) != 7 || fread(et, 4, 32, in) != 32) return 3;
    const int64_t k = h[2], count = h[3], n_roots = h[6];
    std::vector<uint64_t> roots;
    if (!ReadVec(in, &roots, (size_t)n_roots)) return 3;
    const size_t m = (size_t)(n_roots * count);
    std::vector<uint64_t> id(m + 1);
    std::vector<float> w(m + 1);
    std::vector<int32_t> t(m + 1);
    std::vector<uint8_t> mask((size_t)n_roots + 1);
    Draw(G.v, tab.data(), (uint64_t)h[0], (uint32_t)h[1], roots.data(), n_roots, et, (int32_t)k, (int32_t)count,
         (int32_t)h[4], h[5], id.data(), w.data(), t.data(), mask.data());
    fwrite(id.data(), 8, m, out);
    fwrite(w.data(), 4, m, out);
    fwrite(t.data(), 4, m, out);
    fwrite(mask.data(), 1, (size_t)n_roots, out);
  }
  fclose(in);
  fclose(out);
  printf("nb_alias_check: %lld entries, %lld calls\n", (long long)E, (long long)calls);
  return 0;
}
