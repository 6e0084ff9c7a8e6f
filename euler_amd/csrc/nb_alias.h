// Alias tables: the build of AliasMethod::Init (euler/common/alias_method.cc:23-63), shared by the
// global node / edge samplers (graph_build.hip: BuildAliasTables) and by the neighbour alias tables
// of the opt-in O(1) neighbour draw (nb_alias_kernels.hip), and the layout, build rule and draw of
// those neighbour tables.  No HIP header is needed: tests/csrc/nb_alias_check.cc compiles this file
// with the host compiler.
//
// THE NEIGHBOUR TABLE.  One 32-byte entry per edge, at the edge's flat index: entry e describes
// edge e of nbr / prefix_w.  Every (row, edge-type group) has a table of its own over the group's
// d edges - the entries [row_ptr + type_end[t - 1], row_ptr + type_end[t]) - so the row record is
// all the addressing a draw needs.  A draw reads ONE entry: column hit or alias, id and weight of
// either, no dependent load.
//
// BUILD RULE of a group, in storage order (pinned: tests/neighbor_alias_ref.py restates it bit for
// bit):
//   w_i    = fl(prefix_w[e] - prefix_w[e - 1]), 0 before the ROW's first edge: the weight the exact
//            mode returns for the edge
//   S      = the sequential f32 sum of the w_i;  norm_i = fl(w_i / S)
//            (FastWeightedCollection::Init, euler/common/fast_weighted_collection.h:55-75)
//   table  = AliasBuild(norm) below, then NbAliasFixup.
// A group with d == 0 or S == 0 has no table: its entries are all-zero bytes.
//
// THE ONE DEPARTURE FROM THE REFERENCE (NbAliasFixup).  AliasMethod::Init's drain loops give
// prob = 1.0 to whatever is left on the stacks; after float rounding that can be an entry of weight
// 0, which would then be drawn with probability 1 / d.  Here an entry with w_i == 0 that leaves the
// build with prob != 0 gets prob = 0 and the first entry of the group with the largest w as its
// alias.  With it: AN EDGE OF WEIGHT 0 IS NEVER DRAWN (an alias target always had a working weight
// above 1 / d, so its own weight is positive).
#pragma once

#include <math.h>
#include <stdint.h>

#include "philox.h"

// correctly rounded, never contracted (the host build is compiled -ffp-contract=off)
#if defined(__HIP_DEVICE_COMPILE__)
#define EG_NBA_FADD(a, b) __fadd_rn((a), (b))
#define EG_NBA_FSUB(a, b) __fsub_rn((a), (b))
#define EG_NBA_FMUL(a, b) __fmul_rn((a), (b))
#define EG_NBA_FDIV(a, b) __fdiv_rn((a), (b))
#define EG_NBA_DSUB(a, b) __dsub_rn((a), (b))
#define EG_NBA_DMUL(a, b) __dmul_rn((a), (b))
#else
#define EG_NBA_FADD(a, b) ((float)(a) + (float)(b))
#define EG_NBA_FSUB(a, b) ((float)(a) - (float)(b))
#define EG_NBA_FMUL(a, b) ((float)(a) * (float)(b))
#define EG_NBA_FDIV(a, b) ((float)(a) / (float)(b))
#define EG_NBA_DSUB(a, b) ((double)(a) - (double)(b))
#define EG_NBA_DMUL(a, b) ((double)(a) * (double)(b))
#endif

namespace euler_gpu {

// AliasMethod::Init (alias_method.cc:23-63) over caller-provided storage: LIFO small / large
// stacks, `avg` in double, working weights updated in float, prob = fl(w[less] * n) in float.
// Element order is the caller's (Q7).
//   Tab: float w(i) / void set_w(i, x)   the working weights: the normalised weights on entry,
//                                        overwritten
//        void set_prob(i, p), void set_alias(i, a)
//        every element starts with prob 0 and alias 0, as the reference's resize() leaves them
//   stack[n]: the small stack grows up from stack[0], the large one down from stack[n - 1]; an
//   iteration pops one of each and pushes one, so together they never hold more than n.
template <typename Tab, typename Idx>
EG_HD void AliasBuild(Tab& t, int64_t n, Idx* stack) {
  int64_t ns = 0, nl = 0;                  // sizes; large element x lives at stack[n - 1 - x]
  const double avg = 1 / static_cast<double>(n);
  const float fn = (float)(uint64_t)n;     // `weights_[less] * weights_.size()`: size_t -> float
  for (int64_t i = 0; i < n; ++i) {
    t.set_prob(i, 0.f);
    t.set_alias(i, 0);
    if ((double)t.w(i) > avg) stack[n - 1 - nl++] = (Idx)i; else stack[ns++] = (Idx)i;
  }
  while (nl > 0 && ns > 0) {
    const int64_t less = (int64_t)stack[--ns];
    const int64_t more = (int64_t)stack[n - 1 - --nl];
    const float wl = t.w(less);
    t.set_prob(less, EG_NBA_FMUL(wl, fn));
    t.set_alias(less, more);
    // weights_[more] + weights_[less] - avg: a float add, then a double subtraction, stored as float
    const float wm = (float)EG_NBA_DSUB((double)EG_NBA_FADD(t.w(more), wl), avg);
    t.set_w(more, wm);
    if ((double)wm > avg) stack[n - 1 - nl++] = (Idx)more; else stack[ns++] = (Idx)more;
  }
  while (ns > 0) t.set_prob((int64_t)stack[--ns], 1.0f);
  while (nl > 0) t.set_prob((int64_t)stack[n - 1 - --nl], 1.0f);
}

// plain arrays as a table (the node / edge samplers, the tests)
template <typename AliasT>
struct AliasArrays {
  float* wv; float* probv; AliasT* aliasv;
  EG_HD float w(int64_t i) const { return wv[i]; }
  EG_HD void set_w(int64_t i, float x) { wv[i] = x; }
  EG_HD void set_prob(int64_t i, float p) { probv[i] = p; }
  EG_HD void set_alias(int64_t i, int64_t a) { aliasv[i] = (AliasT)a; }
};

// Alias-table entry of the neighbour draw.  w_* is the weight the exact mode returns for that edge.
struct NbAliasEntry {
  uint64_t id_self, id_alias;
  float prob, w_self, w_alias;
  uint32_t pad;                 // 0 (the alias's index inside the group while the group is built)
};
static_assert(sizeof(NbAliasEntry) == 32, "NbAliasEntry must be 32 bytes");

// The zero-weight fix-up (see the head of this file) over
//   Fix: float weight(i)  the edge's own weight w_i;  float prob(i);
//        void set_prob(i, p), void set_alias(i, a)
// Returns the number of entries it changed.
template <typename Fix>
EG_HD int64_t NbAliasFixup(Fix& f, int64_t d) {
  int64_t heaviest = -1, changed = 0;
  for (int64_t i = 0; i < d; ++i) {
    if (f.weight(i) == 0.f && f.prob(i) != 0.f) {
      if (heaviest < 0) {
        heaviest = 0;
        for (int64_t x = 1; x < d; ++x) if (f.weight(x) > f.weight(heaviest)) heaviest = x;
      }
      f.set_prob(i, 0.f);
      f.set_alias(i, heaviest);
      ++changed;
    }
  }
  return changed;
}

// the fix-up over plain arrays (tests)
struct NbAliasFixArrays {
  const float* wv; float* probv; int64_t* aliasv;
  EG_HD float weight(int64_t i) const { return wv[i]; }
  EG_HD float prob(int64_t i) const { return probv[i]; }
  EG_HD void set_prob(int64_t i, float p) { probv[i] = p; }
  EG_HD void set_alias(int64_t i, int64_t a) { aliasv[i] = a; }
};

// One group in place: the entries and the stack scratch of the group's d edges (pointers AT the
// group's first edge), the row's running sums and ids at the same edges, and the running sum before
// the group's first edge (0 for the row's first edge).  While the group is built, w_self holds
// the working weights and pad the alias's index; the last pass writes the final entries.
struct NbAliasGroup {
  NbAliasEntry* e; const float* pw; float before;
  EG_HD float weight(int64_t i) const { return EG_NBA_FSUB(pw[i], i == 0 ? before : pw[i - 1]); }
  EG_HD float w(int64_t i) const { return e[i].w_self; }
  EG_HD void set_w(int64_t i, float x) { e[i].w_self = x; }
  EG_HD float prob(int64_t i) const { return e[i].prob; }
  EG_HD void set_prob(int64_t i, float p) { e[i].prob = p; }
  EG_HD void set_alias(int64_t i, int64_t a) { e[i].pad = (uint32_t)a; }
};

// Returns 1 when the group has a table, 0 when it has none (its entries are zeroed).
EG_HD int NbAliasBuildGroup(NbAliasEntry* e, int32_t* stack, const uint64_t* nbr, const float* pw,
                            float before, int32_t d) {
  NbAliasGroup g{e, pw, before};
  float S = 0.f;
  for (int32_t i = 0; i < d; ++i) S = EG_NBA_FADD(S, g.weight(i));
  if (d <= 0 || S == 0.f) {
    for (int32_t i = 0; i < d; ++i) e[i] = NbAliasEntry{0, 0, 0.f, 0.f, 0.f, 0u};
    return 0;
  }
  for (int32_t i = 0; i < d; ++i) e[i].w_self = EG_NBA_FDIV(g.weight(i), S);
  AliasBuild(g, (int64_t)d, stack);
  (void)NbAliasFixup(g, (int64_t)d);
  for (int32_t i = 0; i < d; ++i) {
    const uint32_t a = e[i].pad;
    e[i].id_self = nbr[i];
    e[i].id_alias = nbr[a];
    e[i].w_self = g.weight(i);
    e[i].w_alias = g.weight(a);
    e[i].pad = 0u;
  }
  return 1;
}

// AliasMethod::Next (alias_method.cc:66-78) over a group's d entries: column = floor(d * u_col) as
// one rounded double product, one 32-byte entry read, u_coin < prob ? self : alias; id and weight
// come from the same entry.
EG_HD void NbAliasPick(const NbAliasEntry* tab, int32_t d, double u_col, double u_coin, uint64_t* id,
                       float* w) {
  const int64_t column = (int64_t)floor(EG_NBA_DMUL((double)d, u_col));
  const NbAliasEntry e = tab[column];
  const bool self = u_coin < (double)e.prob;
  *id = self ? e.id_self : e.id_alias;
  *w = self ? e.w_self : e.w_alias;
}

}  // namespace euler_gpu
