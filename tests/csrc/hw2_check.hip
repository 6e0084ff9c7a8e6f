// TEST INFRASTRUCTURE (not product code): runs the per-item functions of
// euler_amd/csrc/wb_hw2.h - the source the builder and hop 2 of the fanout kernels call one
// item per lane - in plain host loops over host arrays, so that `pytest -m "not gpu"` can
// compare their logic with the oracle's RandomSelect; the lines of wb_hw.h are built over the
// same rows, so the two formats' second-entry shares come from the same draws.  Compiled on
// demand by tests/test_wb_hw2_host.py with `hipcc -ffp-contract=off` (the host pass only is used).
#include <hip/hip_runtime.h>

#include <vector>

#include "wb_hw2.h"

using namespace euler_gpu;

namespace {

struct Hw2Host {
  std::vector<WbRec> rec;
  std::vector<HwLine> lines;      // wb_hw2.h
  std::vector<HwLine> lines1;     // wb_hw.h, same buckets
  int64_t overflows = 0;
};

}  // namespace

extern "C" {

// rows of a single-type CSR: row r owns the flat edges [row_ptr[r], row_ptr[r + 1]); prefix_w
// holds row-relative running sums.
void* hw2_build(int64_t n, const int64_t* row_ptr, const float* prefix_w, const uint64_t* nbr) {
  Hw2Host* g = new Hw2Host();
  g->rec.resize((size_t)n);
  uint64_t lines = 0;
  for (int64_t r = 0; r < n; ++r) {
    const uint32_t deg = (uint32_t)(row_ptr[r + 1] - row_ptr[r]);
    g->rec[(size_t)r] = WbRec{(uint32_t)lines, (uint32_t)row_ptr[r], deg,
                              deg ? prefix_w[row_ptr[r] + deg - 1] : 0.f};
    lines += WbBuckets(deg);
  }
  g->lines.resize((size_t)lines);
  g->lines1.resize((size_t)lines);
  for (int64_t r = 0; r < n; ++r) {
    const WbRec& rec = g->rec[(size_t)r];
    for (uint32_t j = 0; j < WbBuckets(rec.deg); ++j) {
      if (Hw2BuildLine(prefix_w, nbr, rec.lo, rec.deg, rec.total, j, &g->lines[rec.wb_lo + j])) ++g->overflows;
      HwBuildLine(prefix_w, nbr, rec.lo, rec.deg, rec.total, j, &g->lines1[rec.wb_lo + j]);
    }
  }
  return g;
}

void hw2_destroy(void* h) { delete static_cast<Hw2Host*>(h); }
int64_t hw2_lines(void* h) { return (int64_t)static_cast<Hw2Host*>(h)->lines.size(); }
int64_t hw2_overflows(void* h) { return static_cast<Hw2Host*>(h)->overflows; }

// line `i` as its 32 words (layout checks); which = 1: the line of wb_hw.h for the same bucket
void hw2_line(void* h, int64_t i, int32_t which, uint32_t* out) {
  Hw2Host* g = static_cast<Hw2Host*>(h);
  const HwLine& l = which ? g->lines1[(size_t)i] : g->lines[(size_t)i];
  for (int k = 0; k < 32; ++k) out[k] = l.w[k];
}

// One draw u on row rows[i] through the line alone.  windows_out: 1 / 2 = settled by the first /
// second window (id / weight set), 0 = cold without a load (the draw is not below the row's
// total), -1 / -2 = cold after one / two windows; an empty row reports -3.  old_windows_out: what
// HwSampleHot (wb_hw.h) reports for the same draw: 1, 2 (the entry before the guessed one), or
// <= 0 cold (-3: empty row).
void hw2_sample(void* h, const int64_t* rows, const double* us, int64_t n, uint64_t* id_out,
                float* w_out, int32_t* windows_out, int32_t* old_windows_out) {
  Hw2Host* g = static_cast<Hw2Host*>(h);
  for (int64_t i = 0; i < n; ++i) {
    const WbRec& rec = g->rec[(size_t)rows[i]];
    id_out[i] = 0; w_out[i] = 0.f; windows_out[i] = -3; old_windows_out[i] = -3;
    if (rec.deg == 0) continue;
    uint64_t id = 0; float w = 0.f; int32_t win = 0;
    if (Hw2SampleHot(g->lines.data(), rec, us[i], &id, &w, &win)) { id_out[i] = id; w_out[i] = w; }
    windows_out[i] = win;
    uint64_t id1 = 0; float w1 = 0.f; int32_t win1 = 0;
    const bool hot1 = HwSampleHot(g->lines1.data(), rec, us[i], &id1, &w1, &win1);
    old_windows_out[i] = hot1 ? win1 : (win1 == 0 ? 0 : -1);
  }
}

}  // extern "C"
