// TEST INFRASTRUCTURE (not product code): runs the per-item functions of
// euler_amd/csrc/wb_hw.h - the source the builder and hop 2 of the fanout kernels call one
// item per lane - in plain host loops over host arrays, so that `pytest -m "not gpu"` can
// compare their logic with the oracle's RandomSelect.  Compiled on demand by
// tests/test_wb_hw_host.py with `hipcc -ffp-contract=off` (the host pass only is used).
#include <hip/hip_runtime.h>

#include <vector>

#include "wb_hw.h"

using namespace euler_gpu;

namespace {

struct HwHost {
  const float* prefix_w;
  const uint64_t* nbr;
  std::vector<WbRec> rec;
  std::vector<HwLine> lines;
  int64_t overflows = 0;
};

}  // namespace

extern "C" {

// rows of a single-type CSR: row r owns the flat edges [row_ptr[r], row_ptr[r + 1]); prefix_w
// holds row-relative running sums.  The arrays must outlive the handle.
void* hw_build(int64_t n, const int64_t* row_ptr, const float* prefix_w, const uint64_t* nbr) {
  HwHost* g = new HwHost();
  g->prefix_w = prefix_w; g->nbr = nbr;
  g->rec.resize((size_t)n);
  uint64_t lines = 0;
  for (int64_t r = 0; r < n; ++r) {
    const uint32_t deg = (uint32_t)(row_ptr[r + 1] - row_ptr[r]);
    g->rec[(size_t)r] = WbRec{(uint32_t)lines, (uint32_t)row_ptr[r], deg,
                              deg ? prefix_w[row_ptr[r] + deg - 1] : 0.f};
    lines += WbBuckets(deg);
  }
  g->lines.resize((size_t)lines);
  for (int64_t r = 0; r < n; ++r) {
    const WbRec& rec = g->rec[(size_t)r];
    for (uint32_t j = 0; j < WbBuckets(rec.deg); ++j)
      if (HwBuildLine(prefix_w, nbr, rec.lo, rec.deg, rec.total, j, &g->lines[rec.wb_lo + j])) ++g->overflows;
  }
  return g;
}

void hw_destroy(void* h) { delete static_cast<HwHost*>(h); }
int64_t hw_lines(void* h) { return (int64_t)static_cast<HwHost*>(h)->lines.size(); }
int64_t hw_overflows(void* h) { return static_cast<HwHost*>(h)->overflows; }

// line `i` as its 32 words (layout checks)
void hw_line(void* h, int64_t i, uint32_t* out) {
  const HwLine& l = static_cast<HwHost*>(h)->lines[(size_t)i];
  for (int k = 0; k < 32; ++k) out[k] = l.w[k];
}

// One draw u on row rows[i] through the line alone: windows_out = 1 (the guessed entry was the
// answer) / 2 (the entry before it), 0 = cold without a load (the draw is not below the row's
// total), -1 = cold after the line's two entries.  id / weight are set for hot draws only; an empty row reports -2.
void hw_sample(void* h, const int64_t* rows, const double* us, int64_t n, uint64_t* id_out,
               float* w_out, int32_t* windows_out) {
  HwHost* g = static_cast<HwHost*>(h);
  for (int64_t i = 0; i < n; ++i) {
    const WbRec& rec = g->rec[(size_t)rows[i]];
    id_out[i] = 0; w_out[i] = 0.f; windows_out[i] = -2;
    if (rec.deg == 0) continue;
    uint64_t id = 0; float w = 0.f; int32_t win = 0;
    if (HwSampleHot(g->lines.data(), rec, us[i], &id, &w, &win)) {
      id_out[i] = id; w_out[i] = w; windows_out[i] = win;
    } else {
      windows_out[i] = win == 0 ? 0 : -1;
    }
  }
}

}  // extern "C"
