// Host build of the shared pieces of the fused per-column top-k (euler_amd/csrc/mp_topk.h) for
// tests/test_segment_topk_host.py: the segment forms, the index fetch with its range rule, the
// sticky-shift insertion at the template capacity that serves k, and the stored form - driven over
// whole calls on plain host arrays, one (destination, column) at a time.
#include <stdint.h>

#include "mp_topk.h"

using namespace euler_gpu;

namespace {

struct Call {
  const void* params; int64_t rows;
  const void* gather; int32_t is_ids;
  const int64_t* seg_ptr; int64_t count, e, d;
  int32_t size, k;
  float fill;
  void* out; bool out_f32;
  int32_t* sel;
};

template <int DT>
uint32_t Get(const void* base, int64_t at) {
  if (DT == kF32) return static_cast<const uint32_t*>(base)[at];
  return static_cast<const uint16_t*>(base)[at];
}

void Put(void* base, bool f32, int64_t at, uint32_t raw) {
  if (f32) static_cast<uint32_t*>(base)[at] = raw;
  else static_cast<uint16_t*>(base)[at] = (uint16_t)raw;
}

template <int DT, int K, bool SEL>
void Run(const Call& c) {
  const bool out_f32 = DT == kF32 || c.out_f32;
  for (int64_t r = 0; r < c.size; ++r) {
    int64_t b, en;
    TkSegment(c.seg_ptr, c.count, c.e, r, &b, &en);
    for (int64_t col = 0; col < c.d; ++col) {
      float slot[K];
      int32_t pos[K];
      for (int j = 0; j < K; ++j) { slot[j] = 0.f; pos[j] = -1; }
      int32_t seen = 0;
      for (int64_t p = b; p < en; ++p, ++seen) {
        const int64_t row = TkRow(c.gather, c.is_ids, p, c.rows);
        const uint32_t raw = row < 0 ? 0u : Get<DT>(c.params, row * c.d + col);
        TkInsert<K, SEL>(true, TkWiden<DT>(raw), (int32_t)p, seen, slot, SEL ? pos : nullptr);
      }
      for (int j = 0; j < K && j < c.k; ++j) {
        const int64_t at = (r * c.k + j) * c.d + col;
        Put(c.out, out_f32, at, j < seen ? TkStored<DT>(slot[j], out_f32) : TkStored<DT>(c.fill, out_f32));
        if (SEL) c.sel[at] = j < seen ? pos[j] : -1;
      }
    }
  }
}

template <int DT, int K>
void RunSel(const Call& c) {
  if (c.sel) Run<DT, K, true>(c);
  else Run<DT, K, false>(c);
}

template <int DT>
void RunK(const Call& c) {
  switch (TkCapacity(c.k)) {
    case 1: return RunSel<DT, 1>(c);
    case 2: return RunSel<DT, 2>(c);
    case 4: return RunSel<DT, 4>(c);
    case 8: return RunSel<DT, 8>(c);
    default: return RunSel<DT, 16>(c);
  }
}

}  // namespace

extern "C" int tk_capacity(int32_t k) { return TkCapacity(k); }

extern "C" int tk_chunk_width(int64_t d, uint64_t params, int params_f32, uint64_t out, int out_f32, uint64_t sel,
                              int32_t cap) {
  return TkChunkWidth(d, (uintptr_t)params, params_f32 != 0, (uintptr_t)out, out_f32 != 0, (uintptr_t)sel, cap);
}

extern "C" int tk_precedes(float a, float b) { return TkPrecedes(a, b) ? 1 : 0; }

// One whole call on host arrays, the arguments of euler_gpu_gather_segment_topk without the stream;
// dtype codes 0 fp32, 1 bf16, 2 fp16 (16-bit data: uint16).  -> 0, or -1 where the entry returns
// EULER_GPU_EINVAL.
extern "C" int tk_call(const void* params, int32_t in_dt, int64_t rows, const void* gather, int32_t is_ids,
                       const int64_t* seg_ptr, int64_t count, int64_t e, int64_t d, int32_t size, int32_t k,
                       float fill, void* out, int32_t out_dt, int32_t* sel) {
  if (k < 1 || k > kTkMaxK || in_dt < 0 || in_dt > 2 || (out_dt != kF32 && out_dt != in_dt)) return -1;
  if (size < 0 || e < 0 || d < 0 || count < 0 || (seg_ptr != nullptr) == (count > 0)) return -1;
  if (!seg_ptr && e != (int64_t)size * count) return -1;
  if (size == 0 || d == 0) return 0;
  if (!params || !out || rows < 1) return -1;
  const Call c{params, rows, gather, is_ids, seg_ptr, count, e, d, size, k, fill, out, out_dt == kF32, sel};
  if (in_dt == kF32) RunK<kF32>(c);
  else if (in_dt == kBF16) RunK<kBF16>(c);
  else RunK<kF16>(c);
  return 0;
}
