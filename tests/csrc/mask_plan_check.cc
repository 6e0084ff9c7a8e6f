// MaskMakePlan, MaskWaves and the constants of euler_amd/csrc/mp_mask.h through C entries, compiled with
// the host compiler alone (no HIP header) for tests/test_mask_aggregate_host.py and _gpu.py.
#include "mp_mask.h"

extern "C" void mask_plan(int64_t m, int64_t d, int f32, int32_t* out) {
  const euler_gpu::MaskPlan p = euler_gpu::MaskMakePlan(m, d, f32 != 0);
  const int32_t v[5] = {p.nt, p.col_tiles, p.kb, p.stride, p.lds_bytes};
  for (int i = 0; i < 5; ++i) out[i] = v[i];
}

// -> sources of a workgroup's tile at this shape
extern "C" int32_t mask_tile(int64_t batch, int64_t n, int32_t col_tiles) {
  return euler_gpu::MaskTile(euler_gpu::MaskWaves(batch, n, col_tiles));
}

extern "C" int32_t mask_max_blocks() { return euler_gpu::kMaskMaxBlocks; }
