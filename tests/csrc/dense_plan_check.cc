// DenseMakePlan of euler_amd/csrc/mp_dense.h through a C entry, compiled with the host compiler
// alone (no HIP header) for tests/test_aggregate_dense_host.py.
#include "mp_dense.h"

extern "C" void dense_plan(int64_t d, int64_t ds_w, int64_t f_max, int f32, int32_t* out) {
  const euler_gpu::DensePlan p = euler_gpu::DenseMakePlan(d, ds_w, f_max, f32 != 0);
  const int32_t v[7] = {p.nt, p.f_passes, p.w_tile, p.w_tiles, p.stride_n, p.stride_s, p.lds_bytes};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
}
