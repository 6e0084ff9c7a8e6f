// GruMakePlan and GruStateRow of euler_amd/csrc/mp_gru.h through C entries, compiled with the host
// compiler alone (no HIP header) for tests/test_aggregate_gru_host.py.
#include "mp_gru.h"

extern "C" void gru_plan(int64_t d, int64_t u, int f32, int32_t* out) {
  const euler_gpu::GruPlan p = euler_gpu::GruMakePlan(d, u, f32 != 0);
  const int32_t v[8] = {p.ch, p.nt, p.kd, p.ku, p.r_passes, p.c_passes, p.stride, p.lds_bytes};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
}

extern "C" int32_t gru_state_row(int32_t slot) { return euler_gpu::GruStateRow(slot); }
