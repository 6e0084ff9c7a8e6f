// Largest relative error of the numerator step of mask_attention - v_exp_f32 on fl(x * log2e) - against
// float64 exp over x in [-30, 0]: the figure DESIGN 4.34 records and tests/test_mask_attention_gpu.py
// doubles in its bound.  Every fp32 x = -30 + k * 2^-18 of the range, in blocks; prints one line.
//
//     hipcc --offload-arch=gfx950 -O2 -ffp-contract=off tools/hw_exp_error.hip -o hw_exp_error && ./hw_exp_error
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

__global__ void ExpKernel(const float* x, float* y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = __builtin_amdgcn_exp2f(__fmul_rn(x[i], 1.44269504088896340736f));
}

int main() {
  const int n = 30 << 18;
  std::vector<float> x(n + 1), y(n + 1);
  for (int k = 0; k <= n; ++k) x[k] = -30.0f + (float)k / (float)(1 << 18);
  float *dx, *dy;
  if (hipMalloc(&dx, (n + 1) * 4) != hipSuccess || hipMalloc(&dy, (n + 1) * 4) != hipSuccess) return 1;
  if (hipMemcpy(dx, x.data(), (n + 1) * 4, hipMemcpyHostToDevice) != hipSuccess) return 1;
  hipLaunchKernelGGL(ExpKernel, dim3((n + 256) / 256), dim3(256), 0, 0, dx, dy, n + 1);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 1;
  if (hipMemcpy(y.data(), dy, (n + 1) * 4, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  double worst = 0.0, at = 0.0;
  for (int k = 0; k <= n; ++k) {
    const double want = std::exp((double)x[k]), rel = std::fabs((double)y[k] - want) / want;
    if (rel > worst) { worst = rel; at = x[k]; }
  }
  std::printf("points %d  largest relative error %.4g (%.3f * 2^-24) at x = %.6f  exp(0) = %.9g\n", n + 1, worst,
              worst * 16777216.0, at, (double)y[n]);
  (void)hipFree(dx);
  (void)hipFree(dy);
  return 0;
}
