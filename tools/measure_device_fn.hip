// Largest relative error, against float64 on the host, of the four device functions the kernels use that are not exactly rounded:
// rsqrtf (GroupNorm), expf (softmax), tanhf and v / (1 + __expf(-v)) (apply_act of csrc/common.h), each over the argument range of the
// rows of tests/front_cases.py.  The bounds of tests/test_gpu_front_kernels.py are 4 x these figures (DESIGN.md lists them).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/measure_device_fn.hip -o measure_device_fn && ./measure_device_fn
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

__global__ void eval_kernel(const float* __restrict__ a, float* __restrict__ y, int n, int fn) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = a[i];
  y[i] = fn == 0 ? rsqrtf(v) : fn == 1 ? expf(v) : fn == 2 ? tanhf(v) : v / (1.f + __expf(-v));
}

static double ref(int fn, double v) {
  return fn == 0 ? 1.0 / std::sqrt(v) : fn == 1 ? std::exp(v) : fn == 2 ? std::tanh(v) : v / (1.0 + std::exp(-v));
}

int main() {
  const char* name[4] = {"rsqrtf", "expf", "tanhf", "silu"};
  const double lo[4] = {1.0 / 1024, -87.0, -24.0, -24.0}, hi[4] = {128.0, 0.0, 24.0, 24.0};
  const int n = 1 << 22;
  float *da, *dy;
  if (hipMalloc(&da, n * sizeof(float)) != hipSuccess || hipMalloc(&dy, n * sizeof(float)) != hipSuccess) return 1;
  for (int fn = 0; fn < 4; ++fn) {
    std::vector<float> a(n), y(n);
    for (int i = 0; i < n; ++i) {
      // half the points uniform over the range, half on the grid of multiples of 1/64 the test rows sit on
      const double u = (i >> 1) / (double)(n >> 1);
      const double v = lo[fn] + (hi[fn] - lo[fn]) * u;
      a[i] = (i & 1) ? (float)(std::floor(v * 64.0) / 64.0) : (float)v;
      if (fn == 0 && a[i] <= 0.f) a[i] = (float)lo[0];
    }
    if (hipMemcpy(da, a.data(), n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return 1;
    hipLaunchKernelGGL(eval_kernel, dim3(n / 256), dim3(256), 0, 0, da, dy, n, fn);
    if (hipMemcpy(y.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    double worst = 0.0, at = 0.0;
    for (int i = 0; i < n; ++i) {
      const double r = ref(fn, (double)a[i]);
      if (r == 0.0 || std::fabs(r) < 1e-37) continue;        // below the fp32 normal range: no relative figure
      const double e = std::fabs((double)y[i] - r) / std::fabs(r);
      if (e > worst) { worst = e; at = a[i]; }
    }
    printf("%-7s [%g, %g]: max relative error %.3e (%.2f fp32 ulp of 2^-24) at %.9g\n", name[fn], lo[fn], hi[fn], worst, worst * 16777216.0, at);
  }
  (void)hipFree(da);
  (void)hipFree(dy);
  return 0;
}
