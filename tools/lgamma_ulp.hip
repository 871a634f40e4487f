// lgamma_ulp.hip — the largest error of the device's fp64 lgamma and log, in fp64 ulps of the exact value,
// against the host's lgammal / logl, over the arguments the structure-score cases produce: the integers
// 1 .. max_count and integer + beta for the betas (and alphas) of the tests' families.  Stand-alone: it
// calls the math library functions the score kernel calls, not the kernel.  The result is the U of the
// tests' error bound (tests/score_cases.py, DESIGN.md "Structure scores").
//   hipcc --offload-arch=gfx950 -O3 tools/lgamma_ulp.hip -o lgamma_ulp && ./lgamma_ulp [max_count]
//   ./lgamma_ulp --args FILE
// measures a list of arguments instead: FILE holds lines "lgamma <x>" and "log <x>" (hexadecimal floats), as
// tests/crafted_cases.py write_ulp_arguments writes the distinct arguments of the large-count score cases
// (score_cases.U_DEVICE_LARGE records the result).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define HIP_OK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
      return 2;                                                                       \
    }                                                                                 \
  } while (0)

__global__ void k_eval(const double *__restrict__ x, int64_t n, int32_t use_log, double *__restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = use_log ? log(x[i]) : lgamma(x[i]);
}

// error of `got` in ulps of the fp64 nearest to `exact`
static double ulps(double got, long double exact) {
  const double e = (double)exact;
  if (e == 0.0) return got == 0.0 ? 0.0 : INFINITY;
  const double ulp = std::nextafter(std::fabs(e), INFINITY) - std::fabs(e);
  return (double)(fabsl((long double)got - exact) / (long double)ulp);
}

static int run(const std::vector<double> &x, int use_log, const char *what, double *worst_all) {
  const int64_t n = (int64_t)x.size();
  double *dx = nullptr, *dy = nullptr;
  HIP_OK(hipMalloc(&dx, n * sizeof(double)));
  HIP_OK(hipMalloc(&dy, n * sizeof(double)));
  HIP_OK(hipMemcpy(dx, x.data(), n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, n, use_log, dy);
  HIP_OK(hipGetLastError());
  std::vector<double> y((size_t)n);
  HIP_OK(hipMemcpy(y.data(), dy, n * sizeof(double), hipMemcpyDeviceToHost));
  HIP_OK(hipFree(dx));
  HIP_OK(hipFree(dy));
  double worst = 0.0, at = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    const long double exact = use_log ? logl((long double)x[i]) : lgammal((long double)x[i]);
    const double u = ulps(y[i], exact);
    if (u > worst) worst = u, at = x[i];
  }
  printf("%-28s n %9lld  worst %.3f ulp at x = %.17g\n", what, (long long)n, worst, at);
  if (worst > *worst_all) *worst_all = worst;
  return 0;
}

static int run_list(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    return 2;
  }
  std::vector<double> lg, lo;
  char what[16];
  double v;
  while (fscanf(f, "%15s %la", what, &v) == 2) {
    if (strcmp(what, "lgamma") == 0) lg.push_back(v);
    else if (strcmp(what, "log") == 0) lo.push_back(v);
    else {
      fprintf(stderr, "%s: unknown function %s\n", path, what);
      fclose(f);
      return 2;
    }
  }
  fclose(f);
  double worst = 0.0;
  if (!lg.empty() && run(lg, 0, "lgamma(listed)", &worst)) return 2;
  if (!lo.empty() && run(lo, 1, "log(listed)", &worst)) return 2;
  printf("U = %.3f\n", worst);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 2 && strcmp(argv[1], "--args") == 0) return run_list(argv[2]);
  const int64_t max_count = argc > 1 ? atoll(argv[1]) : 100000;
  if (max_count < 1 || max_count > 100000000) {
    fprintf(stderr, "max_count 1 .. 1e8\n");
    return 2;
  }
  // 10 / q and 10 / (q r) of the tests' families (equivalent sample size 10), and the integers (K2: 1 and r)
  const double denom[] = {1,  2,  3,   4,   6,   8,   9,   12,  16,   18,   24,    27,
                          36, 54, 72, 81, 108, 162, 254, 381, 384, 1260, 4096, 4097, 12288};
  double worst = 0.0;
  std::vector<double> x;
  for (int64_t n = 1; n <= max_count + 254; ++n) x.push_back((double)n);
  if (run(x, 0, "lgamma(integer)", &worst)) return 2;
  if (run(x, 1, "log(integer)", &worst)) return 2;
  for (double d : denom) {
    x.clear();
    for (int64_t n = 0; n <= max_count; ++n) x.push_back((double)n + 10.0 / d);
    char what[64];
    snprintf(what, sizeof what, "lgamma(integer + 10/%g)", d);
    if (run(x, 0, what, &worst)) return 2;
  }
  printf("U = %.3f\n", worst);
  return 0;
}
