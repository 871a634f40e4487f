// pgm_igamc.h — the chi-square survival function behind pgm_fit_citest: Q(a, x), the regularised upper
// incomplete gamma function, as one __host__ __device__ inline function so that a host program can test
// the very code the kernel runs (tools/ci_selftest.cpp).  fp64 throughout.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define PGM_HD __host__ __device__
#else
#define PGM_HD
#endif

// Q(a, x) = Gamma(a, x) / Gamma(a) for a > 0, x >= 0 (1 for x < 0).  Both branches share the prefactor
// x^a e^-x / Gamma(a), formed in the log domain.  x < a + 1: the series of the lower function,
// P = prefactor * sum_n x^n / (a (a + 1) ... (a + n)), Q = 1 - P (there Q > 0.08, so the subtraction
// keeps its relative precision); otherwise the continued fraction of the upper function by the
// modified Lentz method.  Both converge in O(sqrt(a)) + O(10) steps near x = a, faster elsewhere; the
// caps are far above what a <= 2^31 needs and only bound the loop.
PGM_HD inline double pgm_igamc(double a, double x) {
  if (!(a > 0.0) || x != x) return NAN;  // NaN arguments too
  // x < 0: a statistic that is 0 up to rounding (lambda != 1 adds terms of both signs), as scipy's chi2.sf
  if (x <= 0.0) return 1.0;
  if (std::isinf(x)) return 0.0;
  const double lead = a * std::log(x) - x - std::lgamma(a);
  if (x < a + 1.0) {
    double term = 1.0 / a, sum = term, ap = a;
    for (int n = 0; n < 1000000; ++n) {
      ap += 1.0;
      term *= x / ap;
      sum += term;
      if (term < sum * 1e-17) break;
    }
    return 1.0 - std::exp(lead) * sum;
  }
  const double tiny = 1e-300;
  double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
  for (int i = 1; i < 1000000; ++i) {
    const double an = -(double)i * ((double)i - a);
    b += 2.0;
    d = an * d + b;
    if (std::fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (std::fabs(del - 1.0) < 1e-16) break;
  }
  return std::exp(lead) * h;
}

// The p-value of a chi-square statistic with `dof` degrees of freedom.  dof = 0 is the caller's case.
PGM_HD inline double pgm_chi2_sf(double stat, double dof) { return pgm_igamc(0.5 * dof, 0.5 * stat); }
