// pgm_ibeta.h — the p-value behind pgm_lgs_pcorr: I_x(a, 1/2), the regularised incomplete beta function
// with second parameter 1/2, as one __host__ __device__ inline function so that a host program or test can
// run the very code the kernel runs (as pgm_igamc.h).  fp64 throughout.
//
// With r the (partial) correlation of n rows, 2 Beta(n/2 - 1, n/2 - 1).sf(|r|) on [-1, 1] (scipy's
// pearsonr) equals I_{1 - r^2}((n - 2) / 2, 1 / 2), the two-sided Student t with n - 2 degrees of freedom.
// The argument is handed over as y = r^2 = 1 - x: for a p-value that matters x is close to 1 and 1 - r^2
// formed first would lose the digits of r^2.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define PGM_HD __host__ __device__
#else
#ifndef PGM_HD
#define PGM_HD
#endif
#endif

// steps of the continued fraction at which the loop gives up (below)
#define PGM_IBETA_MAX_STEPS 200000

// log(Gamma(a + 1/2) / Gamma(a)).  The difference of two lgamma values of size a log a loses a log a
// ulps, 1e-9 of the p-value at a = 5e5; from a = 32 on the Stirling series of the quotient is used
// instead (its first omitted term, 31 / (18432 a^9) < 5e-17 there, is below half an ulp of the result).
PGM_HD inline double pgm_lgamma_half_ratio(double a) {
  if (a < 32.0) return std::lgamma(a + 0.5) - std::lgamma(a);
  const double r = 1.0 / a, r2 = r * r;
  return 0.5 * std::log(a) - r * (0.125 - r2 * (1.0 / 192.0 - r2 * (1.0 / 640.0 - r2 * (17.0 / 14336.0))));
}

// The continued fraction of the incomplete beta function (modified Lentz): I_x(a, b) = front * cf / a for
// x < (a + 1) / (a + b + 2).  It converges in O(sqrt(max(a, b))) + O(10) steps; at PGM_IBETA_MAX_STEPS
// (enough for a, b ~ 1e9) the loop ends and the value reached so far is returned.
//
// Accuracy.  The fraction's value is a sensitive function of x when a is large and x is next to 1: with S =
// |d log cf / d log x| = |front / ((1 - x) I) - a + x / (2 (1 - x))| (b = 1/2), up to a few tenths of a, the u of
// every coefficient's roundings (x multiplies each of them) comes back as about 8 S u in the result: 1e-15 for a
// up to 100, 1e-11 of the p-value at a = 5e5 (n = 10^6 rows), 1e-9 at a = 5e7.  The digits a test decision or a
// ranking of p-values needs are not among those; tests/lgs_cases.py ibeta_rel states the bound the tests hold it to.
PGM_HD inline double pgm_ibeta_cf(double a, double b, double x) {
  const double tiny = 1e-300;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (std::fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= PGM_IBETA_MAX_STEPS; ++m) {
    const double m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (std::fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (std::fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (std::fabs(del - 1.0) < 2e-16) break;
  }
  return h;
}

// I_{1 - y}(a, 1/2) for a > 0 and y in [0, 1]; NaN for any other argument (NaN included).  The prefactor
// (1 - y)^a sqrt(y) Gamma(a + 1/2) / (Gamma(a) sqrt(pi)) is formed in the log domain with log1p(-y), so
// its relative error is a few ulps of the exponent a |log(1 - y)|, which is below 750 for any result
// above the smallest normal number.  x = 1 - y below the mean (a + 1) / (a + 5/2): the fraction in (a, 1/2)
// at x; otherwise 1 minus the fraction in (1/2, a) at y, where the result is above 0.15 and the
// subtraction keeps its relative precision.
PGM_HD inline double pgm_ibeta_half(double a, double y) {
  if (!(a > 0.0) || !(y >= 0.0) || !(y <= 1.0)) return NAN;
  if (y == 0.0) return 1.0;
  if (y == 1.0) return 0.0;
  const double x = 1.0 - y;
  const double front = std::exp(a * std::log1p(-y) + 0.5 * std::log(y) + pgm_lgamma_half_ratio(a)) * 0.56418958354775628695;
  if (x < (a + 1.0) / (a + 2.5)) return front * pgm_ibeta_cf(a, 0.5, x) / a;
  return 1.0 - front * pgm_ibeta_cf(0.5, a, y) * 2.0;
}

// The two-sided p-value of a correlation coefficient r over n rows (n > 2).
PGM_HD inline double pgm_pearson_p(double r, double n) { return pgm_ibeta_half(0.5 * (n - 2.0), r * r); }
