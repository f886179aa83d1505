// Device-side draws of the observation families' forecasts: Student-t, Poisson, binomial.
//
// Like the transforms of device_rng.h they are wave-uniform on a sequential view of a
// stream: every lane of the calling wave reads the same numbers and returns the same draw,
// and a draw is a function of the stream position it starts at alone.
//
//   d_rstudent   rstudent_mt, distributions/student_fix.cpp:60-63, draw for draw: the
//                reference's own two calls (rgamma_mt, rnorm_mt) on the same stream.
//   d_rpois      an exact Poisson sampler, NOT draw-for-draw what Bmath/rpois.cpp makes of a
//   d_rbinom     stream (resp. Bmath/rbinom.cpp): the short exact algorithms
//                  inversion by sequential search on one uniform (small means), and
//                  W. Hoermann (1993), "The transformed rejection method for generating
//                  Poisson random variables", Insurance: Mathematics and Economics 12, 39-45
//                  (PTRS), and W. Hoermann (1993), "The generation of binomial random
//                  variates", J. Statist. Comput. Simul. 46, 101-110 (BTRS)
//                -- no normal approximation at any size.  tests/family_forecast_ref.py restates
//                both in Python on the oracle's uniforms; the tests pin the device on that
//                restatement draw for draw and the restatement on the exact pmf.
//                (probit_kernel.hip has a d_rbinom(SeqRng &, unsigned, double) of its own: the
//                reference's BTPE in the reference's order, for the logit imputer's cell counts.
//                It is file-local, takes the count as an unsigned and is not what a forecast
//                needs, whose trial counts are doubles without that bound.)
//
// LOG-FACTORIALS.  The acceptance tests of PTRS and BTRS compare log(v ...) with the log of a
// ratio of probabilities.  Its log-factorial terms are formed as lgamma(k + 1) of the (large)
// arguments themselves, not as a Stirling form: at lambda = 1e6 the terms k log(lambda) and
// lgamma(k + 1) are about 1.4e7 each and cancel to O(1), so a few ulps of lgamma are about 1e-8
// absolute in the compared value -- the bias this puts on an acceptance probability is of that
// order, and a draw whose comparison comes closer than that is what the tests' margin rule
// sets aside.  (At lambda = 1e12 the terms are about 2.7e13 and the error about 1e-2 in the
// exponent of a test that only the few percent of candidates outside the squeeze reach.)
//
// LOOP CAPS.  The search of an inversion ends at RCOUNT_SEARCH_CAP (Poisson; the mean is below 10,
// the mass beyond 128 is below 1e-90) or at k = n (binomial), and before that as soon as the next
// term no longer moves the accumulated sum (u lies in the rounding of the total mass: the tail).
// A rejection loop runs at most RCOUNT_REJECT_CAP rounds (an acceptance takes 1.1 - 1.3 rounds on
// average; every round accepts with probability > 0.7) and then returns NaN.
#pragma once
#include "device_rng.h"

namespace boom_amd {

enum { RCOUNT_SEARCH_CAP = 128, RCOUNT_REJECT_CAP = 256 };

// rstudent_mt(rng, mu, sigma, nu): w ~ Gamma(nu / 2, rate nu / 2), then rnorm_mt(mu, sigma / sqrt(w)).
// (rgamma_mt takes the scale 1 / rate; *bad as d_rgamma_scale: nu < 0.6 and 1000 rejections.)
template <class R>
__device__ __forceinline__ double d_rstudent(R &rng, double mu, double sigma, double nu, int *bad) {
  const double w = d_rgamma_scale(rng, nu / 2.0, 1.0 / (nu / 2.0), bad);
  return d_rnorm(rng, mu, sigma / sqrt(w));
}

// Poisson(lambda), an integer-valued double.  lambda = 0: 0 without reading the stream; a
// negative, infinite or NaN lambda: NaN without reading the stream.
template <class R>
__device__ __forceinline__ double d_rpois(R &rng, double lambda) {
  if (!(lambda >= 0.0) || isinf(lambda)) return __builtin_nan("");
  if (lambda == 0.0) return 0.0;
  if (lambda < 10.0) {
    // inversion: the first k with u <= p_0 + ... + p_k, p_{k+1} = p_k lambda / (k + 1)
    const double u = rng();
    double pk = exp(-lambda), cdf = pk;
    int k = 0;
    while (u > cdf && k < RCOUNT_SEARCH_CAP) {
      ++k;
      pk *= lambda / (double)k;
      const double next = cdf + pk;
      if (next == cdf) break;
      cdf = next;
    }
    return (double)k;
  }
  // PTRS
  const double slam = sqrt(lambda), loglam = log(lambda);
  const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
  const double inv_alpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
  for (int round = 0; round < RCOUNT_REJECT_CAP; ++round) {
    const double u = rng() - 0.5, v = rng();
    const double us = 0.5 - fabs(u);
    const double k = floor((2.0 * a / us + b) * u + lambda + 0.43);
    if (us >= 0.07 && v <= vr) return k;
    if (k < 0.0 || (us < 0.013 && v > us)) continue;
    if (log(v) + log(inv_alpha) - log(a / (us * us) + b) <= -lambda + k * loglam - lgamma(k + 1.0)) return k;
  }
  return __builtin_nan("");
}

// Binomial(n, p), n a non-negative integer held in a double; an integer-valued double.  n = 0,
// p = 0, p = 1: 0, 0, n without reading the stream; a NaN or out-of-range p, a negative, infinite
// or NaN n: NaN without reading the stream.  The draw is made at q = min(p, 1 - p) and mirrored.
template <class R>
__device__ __forceinline__ double d_rbinom(R &rng, double n, double p) {
  if (!(p >= 0.0 && p <= 1.0) || !(n >= 0.0) || isinf(n)) return __builtin_nan("");
  if (n == 0.0 || p == 0.0) return 0.0;
  if (p == 1.0) return n;
  const bool mirror = p > 0.5;
  const double q = mirror ? 1.0 - p : p;
  double k = 0.0;
  if (n * q < 10.0) {
    // inversion: p_0 = (1 - q)^n, p_{k+1} = p_k (n - k) / (k + 1) q / (1 - q); ends at k = n
    const double u = rng();
    const double odds = q / (1.0 - q);
    double pk = exp(n * log1p(-q)), cdf = pk;
    while (u > cdf && k < n) {
      pk *= odds * ((n - k) / (k + 1.0));
      k += 1.0;
      const double next = cdf + pk;
      if (next == cdf) break;
      cdf = next;
    }
  } else {
    // BTRS
    const double spq = sqrt(n * q * (1.0 - q));
    const double b = 1.15 + 2.53 * spq, a = -0.0873 + 0.0248 * b + 0.01 * q, c = n * q + 0.5;
    const double vr = 0.92 - 4.2 / b, alpha = (2.83 + 5.1 / b) * spq;
    const double m = floor((n + 1.0) * q), lodds = log(q / (1.0 - q));
    const double h = lgamma(m + 1.0) + lgamma(n - m + 1.0);
    bool done = false;
    for (int round = 0; round < RCOUNT_REJECT_CAP && !done; ++round) {
      const double u = rng() - 0.5, v = rng();
      const double us = 0.5 - fabs(u);
      k = floor((2.0 * a / us + b) * u + c);
      if (k < 0.0 || k > n) continue;
      if (us >= 0.07 && v <= vr) { done = true; continue; }
      if (log(v * alpha / (a / (us * us) + b)) <= (h - lgamma(k + 1.0) - lgamma(n - k + 1.0)) + (k - m) * lodds) done = true;
    }
    if (!done) return __builtin_nan("");
  }
  return mirror ? n - k : k;
}

}  // namespace boom_amd
