// The two-sided truncated normal of the autoregression samplers (rtrun_norm_2_mt and its
// Tn2Sampler): one definition for the kernels that draw AR coefficients one at a time
// (ar_sampler_device.h: ar_draw; ssg_device.h: the semilocal slope) and for the test probe that calls it directly.
#pragma once
#include <hip/hip_runtime.h>

#include "device_rng.h"

namespace boom_amd {

// Tn2Sampler (distributions/Tn2Sampler.cpp:25-131): adaptive rejection sampling of a
// standard normal on [lo, hi] under the hull of tangents at the points x (logf =
// -x^2/2).  As in d_ars_gamma_tail the hull lives across the wave: lane i holds
// point i (abscissa, log density, slope, cdf) and knot i; lane n holds the last knot,
// so up to 63 points.  Every lane of the wave must be active.  Restated as written,
// update_cdf's increment (exp(y - y0) / d) * expm1(d * knots[k + 1] - knots[k]) included.
__device__ __forceinline__ double ar_tn2_draw(SeqRng &rng, double lo, double hi, int *bad) {
  const int lane = (int)(threadIdx.x & 63);
  int n = 2;
  double xs = (lane == 0) ? lo : hi;   // (lanes past n - 1 hold copies of the last point)
  double ys = -.5 * xs * xs, ds = -xs, kn = 0.0, cdf = 0.0;
  for (int level = 0; level <= 1001; ++level) {
    // refresh_knots: knots[0] = x[0], knots[n] = x[n - 1], compute_knot in between
    {
      const double x1 = __shfl_up(xs, 1), y1 = __shfl_up(ys, 1), d1 = __shfl_up(ds, 1);
      double ans = (y1 - d1 * x1) - (ys - ds * xs);
      ans /= (ds - d1);
      kn = (lane == 0) ? xs : ((lane >= n) ? x1 : ans);
    }
    // update_cdf
    {
      const double y0 = ars_lane(ys, 0);
      const double knext = __shfl_down(kn, 1);
      const double y = ys + ds * (kn - xs);
      const double inc = (fabs(ds) < .00000000001) ? exp(y - y0) * (knext - kn)
                                                  : (exp(y - y0) / ds) * expm1(ds * knext - kn);
      double last = 0.0;
      for (int k = 0; k < n; ++k) {
        const double ik = ars_lane(inc, k);
        last = (k == 0) ? ik : last + ik;
        if (lane == k) cdf = last;
      }
    }
    const double u = d_runif(rng, 0.0, ars_lane(cdf, n - 1));
    const int k = ars_lower_bound(cdf, n, u);
    if (k >= n) break;   // (past the end of cdf in the reference)
    const double klo = ars_lane(kn, k), khi = ars_lane(kn, k + 1);
    const double dk = ars_lane(ds, k);
    const double lam = -1 * dk;
    double cand;
    if (lam == 0 || fabs(khi - klo) < 1.4901161193847656e-08) cand = d_runif(rng, klo, khi);   // sqrt(epsilon)
    else cand = d_rtrun_exp(rng, lam, klo, khi);
    const double target = -.5 * cand * cand;
    const double logu = (ars_lane(ys, k) + dk * (cand - ars_lane(xs, k))) - d_rexp(rng, 1.0);
    if (logu < target) return cand;
    // add_point (an error in the reference when the candidate left [x[0], x.back()])
    if (cand > ars_lane(xs, n - 1) || cand < ars_lane(xs, 0) || n >= 63) break;
    const int pos = ars_lower_bound(xs, n, cand);
    {
      const double xu = __shfl_up(xs, 1), yu = __shfl_up(ys, 1), du = __shfl_up(ds, 1);
      if (lane > pos) { xs = xu; ys = yu; ds = du; }
      if (lane == pos) { xs = cand; ys = target; ds = -cand; }
    }
    ++n;
  }
  *bad = 1;
  return 0.0;
}
// rtrun_norm_2_mt (trun_norm.cpp:273-325), lo and hi finite: the two rejection samplers
// of lo < mu < hi, the Tn2Sampler in the tails
__device__ __forceinline__ double ar_rtrun_norm_2(SeqRng &rng, double mu, double sigma, double lo, double hi,
                                                  int *bad) {
  if (lo < mu && hi > mu) {
    if ((hi - lo) / sigma > .5) {
      double y = lo - 1;
      while (y < lo || y > hi) y = d_rnorm(rng, mu, sigma);
      return y;
    }
    const double ln_sqrt_2pi = 0.918938533204672741780329736406;
    const double phi_mu = -(ln_sqrt_2pi + 0.5 * 0.0 * 0.0 + log(sigma));
    double phi = phi_mu, u = phi + 1, y = 0;
    while (u > phi) {
      y = d_runif(rng, lo, hi);
      const double x = (y - mu) / sigma;
      phi = -(ln_sqrt_2pi + 0.5 * x * x + log(sigma));
      u = phi_mu - d_rexp(rng, 1.0);
    }
    return y;
  }
  hi = (hi - mu) / sigma;
  lo = (lo - mu) / sigma;
  if (hi < 0) {
    // (the reference recurses with (0, 1, -hi, -lo), which lands in its Tn2Sampler)
    const double y = ar_tn2_draw(rng, -hi, -lo, bad);
    return mu - sigma * y;
  }
  const double y = ar_tn2_draw(rng, lo, hi, bad);
  return y * sigma + mu;
}

}  // namespace boom_amd
