// ArPosteriorSampler::draw (ArPosteriorSampler.cpp:52-143) for one chain, by one (whole) wave: the
// sampler of an ArStateModel in the general structural kernel (ssg_simsmooth.h) and in its template
// (ssm_template_kernel.hip); the spike-and-slab sampler (ar_spike_kernel.hip) borrows the solves.
#pragma once
#include <hip/hip_runtime.h>

#include "ar_trunc_device.h"
#include "device_rng.h"
#include "kalman_params.h"
#include "wave_lanes.h"

namespace boom_amd {

namespace {

// ---- ArPosteriorSampler::draw for one chain, by one (whole) wave.  Vectors sit one
// component per lane (lane i < L), the L x L matrices in LDS at leading dimension
// AR_MAX; every lane reads the same random numbers.
struct ArLds {
  double X[AR_MAX * AR_MAX];    // xtx
  double Lc[AR_MAX * AR_MAX];   // chol(xtx)
  double Lp[AR_MAX * AR_MAX];   // chol(xtx / sigsq)
};
// lower Cholesky factor of `scale` * A (A symmetric, full storage); false: not positive definite
__device__ __forceinline__ bool ar_chol(const double *A, double scale, double *Lc, int L, int lane) {
  for (int j = 0; j < L; ++j) {
    double sacc = 0.0;
    if (lane >= j && lane < L) {
      sacc = A[lane * AR_MAX + j] * scale;
      for (int k = 0; k < j; ++k) sacc -= Lc[lane * AR_MAX + k] * Lc[j * AR_MAX + k];
    }
    const double djj = rl(sacc, j);
    if (!(djj > 0.0)) return false;
    const double d = sqrt(djj);
    if (lane == j) Lc[j * AR_MAX + j] = d;
    else if (lane > j && lane < L) Lc[lane * AR_MAX + j] = sacc / d;
    __builtin_amdgcn_wave_barrier();
  }
  return true;
}
// x: Lc x = b
__device__ __forceinline__ double ar_lsolve(const double *Lc, double b, int L, int lane) {
  double x = 0.0;
  for (int i = 0; i < L; ++i) {
    const double tot = row_total((lane < i) ? Lc[i * AR_MAX + lane] * x : 0.0);
    const double xi = (rl(b, i) - tot) / Lc[i * AR_MAX + i];
    if (lane == i) x = xi;
  }
  return x;
}
// x: Lc' x = b
__device__ __forceinline__ double ar_ltsolve(const double *Lc, double b, int L, int lane) {
  double x = 0.0;
  for (int i = L - 1; i >= 0; --i) {
    const double tot = row_total((lane > i && lane < L) ? Lc[lane * AR_MAX + i] * x : 0.0);
    const double xi = (rl(b, i) - tot) / Lc[i * AR_MAX + i];
    if (lane == i) x = xi;
  }
  return x;
}
// ArModel::check_stationary (ArModel.cpp:142-170).  The quick bound sum |phi| < 1,
// then -- where the reference finds the polynomial's roots (Jenkins-Traub) -- the
// equivalent step-down recursion: every partial autocorrelation inside (-1, 1).
__device__ __forceinline__ bool ar_stationary(double a, int L, int lane) {
  if (row_total((lane < L) ? fabs(a) : 0.0) < 1.0) return true;
  for (int k = L; k >= 1; --k) {
    const double r = rl(a, k - 1);
    if (!(fabs(r) < 1.0)) return false;
    const double den = 1.0 - r * r;
    const int src = k - 2 - lane;
    const double rev = __shfl(a, src < 0 ? 0 : src);
    if (lane < k - 1) a = (a + r * rev) / den;
  }
  return true;
}
// draw_phi (up to three multivariate proposals, else one coefficient at a time) and
// draw_sigma.  suf: the block's sufficient statistics; phi_l: the lane's coefficient
// (in: current, out: drawn); *sigsq likewise.
__device__ __forceinline__ int ar_draw(ArLds &W, const double *suf, int L, double prior_df, double prior_ss,
                                       double sigma_max, SeqRng &rng, double &phi_l, double &sigsq, int lane) {
  for (int e = lane; e < AR_MAX * AR_MAX; e += WAVE) W.X[e] = suf[e];
  const double xty = (lane < L) ? suf[AR_SUF_XTY + lane] : 0.0;
  const double yty = suf[AR_SUF_YTY], n = suf[AR_SUF_N];
  __builtin_amdgcn_wave_barrier();
  if (!ar_chol(W.X, 1.0, W.Lc, L, lane)) return CHAIN_NOT_PD;
  const double phi_hat = ar_ltsolve(W.Lc, ar_lsolve(W.Lc, xty, L, lane), L, lane);
  // rmvn_ivar(phi_hat, xtx / sigsq)
  if (!ar_chol(W.X, 1.0 / sigsq, W.Lp, L, lane)) return CHAIN_NOT_PD;
  bool ok = false;
  for (int attempt = 0; attempt < 3 && !ok; ++attempt) {
    double z = 0.0;
    for (int i = 0; i < L; ++i) {
      const double zi = d_rnorm(rng, 0.0, 1.0);
      if (lane == i) z = zi;
    }
    const double zs = ar_ltsolve(W.Lp, z, L, lane);   // (whole wave: the lanes talk to each other)
    const double cand = (lane < L) ? zs + phi_hat : 0.0;
    ok = ar_stationary(cand, L, lane);
    if (ok) phi_l = cand;
  }
  if (!ok) {
    double ph = phi_l;
    if (!ar_stationary(ph, L, lane)) return CHAIN_RNG_BRANCH;
    for (int i = 0; i < L; ++i) {
      const double initial_phi = rl(ph, i);
      double lo = -1, hi = 1;
      const double ivar = W.X[i * AR_MAX + i];
      const double dot = row_total((lane < L) ? ph * W.X[lane * AR_MAX + i] : 0.0);
      const double mu = (rl(xty, i) - (dot - initial_phi * ivar)) / ivar;
      for (;;) {
        int bad = 0;
        const double candidate = ar_rtrun_norm_2(rng, mu, sqrt(1.0 / ivar), lo, hi, &bad);
        if (bad) return CHAIN_RNG_BRANCH;
        if (lane == i) ph = candidate;
        if (ar_stationary(ph, L, lane)) break;
        if (candidate > initial_phi) hi = candidate; else lo = candidate;
      }
    }
    phi_l = ph;
  }
  // draw_sigma: ss = phi' xtx phi - 2 phi' xty + yty, df = n
  double row = 0.0;
  for (int j = 0; j < L; ++j) {
    const double pj = rl(phi_l, j);
    if (lane < L) row += W.X[lane * AR_MAX + j] * pj;
  }
  const double quad = row_total((lane < L) ? phi_l * row : 0.0);
  const double lin = row_total((lane < L) ? phi_l * xty : 0.0);
  const double ss = quad - 2 * lin + yty;
  int bad = 0;
  sigsq = d_draw_variance(rng, n + prior_df, ss + prior_ss, sigma_max, &bad);
  return bad ? CHAIN_RNG_BRANCH : CHAIN_OK;
}

}  // namespace

}  // namespace boom_amd
