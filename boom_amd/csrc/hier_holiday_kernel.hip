// HierarchicalRegressionHolidayStateModel (bsts AddHierarchicalRegressionHoliday) for many chains.  To the
// state space model it is the plain regression holiday (reg_holiday_kernel.hip): a constant state, an
// offset on the chain's series, observe_state's totals per coefficient.  What is its own is the sampler,
// HierGaussianRegressionAsisSampler::draw: with the sigma^2 just drawn, the totals s_h and counts n_h of
// the last state draw (the regression sufficient statistics of holiday h are xtx = diag(n_h), xty = s_h)
// and the chain's current mu and Omega,
//   1  beta_h ~ N(A^-1 b, A^-1), A = diag(n_h) / sigma^2 + Omega, b = s_h / sigma^2 + Omega mu, h = 0 .. H - 1
//   2  (a) mu' ~ N(I^-1 (H Omega betabar + Sigma0^-1 mu0), I^-1), I = H Omega + Sigma0^-1
//      (b) a Wishart draw whose result step 3 overwrites unread: its numbers are consumed
//   3  c_h = beta_h - mu';  mu ~ N(A^-1 b, A^-1), A = sum_h diag(n_h) / sigma^2 + Sigma0^-1,
//      b = sum_h (s_h - n_h c_h) / sigma^2 + Sigma0^-1 mu0;  Omega ~ Wishart(nu0 + H, (sum_h c_h c_h' + S0)^-1)
// in this order of random numbers (mvn_wishart_device.h: rhh_draw_model).  All hierarchical models of a
// chain read one position of the chain's stream RHH_STREAM, in (model, step) order -- a convention of ours:
// the reference draws from the sampler's generator and, in 2 (a), the global one.
//
// rhh_draw_kernel: one wavefront per chain, launched ahead of rh_draw_kernel (which passes the hierarchical
// models' coefficients by and writes the chains' series from all of them).  A draw that fails sets
// RHH_BAD_DRAW and leaves the chain's coefficients, mu, Omega and stream position as they were.
#include <hip/hip_runtime.h>

#include "ktimer.h"

#include "mvn_wishart_device.h"

namespace boom_amd {

__global__ __launch_bounds__(64) void rhh_draw_kernel(SsParams P, RhParams R, RhhParams Q) {
  const int chain = (int)blockIdx.x + P.chain_first, lane = (int)threadIdx.x;
  if ((int)blockIdx.x >= P.chain_count) return;
  if (P.status[chain] != CHAIN_OK) return;
  if (P.only_ran && P.only_ran[chain] == 0) return;
  __shared__ MwLds W;
  const double sigsq = P.sigsq[chain];
  double *coef = R.coef + (size_t)chain * RH_MAX_COEF;
  const double *tot = R.totals + (size_t)chain * RH_MAX_COEF;
  double *mu = Q.mu + (size_t)chain * RH_MAX_MODELS * RHH_MAX_WIDTH;
  double *om = Q.omega + (size_t)chain * RH_MAX_MODELS * RHH_MAX_WIDTH * RHH_MAX_WIDTH;
  SeqRng rng{PhiloxKey{P.seed_lo, P.seed_hi, (uint32_t)(P.chain_offset + chain), RHH_STREAM}, Q.pos[chain]};
  bool ok = true;
  for (int k = 0; k < Q.nmodels; ++k) {
    if (Q.width[k] <= 0 || !ok) continue;
    ok = rhh_draw_model(W, rng, lane, Q.width[k], Q.nhol[k], R.first[k], sigsq, Q.nu0[k], R.counts, tot,
                        mu + k * RHH_MAX_WIDTH, om + k * RHH_MAX_WIDTH * RHH_MAX_WIDTH,
                        Q.hyper + (size_t)k * RHH_HYPER_STRIDE, W.mu_out[k], W.om_out[k]);
  }
  if (!ok) {
    if (lane == 0) P.status[chain] = RHH_BAD_DRAW;
    return;
  }
  for (int k = 0; k < Q.nmodels; ++k) {
    const int d = Q.width[k];
    if (d <= 0) continue;
    for (int j = R.first[k] + lane; j < R.first[k + 1]; j += WAVE) coef[j] = W.beta[j];
    if (lane < d) mu[k * RHH_MAX_WIDTH + lane] = W.mu_out[k][lane];
    for (int i = lane; i < d * d; i += WAVE) {
      const int at = (i / d) * RHH_MAX_WIDTH + i % d;
      om[k * RHH_MAX_WIDTH * RHH_MAX_WIDTH + at] = W.om_out[k][at];
    }
  }
  if (lane == 0) Q.pos[chain] = rng.pos;
}

hipError_t launch_rhh_draw(hipStream_t stream, const SsParams &P, const RhParams &R, const RhhParams &Q) {
  KtScope kt(stream, KT_SS_REGHOLIDAY);
  hipLaunchKernelGGL(rhh_draw_kernel, dim3((unsigned)P.chain_count), dim3(WAVE), 0, stream, P, R, Q);
  return hipGetLastError();
}

}  // namespace boom_amd
