// simulate_forecast of the observation families of the structural model, for every chain's
// current draw (simulate_multiplex_forecast with consecutive timestamps):
//   Student-t   StateSpaceStudentRegressionModel.cpp:233-251   rstudent_mt(eta, sigma, nu)
//   Poisson     StateSpacePoissonModel.cpp:223-242             rpois_mt(exposure_i exp(eta))
//   logit       StateSpaceLogitModel.cpp:229-248               rbinom_mt(lround(trials_i), plogis(eta))
// with eta = Z'state + x_i'beta.  The state advances as in the Gaussian forecast
// (ssg_forecast_step, ssg_forecast_device.h); the draw order is the reference's: the state
// errors of the step, then the observation, on the chain's forecast stream (id 5) from the
// position the engine keeps across calls.  The Student draw is the reference's own on that
// stream; the count draws are exact samplers of our own (device_rng_counts.h), so the counts
// have the reference's distribution, not its numbers.
//
// One wavefront per chain, lane = state component.  A translation unit of its own: the
// instances of ssm_kernel.hip are not touched by what the samplers need.
#include <hip/hip_runtime.h>

#include "device_rng.h"
#include "device_rng_counts.h"
#include "kalman_params.h"
#include "ssg_forecast_device.h"

namespace boom_amd {

// plogis: 1 / (1 + exp(-eta)) is exactly 0 (exp overflows to +inf) or 1 (exp underflows to 0)
// at large |eta|, never NaN for a number
__device__ __forceinline__ double d_plogis(double eta) { return 1.0 / (1.0 + exp(-eta)); }

// FAMILY: SS_FORECAST_STUDENT / _POISSON / _LOGIT.  scale: the horizon's exposures (Poisson) or
// trial counts, already rounded (logit); nu: every chain's degrees of freedom (Student).
template <int FAMILY>
__global__ __launch_bounds__(64) void ssf_forecast_kernel(SsParams P, int horizon, const double *newX,
                                                          const double *scale, const double *nu,
                                                          uint64_t *pos_forecast, double *out) {
  const int chain = (int)blockIdx.x + P.chain_first, lane = threadIdx.x;
  if ((int)blockIdx.x >= P.chain_count) return;
  if (P.status[chain] != CHAIN_OK) return;
  const SsmParams &M = P.ssm;
  const SsgSpec &Q = *M.spec;
  const int T = P.T, p = P.p, m = M.m;
  const double *beta = P.beta + (size_t)chain * p;
  const double *gst = M.work + (size_t)chain * M.work_stride + (size_t)m * T;
  double st = (lane < m) ? gst[(size_t)(T - 1) * m + lane] : 0.0;
  double sd_obs = 0.0, df = 0.0;
  if (FAMILY == SS_FORECAST_STUDENT) {
    sd_obs = sqrt(P.sigsq[chain]);
    df = nu[chain];
  }
  SeqRng rng{PhiloxKey{P.seed_lo, P.seed_hi, (uint32_t)(P.chain_offset + chain), 5u}, pos_forecast[chain]};
  for (int i = 0; i < horizon; ++i) {
    const double zs = ssg_forecast_step(M, Q, chain, lane, T - 2 + i, rng, st);
    double part = 0.0;
    for (int j = lane; j < p; j += WAVE) part += newX[(size_t)j * horizon + i] * beta[j];
    const double eta = zs + wsum<false>(part);
    double obs;
    if (FAMILY == SS_FORECAST_STUDENT) {
      int bad = 0;
      obs = d_rstudent(rng, eta, sd_obs, df, &bad);
      if (bad) obs = __builtin_nan("");
    } else if (FAMILY == SS_FORECAST_POISSON) {
      obs = d_rpois(rng, scale[i] * exp(eta));
    } else {
      obs = d_rbinom(rng, scale[i], d_plogis(eta));
    }
    if (lane == 0) out[(size_t)chain * horizon + i] = obs;
  }
  if (lane == 0) pos_forecast[chain] = rng.pos;
}

hipError_t launch_ss_family_forecast(hipStream_t stream, const SsParams &P, int family, int horizon,
                                     const double *newX, const double *scale, const double *nu,
                                     uint64_t *pos_forecast, double *out) {
  const dim3 grid(P.chain_count), block(WAVE);
  switch (family) {
    case SS_FORECAST_STUDENT:
      hipLaunchKernelGGL(ssf_forecast_kernel<SS_FORECAST_STUDENT>, grid, block, 0, stream, P, horizon, newX, scale,
                         nu, pos_forecast, out);
      break;
    case SS_FORECAST_POISSON:
      hipLaunchKernelGGL(ssf_forecast_kernel<SS_FORECAST_POISSON>, grid, block, 0, stream, P, horizon, newX, scale,
                         nu, pos_forecast, out);
      break;
    case SS_FORECAST_LOGIT:
      hipLaunchKernelGGL(ssf_forecast_kernel<SS_FORECAST_LOGIT>, grid, block, 0, stream, P, horizon, newX, scale, nu,
                         pos_forecast, out);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace boom_amd
