// The general structural state-space kernel's launchers and the forecast kernel.  The kernel itself --
// the state half of StateSpacePosteriorSampler::draw() for any list of state models -- is the template
// of ssg_simsmooth.h; this file makes its plain and H_t instances (launch_ssg_plain, launch_ssg_ht).
#include "ssg_simsmooth.h"

namespace boom_amd {

// StateSpaceRegressionModel::simulate_forecast for every chain's current draw of the
// structural model (StateSpaceRegressionModel.cpp:216-219, :256-278): the state
// advances by T state + state errors (model by model), the observation is
// rnorm(Z'state, sigma_obs) + x'beta; normals in the reference's order on the
// chain's forecast stream (id 5).  One wavefront per chain, lane = state component
// (logical order; the horizon is short, a seasonal block simply shifts).  As the
// reference (advance_to_timestamp, StateSpaceModelBase.cpp:455-459) forecast step i
// uses the transition matrix and state errors of time T - 2 + i.  The state's step is
// ssg_forecast_step (ssg_forecast_device.h), which the observation families' forecast kernel
// (ss_family_forecast_kernel.hip) runs too.  The list's regression holiday models (R.nmodels; none: 0) add
// their coefficient active at time T + i to the forecast, model by model: (obs + pred) + effect.
__global__ __launch_bounds__(64) void ssg_forecast_kernel(SsParams P, RhParams R, int horizon, const double *newX,
                                                          uint64_t *pos_forecast, double *out) {
  const int chain = (int)blockIdx.x + P.chain_first, lane = threadIdx.x;
  if ((int)blockIdx.x >= P.chain_count) return;
  if (P.status[chain] != CHAIN_OK) return;
  const SsmParams &M = P.ssm;
  const SsgSpec &Q = *M.spec;
  const int T = P.T, p = P.p, m = M.m;
  const double *beta = P.beta + (size_t)chain * p;
  const double sd_obs = sqrt(P.sigsq[chain]);
  const double *gst = M.work + (size_t)chain * M.work_stride + (size_t)m * T;
  double st = (lane < m) ? gst[(size_t)(T - 1) * m + lane] : 0.0;
  SeqRng rng{PhiloxKey{P.seed_lo, P.seed_hi, (uint32_t)(P.chain_offset + chain), 5u}, pos_forecast[chain]};
  for (int i = 0; i < horizon; ++i) {
    // (the transition's index is T - 2 + i)
    const double zs = ssg_forecast_step(M, Q, chain, lane, T - 2 + i, rng, st, P.cal, P.dyn, P.dyn_cols);
    const double obs = d_rnorm(rng, zs, sd_obs);
    double part = 0.0;
    for (int j = lane; j < p; j += WAVE) part += newX[(size_t)j * horizon + i] * beta[j];
    const double pred = wsum<false>(part);
    double fc = obs + pred;
    for (int k = 0; k < R.nmodels; ++k) {
      const int j = R.table[(size_t)(T + i) * RH_MAX_MODELS + k];
      if (j >= 0) fc = fc + R.coef[(size_t)chain * RH_MAX_COEF + j];
    }
    if (lane == 0) out[(size_t)chain * horizon + i] = fc;
  }
  if (lane == 0) pos_forecast[chain] = rng.pos;
}

hipError_t launch_ssm_forecast(hipStream_t stream, const SsParams &P, const RhParams &R, int horizon, const double *newX,
                               uint64_t *pos_forecast, double *out) {
  hipLaunchKernelGGL(ssg_forecast_kernel, dim3(P.chain_count), dim3(WAVE), 0, stream, P, R, horizon, newX,
                     pos_forecast, out);
  return hipGetLastError();
}

size_t ssm_dynamic_lds(const SsmParams &M) {
  size_t need = (size_t)ssg_pass_lds_doubles(M.m, M.ld, M.bl, M.nerr, M.nar, M.ndyn) * sizeof(double);
  if (need < sizeof(NormalsLds)) need = sizeof(NormalsLds);
  if (need < sizeof(ArLds)) need = sizeof(ArLds);
  return (need + 15) & ~(size_t)15;
}

hipError_t launch_ssm_template(hipStream_t stream, const SsParams &P, int draw_variances);

hipError_t launch_ssg_plain(hipStream_t stream, const SsParams &P, int draw_variances, size_t lds) { return ssg_launch_variant<SSG_V_PLAIN>(stream, P, draw_variances, lds); }
hipError_t launch_ssg_ht(hipStream_t stream, const SsParams &P, int draw_variances, size_t lds) { return ssg_launch_variant<SSG_V_HT>(stream, P, draw_variances, lds); }

hipError_t launch_ssm_simsmooth(hipStream_t stream, const SsParams &P, int draw_variances) {
  const size_t lds = ssm_dynamic_lds(P.ssm);
  const SsgChoice choice = ssg_choose_kernel(P);   // (ssg_instances.h: nothing else decides)
  if (choice.kernel == SSG_CHOICE_INVALID) return hipErrorInvalidValue;
  hipError_t err = hipErrorInvalidValue;
  {
    KtScope kt(stream, KT_SSM);
    if (choice.kernel == SSG_CHOICE_TEMPLATE) err = launch_ssm_template(stream, P, draw_variances);
    else switch (choice.variant) {
      case SSG_V_DR: err = launch_ssg_dr(stream, P, draw_variances, lds); break;
      case SSG_V_HD: err = launch_ssg_hd(stream, P, draw_variances, lds); break;
      case SSG_V_QT: err = launch_ssg_qt(stream, P, draw_variances, lds); break;
      case SSG_V_HT: err = launch_ssg_ht(stream, P, draw_variances, lds); break;
      case SSG_V_PLAIN: err = launch_ssg_plain(stream, P, draw_variances, lds); break;
    }
    if (err != hipSuccess) return err;
    err = hipGetLastError();
  }
  if (err != hipSuccess) return err;
  if (P.h) return hipSuccess;   // (the Student family builds X'W(y - Z alpha) itself, student_kernel.hip)
  // xty[chain, j] = x_j' e_chain (the residual series are array 1 of every chain's scratch block)
  return launch_xte_tiled(stream, P.scratch + (size_t)P.chain_first * P.scratch_stride + P.T, P.scratch_stride,
                          P.chain_count, P.X, (int64_t)P.T, P.p, P.xty + (size_t)P.chain_first * P.p,
                          P.xte_planes);
}

}  // namespace boom_amd
