// RegressionHolidayStateModel (bsts AddRegressionHoliday) for many chains.  The model's state is the
// constant 1 with variance 0 and its Z_t is the coefficient of the holiday and day active at t, so to the
// structural kernels it is an offset on the observation series and nothing else: a list with such models
// runs on every chain's own series y_c[t] = (..((y[t] - effect of model 0) - effect of model 1) ..)
// (SsParams::y with y_stride = T), and the state draw is the draw of the list without them on that series.
// This file holds what is left of the model:
//   rh_draw_kernel     sample_posterior (StateModels/RegressionHolidayStateModel.cpp:161-182): every
//                      coefficient, in (model, coefficient) order, one rnorm each from the chain's stream
//                      RH_COEF_STREAM -- a convention of ours: the reference draws from the model's own
//                      generator --, with the chain's sigma^2, the shared counts and the totals the last
//                      state draw left; then (draw or not) the active steps of the chain's series are
//                      written from the coefficients, so the series is never stale after a setter.
//                      Launched ahead of the state kernel.
//   rh_observe_kernel  ScalarRegressionHolidayStateModel::observe_state (:213-224) over the series: at
//                      every observed active step r = (sres[t] - x_t'beta) + coefficient, summed per
//                      coefficient in time order.  sres is the residual series the state kernel left
//                      (y_c - Z'alpha: every model's effect is off already), beta the chain's current one.
//                      Launched behind the state kernel.
//   rh_fill_kernel     y_c = y for every chain: once per change of the data or a calendar (the steps that
//                      are active no more).
// One wavefront per chain; the coefficients and the totals of a chain sit in LDS (RH_MAX_COEF doubles each).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ktimer.h"

#include "device_rng.h"
#include "kalman_params.h"
#include "ssg_device.h"

namespace boom_amd {

// hier: bit k set where model k is hierarchical -- rhh_draw_kernel (hier_holiday_kernel.hip, launched just
// before) has drawn its coefficients, which are read here as a setter's are
__global__ __launch_bounds__(64) void rh_draw_kernel(SsParams P, RhParams R, int draw, int hier) {
  const int chain = (int)blockIdx.x + P.chain_first, lane = (int)threadIdx.x;
  if ((int)blockIdx.x >= P.chain_count) return;
  if (P.status[chain] != CHAIN_OK) return;
  if (P.only_ran && P.only_ran[chain] == 0) return;
  __shared__ double s_coef[RH_MAX_COEF];
  const int n = R.ncoef, T = P.T;
  double *coef = R.coef + (size_t)chain * RH_MAX_COEF;
  if (draw) {
    // every lane reads the same numbers; lane 0 keeps the draws
    const double sigsq = P.sigsq[chain];
    const double *tot = R.totals + (size_t)chain * RH_MAX_COEF;
    SeqRng rng{PhiloxKey{P.seed_lo, P.seed_hi, (uint32_t)(P.chain_offset + chain), RH_COEF_STREAM}, R.pos[chain]};
    bool bad = false;
    for (int k = 0; k < R.nmodels; ++k) {
      const double mu = R.prior_mean[k], tausq = R.prior_sd[k] * R.prior_sd[k];
      if ((hier >> k) & 1) {
        for (int j = R.first[k] + lane; j < R.first[k + 1]; j += WAVE) s_coef[j] = coef[j];
        continue;
      }
      for (int j = R.first[k]; j < R.first[k + 1]; ++j) {
        const double precision = R.counts[j] / sigsq + 1.0 / tausq;
        double mean = tot[j] / sigsq + mu / tausq;
        mean /= precision;
        const double sd = sqrt(1.0 / precision);
        const double v = d_rnorm(rng, mean, sd);
        bad = bad || !isfinite(v);
        if (lane == 0) s_coef[j] = v;
      }
    }
    if (bad) {
      if (lane == 0) P.status[chain] = RH_BAD_DRAW;
      return;
    }
    wave_lds_sync();
    for (int j = lane; j < n; j += WAVE) coef[j] = s_coef[j];
    if (lane == 0) R.pos[chain] = rng.pos;
  } else {
    for (int j = lane; j < n; j += WAVE) s_coef[j] = coef[j];
    wave_lds_sync();
  }
  // the chain's series at the active steps: the effects come off in model order
  double *ys = R.y + (size_t)chain * T;
  for (int i = lane; i < R.nsteps; i += WAVE) {
    const int t = R.steps[i];
    double v = R.y_shared[t];
    for (int k = 0; k < R.nmodels; ++k) {
      const int j = R.table[(size_t)t * RH_MAX_MODELS + k];
      if (j >= 0) v = v - s_coef[j];
    }
    ys[t] = v;
  }
}

__global__ __launch_bounds__(64) void rh_observe_kernel(SsParams P, RhParams R) {
  const int chain = (int)blockIdx.x + P.chain_first, lane = (int)threadIdx.x;
  if ((int)blockIdx.x >= P.chain_count) return;
  if (P.status[chain] != CHAIN_OK) return;
  if (P.only_ran && P.only_ran[chain] == 0) return;
  __shared__ double s_coef[RH_MAX_COEF], s_tot[RH_MAX_COEF];
  const int n = R.ncoef, T = P.T, p = P.p;
  const double *coef = R.coef + (size_t)chain * RH_MAX_COEF;
  const double *beta = P.beta + (size_t)chain * p;
  const double *sres = P.scratch + (size_t)chain * P.scratch_stride + T;
  for (int j = lane; j < n; j += WAVE) {
    s_coef[j] = coef[j];
    s_tot[j] = 0.0;
  }
  wave_lds_sync();
  // the active steps 64 at a time, a step per lane (ascending: a coefficient's sum runs in time order)
  for (int i0 = 0; i0 < R.nsteps; i0 += WAVE) {
    const bool in_l = i0 + lane < R.nsteps;
    const int t = R.steps[in_l ? i0 + lane : R.nsteps - 1];
    // x_t'beta over the non-zero coefficients, as step 1 of the state kernel
    double pred = 0.0;
    for (int base = 0; base < p; base += WAVE) {
      const int jj = base + lane;
      const double bj = (jj < p) ? beta[jj] : 0.0;
      unsigned long long mk = __ballot(bj != 0.0);
      while (mk) {
        const int l = __ffsll((long long)mk) - 1;
        mk &= mk - 1;
        const double bb = rl(bj, l);
        pred += P.X[(size_t)(base + l) * T + t] * bb;
      }
    }
    const bool ob_l = in_l && P.observed[t] != 0;   // (missing observations are skipped)
    const double r0 = sres[t] - pred;
    for (int k = 0; k < R.nmodels; ++k) {
      const int j = ob_l ? R.table[(size_t)t * RH_MAX_MODELS + k] : -1;
      // one lane at a time, in lane order: two steps of the batch may carry the same coefficient
      unsigned long long mk = __ballot(j >= 0);
      while (mk) {
        const int l = __ffsll((long long)mk) - 1;
        mk &= mk - 1;
        if (lane == l) s_tot[j] += r0 + s_coef[j];
        wave_lds_sync();
      }
    }
  }
  wave_lds_sync();
  double *tot = R.totals + (size_t)chain * RH_MAX_COEF;
  for (int j = lane; j < n; j += WAVE) tot[j] = s_tot[j];
}

__global__ __launch_bounds__(256) void rh_fill_kernel(RhParams R, int T, int chains) {
  const size_t total = (size_t)T * (size_t)chains;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    R.y[i] = R.y_shared[i % (size_t)T];
}

hipError_t launch_rh_draw(hipStream_t stream, const SsParams &P, const RhParams &R, int draw, int hier) {
  KtScope kt(stream, KT_SS_REGHOLIDAY);
  hipLaunchKernelGGL(rh_draw_kernel, dim3((unsigned)P.chain_count), dim3(WAVE), 0, stream, P, R, draw, hier);
  return hipGetLastError();
}

hipError_t launch_rh_observe(hipStream_t stream, const SsParams &P, const RhParams &R) {
  KtScope kt(stream, KT_SS_REGHOLIDAY);
  hipLaunchKernelGGL(rh_observe_kernel, dim3((unsigned)P.chain_count), dim3(WAVE), 0, stream, P, R);
  return hipGetLastError();
}

hipError_t launch_rh_fill(hipStream_t stream, const RhParams &R, int T, int chains) {
  const size_t total = (size_t)T * (size_t)chains;
  const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(rh_fill_kernel, dim3(blocks), dim3(256), 0, stream, R, T, chains);
  return hipGetLastError();
}

}  // namespace boom_amd
