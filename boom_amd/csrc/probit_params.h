// Launch parameters of the probit data-augmentation kernel (probit_kernel.hip),
// shared with the host side (engine_glm.hip).
#pragma once
#include <stdint.h>

#include "latent_params.h"
#include "ssvs_params.h"

namespace boom_amd {

enum { PROBIT_STRIDE = 4096, PROBIT_KMAX = 1024, LOGIT_STRIDE = 256, PG_STRIDE = 4096, POISSON_STRIDE = 256,
       POISSON_MAX_COMP = 32 };
// the variance of the negative log of an exponential, pi^2 / 6: what the state space Poisson
// family's filter uses at a missing step (Constants::pi_squared_over_6)
#define POISSON_MISSING_VARIANCE 1.6449340668482264
// ... and the variance of the standard logistic distribution, pi^2 / 3: the state space logit
// family's (Constants::pi_squared_over_3)
#define LOGIT_MISSING_VARIANCE 3.2898681336964528

// z: the observations' sums of latent normals; w: their total precision (logit and Poisson only)
struct ProbitParams : LatentParams {
  int32_t clt_threshold;
  const double *y;        // successes
  const double *ntrials;  // trials
  double *xtz;            // chains x p: X'z
  // Poisson regression (poisson_impute_kernel): ntrials holds the exposures; the
  // reference table's normal mixtures of NegLogGamma(count) -- mixture m has components
  // [mix_off[m], mix_off[m + 1]) of (mix_mu, mix_sigma, mix_logw); obs_mix[i] = the
  // mixture of observation i's count (-1: the Gaussian limit beyond the table; unused
  // for a zero count), mix_one = the mixture of count 1
  const int32_t *mix_off;
  const double *mix_mu, *mix_sigma, *mix_logw;
  const int32_t *obs_mix;
  int32_t mix_one;
  // the state space Poisson and logit families (poisson_impute_kernel<true>,
  // logit_impute_kernel<true>, latent_ss_h_kernel, latent_ss_suf_kernel; nullptr elsewhere): which steps are observed; the chain's
  // Z_t'alpha_t of the last state draw, offset_stride doubles apart; the latent values v_t
  // (chains x n; w holds their precisions q_t) and the filter's H_t = 1 / q_t (chains x n)
  const uint8_t *observed;
  const double *offset;
  int64_t offset_stride;
  double *value;
  double *h;
};

}  // namespace boom_amd
