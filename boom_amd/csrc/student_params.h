// Launch parameters of the Student-t regression kernels (student_kernel.hip), shared with
// the host side (engine_glm.hip).
#pragma once
#include <stdint.h>

#include "latent_params.h"

namespace boom_amd {

// Substreams of TRegressionSpikeSlabSampler:
//   STUDENT_IMPUTE_STREAM  the weight of observation i in sweep s at slot s n + i, STUDENT_IMPUTE_STRIDE
//   STUDENT_SN_STREAM      sigma^2, then nu, of sweep s at slot s, STUDENT_SN_STRIDE
// (ids 31 and 15: no other sampler reads them.  The fixed ids are 0-5 and 8-11; the structural
// state models' variance samplers take level 1, slope 6, seasonal 7, autoregression 12, trig
// 13 and semilocal 14, each plus 16 per earlier block of its family: 15 + 16 k is never taken)
enum : uint32_t { STUDENT_IMPUTE_STREAM = 31u, STUDENT_SN_STREAM = 15u };
enum { STUDENT_IMPUTE_STRIDE = 256, STUDENT_SN_STRIDE = 4096, STUDENT_KMAX = 1024, STUDENT_SN_BLOCK = 256 };
// the slice sampler's error exits (ScalarSliceSampler.cpp), as chain status words
enum { STUDENT_SLICE_ERROR = 9 };
// a weight of the state space Student family that is negative or not finite ("Weights must be
// finite and non-negative.", StateSpaceStudentRegressionModel.cpp set_weight)
enum { STUDENT_BAD_WEIGHT = 13 };
// the nu prior: Uniform(a, b) or Gamma(a, b) (shape, rate)
enum { STUDENT_NU_UNIFORM = 0, STUDENT_NU_GAMMA = 1 };

// z: w_i y_i; w: the imputed weights; sweep: draws done so far.  (The priors come first: with
// this order of the fields every kernel of student_kernel.hip keeps the register counts it had
// before the structs got their common head)
struct StudentParams : LatentParams {
  // sigma^2 | beta, w: GenericGaussianVarianceSampler (DF = n + prior_df, SS = wsse + prior_ss)
  double prior_df, prior_ss, sigma_max;
  int32_t nu_kind;
  double nu_a, nu_b;
  const double *y;        // n
  double *sigsq;          // chains
  double *nu;             // chains
  double *dx;             // chains: the slice sampler's suggested_dx
  double *margin;         // chains: smallest relative gap of a slice comparison (running min)
  double *u;              // chains x n: (r_i / sigma)^2 at the new beta and sigma
  // recorded draws (ba_enable_draws): row trace_idx[c] - 1 of chain c gets sigma^2 and nu
  const int32_t *trace_idx;
  double *trace_sigsq;
  double *trace_nu;
  int32_t trace_stride;
  // the running summaries (chains x ACC_COUNT): the sweep added the sigma^2 it was given,
  // the sigma^2 / nu kernel puts the new draw in its place
  double *acc;
  // the state space Student family (nullptr: plain Student-t regression): the chain's
  // Z_t'alpha_t of the last state draw, offset_stride doubles apart; which steps are observed;
  // the filter's H_t = sigma^2 / w_t (chains x n)
  const double *offset;
  int64_t offset_stride;
  const uint8_t *observed;
  double *h;
};

}  // namespace boom_amd
