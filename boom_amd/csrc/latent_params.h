// The common head of the imputation kernels' launch parameters (probit_params.h,
// student_params.h, quantile_params.h, mlogit_params.h): what every latent-data family's
// kernel reads, filled by one host function (fill_latent_params, engine_glm.hip).  The
// response stays with each family (MLVS's is int32_t).
#pragma once
#include <stdint.h>

namespace boom_amd {

struct LatentParams {
  int32_t n, p, chains;   // observations, columns of X, chains
  int32_t slot_limit;     // > 0: uniforms a substream slot serves before its spill stream (default: the stride)
  int64_t chain_offset;
  const double *X;        // rows x p column-major (rows = n; MLVS: n * nchoices)
  const uint8_t *gamma;   // chains x p
  const double *beta;     // chains x p
  double *z;              // chains x rows: the latent responses, already weighted
  double *w;              // chains x rows: the observations' weights (none for probit)
  uint32_t seed_lo, seed_hi;
  uint64_t sweep;         // imputations done so far (positions the substreams)
  int32_t *status;
};

}  // namespace boom_amd
