// Launch parameters of the quantile regression imputation kernel (quantile_kernel.hip), shared
// with the host side (engine_glm.hip).
#pragma once
#include <stdint.h>

#include "latent_params.h"

namespace boom_amd {

// Substream of QuantileRegressionSpikeSlabSampler:
//   QUANTILE_IMPUTE_STREAM  the weight of observation i in sweep s at slot s n + i, QUANTILE_IMPUTE_STRIDE
// (id 32: no other sampler reads it.  The fixed ids are 0-5, 8-11, 15 and 31; the structural
// state models' variance samplers take 1, 6, 7, 12, 13 and 14, each plus 16 per earlier block
// of its family: a multiple of 16 is never taken)
enum : uint32_t { QUANTILE_IMPUTE_STREAM = 32u };
enum { QUANTILE_IMPUTE_STRIDE = 256, QUANTILE_KMAX = 1024 };
// an inverse-Gaussian draw that came out non-finite or not positive, as a chain status word
enum { QUANTILE_WEIGHT_ERROR = 10 };

// z: w_i y*_i = w_i y_i - (1 - 2 q); w: the imputed weights lambda_inv (0 where the residual is 0)
struct QuantileParams : LatentParams {
  const double *y;        // n
  double shift;           // 1 - 2 q = 2 (1 - q) - 1
};

}  // namespace boom_amd
