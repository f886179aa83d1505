// Launch parameters of the multinomial logit imputation kernels (mlogit_kernel.hip), shared
// with the host side (engine_glm.hip).
#pragma once
#include <stdint.h>

#include "latent_params.h"

namespace boom_amd {

// Substream of MLVS:
//   MLOGIT_IMPUTE_STREAM  the utilities of observation i in sweep s at slot s n + i, MLOGIT_IMPUTE_STRIDE
// (id 48: the next free multiple of 16 after the quantile sampler's 32; quantile_params.h lists
// the ids in use.)  An observation reads 2 M uniforms -- rlexp(loglam), then for every choice m
// in order rlexp(eta_m) unless m is the response, and the uniform of unmix -- plus one per
// retry of an rlexp whose log(-log(U)) is not finite: at most 32 at M = 16, half the slot.
enum : uint32_t { MLOGIT_IMPUTE_STREAM = 48u };
enum { MLOGIT_IMPUTE_STRIDE = 64, MLOGIT_KMAX = 1024, MLOGIT_MAX_CHOICES = 16, MLOGIT_NCOMP = 10 };
// a non-finite linear predictor or utility, or an unmix scan that fell off its end, as a chain
// status word
enum { MLOGIT_IMPUTE_ERROR = 11 };

// n is the number of SUBJECTS: the rows of X, z, w and u are N = n * nchoices (row i M + m,
// ChoiceData::write_x(false)), p = D = (M - 1) psub + pch columns.  z: w u; w: sigsq_inv of the
// drawn mixture component.
struct MlogitParams : LatentParams {
  int32_t nchoices;
  const int32_t *y;       // n, 0 .. M - 1
  double *u;              // chains x N: the utilities less the component's mean
  double *wss_part;       // chains x blocks: the workgroups' shares of sum w u^2
  double *wss;            // chains: their sum in block order
  // the normal mixture for the extreme value distribution (MLVS_data_imputer.cpp:39-43), as
  // the constructor there derives it: mu_, sd_, sigsq_inv_, log_mixing_weights_ plus log(sd_)
  double mix_mu[MLOGIT_NCOMP], mix_sd[MLOGIT_NCOMP], mix_prec[MLOGIT_NCOMP], mix_logw[MLOGIT_NCOMP],
      mix_logsd[MLOGIT_NCOMP];
};

}  // namespace boom_amd
