// QuantileRegressionSpikeSlabSampler for many chains: the one kernel of a draw() that the
// logit path does not already have.
//   QuantileRegressionSpikeSlabSampler::draw  (Models/Glm/PosteriorSamplers/
//                                              QuantileRegressionPosteriorSampler.cpp:77-91)
//   QuantileRegressionImputeWorker::impute_latent_data_point  (the same file, :30-39)
//   rig_mt                                    (distributions/inverse_gaussian.cpp:59-69)
//
// quantile_impute_kernel: one thread per (chain, observation), the grid of
// student_impute_kernel.  With r_i = |y_i - x_i'beta| > 0 the weight is
// w_i = lambda_inv ~ InverseGaussian(mean 1 / r_i, shape 1), one normal and then one uniform
// from the chain's stream QUANTILE_IMPUTE_STREAM at slot (s n + i).  The weighted regression
// takes (x_i, y*_i, w_i) with y*_i = y_i - (2 (1 - q) - 1) / w_i; the kernel writes w_i and
// z_i = w_i y*_i = w_i y_i - (1 - 2 q), formed that way (w (y - c / w) rounds twice more for
// nothing).  X'Wz and the diagonal of Omega^{-1} + X'WX are the logit path's rows-times-columns
// GEMMs.  A zero residual -- or one so small that 1 / r is not finite -- leaves the
// observation out as the reference does: w = z = 0 and no number is read.
//
// Deviation from the reference: rig_mt forms the smaller root of its quadratic
// as mu + mu y mu2lam - mu2lam sqrt(mu y (4 lambda + mu y)), which cancels when
// t = mu y / (2 lambda) is large, i.e. at small residuals (2e-7 relative at t = 2e4).  The
// kernel evaluates the same root as mu / (1 + t + sqrt(t (2 + t))), accurate to a few ulp
// for every t; y = z^2, the test u > mu / (mu + x) and the other root mu^2 / x are rig_mt's.
#include <hip/hip_runtime.h>

#include "ktimer.h"

#include "device_rng.h"
#include "latent_device.h"
#include "products.h"
#include "quantile_params.h"
#include "ssvs_params.h"

namespace boom_amd {

__global__ __launch_bounds__(256) void quantile_impute_kernel(QuantileParams P) {
  const int chain = (int)blockIdx.y, i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  __shared__ int s_status;
  if (threadIdx.x == 0) s_status = __atomic_load_n(P.status + chain, __ATOMIC_RELAXED);
  __syncthreads();
  if (s_status != CHAIN_OK) return;
  __shared__ int s_idx[QUANTILE_KMAX];
  __shared__ double s_beta[QUANTILE_KMAX];
  const int k = included_coefficients<QUANTILE_KMAX>(P.gamma, P.beta, P.p, chain, s_idx, s_beta);
  if (k > QUANTILE_KMAX) {
    if (threadIdx.x == 0 && blockIdx.x == 0) P.status[chain] = CHAIN_MODEL_TOO_LARGE;
    return;
  }
  if (i >= P.n) return;
  double eta = 0.0;
  for (int m = 0; m < k; ++m) eta += P.X[(size_t)s_idx[m] * P.n + i] * s_beta[m];
  const double yi = P.y[i];
  const double r = fabs(yi - eta);
  const double mu = 1.0 / r;
  double w = 0.0, z = 0.0;
  if (r > 0.0 && isfinite(mu)) {
    SeqRng rng = SeqRng::slot(PhiloxKey{P.seed_lo, P.seed_hi, (uint32_t)(P.chain_offset + chain), QUANTILE_IMPUTE_STREAM},
                              P.sweep * (uint64_t)P.n + (uint64_t)i, QUANTILE_IMPUTE_STRIDE,
                              slot_serve(P.slot_limit, QUANTILE_IMPUTE_STRIDE));
    // rig_mt(rng, mu, 1.0) with the smaller root in its stable form
    const double nz = d_norm_rand(rng);
    const double yy = nz * nz;
    const double t = 0.5 * (mu * yy);
    double x = mu / (1.0 + t + sqrt(t * (2.0 + t)));
    const double u = rng();
    if (u > mu / (mu + x)) x = mu * mu / x;
    if (rng.overran()) {
      P.status[chain] = CHAIN_RNG_BRANCH;
    } else if (!(x > 0.0) || !isfinite(x)) {
      P.status[chain] = QUANTILE_WEIGHT_ERROR;   // (w = z = 0 below: no NaN reaches the GEMM)
    } else {
      w = x;
      z = w * yi - P.shift;
    }
  }
  P.w[(size_t)chain * P.n + i] = w;
  P.z[(size_t)chain * P.n + i] = z;
}

// impute, X'Wz and the diagonal of V = slab precision + X'WX for every chain
hipError_t launch_quantile_impute(hipStream_t stream, const QuantileParams &P, const double *Xsq,
                                  const double *slab_precision, double *xtz, double *v_diag, double *planes) {
  hipError_t err;
  {
    KtScope kt(stream, KT_QUANTILE_IMPUTE);
    hipLaunchKernelGGL(quantile_impute_kernel, dim3((P.n + 255) / 256, P.chains), dim3(256), 0, stream, P);
    err = hipGetLastError();
  }
  if (err != hipSuccess) return err;
  return launch_latent_products(stream, P.z, P.w, P.chains, P.X, Xsq, (int64_t)P.n, P.p, slab_precision, xtz, v_diag,
                                planes);
}

}  // namespace boom_amd
