// TRegressionSpikeSlabSampler for many chains: the two kernels of a draw() that the logit
// path does not already have.
//   TRegressionSpikeSlabSampler::draw          (Models/Glm/PosteriorSamplers/
//                                               TRegressionSpikeSlabSampler.cpp:41-47)
//   impute_latent_data / TDataImputer::impute  (TRegressionSampler.cpp:124-140,
//                                               TDataImputer.cpp:26-30)
//   draw_sigsq_full_conditional                (TRegressionSampler.cpp:160-166,
//                                               GenericGaussianVarianceSampler.cpp:44-63)
//   draw_nu_given_observed_data                (TRegressionSampler.cpp:173-176,
//                                               Samplers/ScalarSliceSampler.cpp:75-253)
//
// student_impute_kernel: one thread per (chain, observation), the grid of
// logit_impute_kernel.  w_i ~ Gamma((nu + 1) / 2, rate (nu + delta_i^2) / 2) with
// delta_i = (y_i - x_i'beta) / sigma, by the device's reference-exact gamma sampler, from the
// chain's stream STUDENT_IMPUTE_STREAM at slot (s n + i).  It writes w_i and z_i = w_i y_i;
// X'Wy and the diagonal of Omega^{-1} + X'WX are the logit path's rows-times-columns GEMMs.
//
// student_sigma_nu_kernel: one workgroup per chain, after the inclusion / coefficient draws.
//   1. r_i = y_i - x_i'beta at the NEW beta; wsse = sum_i w_i r_i^2 (one pass, see DESIGN:
//      the reference forms beta'X'WX beta - 2 beta'X'Wy + y'Wy from the suf);
//   2. sigma^2 by the device variance sampler (rtrun_gamma when sigma has an upper limit);
//   3. u_i = (r_i / sigma)^2 once, kept in a chains x n buffer (L2 / MALL);
//   4. nu by the slice sampler with lower limit 0, unimodal = false, the chain's own
//      suggested_dx.  log f(nu) = log prior(nu) + n [lgamma((nu+1)/2) - lgamma(nu/2)
//      - log(nu pi) / 2] - n log sigma - (nu+1)/2 sum_i log1p(u_i / nu): dt in closed form,
//      one workgroup reduction per evaluation.  Every lane takes the same control path
//      (every value that steers it is a broadcast reduction or a draw every lane makes from
//      the same stream position).
// sigma^2 and nu read the chain's stream STUDENT_SN_STREAM at slot s.
#include <hip/hip_runtime.h>

#include "ktimer.h"

#include "device_rng.h"
#include "latent_device.h"
#include "products.h"
#include "ssvs_params.h"
#include "student_params.h"

namespace boom_amd {

// SS: the state space Student family (StateSpaceStudentPosteriorSampler::
// impute_nonstate_latent_data, StateSpaceStudentPosteriorSampler.cpp:60-80): the residual is
// y_t - x_t'beta - offset_t (the chain's Z_t'alpha_t), a missing step keeps weight 0 and reads no
// random numbers, and beside w_t the kernel writes the filter's H_t = sigma^2 / w_t -- the model's
// student_marginal_variance() where the step is missing or w_t = 0 (StateSpaceStudentRegressionModel::
// observation_variance).  z is left to student_ss_suf_kernel (after the state draw).
template <bool SS>
__global__ __launch_bounds__(256) void student_impute_kernel(StudentParams P) {
  const int chain = (int)blockIdx.y, i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  __shared__ int s_status;
  if (threadIdx.x == 0) s_status = __atomic_load_n(P.status + chain, __ATOMIC_RELAXED);
  __syncthreads();
  if (s_status != CHAIN_OK) return;
  __shared__ int s_idx[STUDENT_KMAX];
  __shared__ double s_beta[STUDENT_KMAX];
  const int k = included_coefficients<STUDENT_KMAX>(P.gamma, P.beta, P.p, chain, s_idx, s_beta);
  if (k > STUDENT_KMAX) {
    if (threadIdx.x == 0 && blockIdx.x == 0) P.status[chain] = CHAIN_MODEL_TOO_LARGE;
    return;
  }
  if (i >= P.n) return;
  double eta = 0.0;
  for (int m = 0; m < k; ++m) eta += P.X[(size_t)s_idx[m] * P.n + i] * s_beta[m];
  double yi = P.y[i];
  const double nu = P.nu[chain];
  if (SS) {
    const double sigsq = P.sigsq[chain];
    if (!P.observed[i]) {
      P.w[(size_t)chain * P.n + i] = 0.0;
      P.h[(size_t)chain * P.n + i] = nu > 2 ? sigsq * nu / (nu - 2) : sigsq * 1e8;
      return;
    }
    yi -= P.offset[(size_t)chain * P.offset_stride + i];
  }
  const double delta = (yi - eta) / sqrt(P.sigsq[chain]);
  SeqRng rng = SeqRng::slot(PhiloxKey{P.seed_lo, P.seed_hi, (uint32_t)(P.chain_offset + chain), STUDENT_IMPUTE_STREAM},
                            P.sweep * (uint64_t)P.n + (uint64_t)i, STUDENT_IMPUTE_STRIDE,
                            slot_serve(P.slot_limit, STUDENT_IMPUTE_STRIDE));
  // rgamma_mt(rng, (nu + 1) / 2, (nu + delta^2) / 2): shape, rate.  The shape is above 1/2,
  // so the small-shape branch (wave-uniform only) is never taken.
  int bad = 0;
  const double w = d_rgamma_scale(rng, 0.5 * (nu + 1), 1.0 / (0.5 * (nu + delta * delta)), &bad);
  if (bad || rng.overran()) P.status[chain] = CHAIN_RNG_BRANCH;
  P.w[(size_t)chain * P.n + i] = w;
  if (SS) {
    const double sigsq = P.sigsq[chain];
    // (the reference throws "Weights must be finite and non-negative." from set_weight)
    if (!(w >= 0.0) || !isfinite(w)) P.status[chain] = STUDENT_BAD_WEIGHT;
    P.h[(size_t)chain * P.n + i] = w > 0.0 ? sigsq / w : (nu > 2 ? sigsq * nu / (nu - 2) : sigsq * 1e8);
  } else {
    P.z[(size_t)chain * P.n + i] = w * yi;
  }
}

// the state space Student family's H_t from weights the caller set (ba_ss_student_set_weights,
// all weights 1 of the first round): the same rule as student_impute_kernel<true>
__global__ __launch_bounds__(256) void student_ss_h_kernel(StudentParams P) {
  const int chain = (int)blockIdx.y, i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= P.n || P.status[chain] != CHAIN_OK) return;
  const double nu = P.nu[chain], sigsq = P.sigsq[chain];
  const double w = P.observed[i] ? P.w[(size_t)chain * P.n + i] : 0.0;
  if (!(w >= 0.0) || !isfinite(w)) { P.status[chain] = STUDENT_BAD_WEIGHT; return; }
  P.h[(size_t)chain * P.n + i] = w > 0.0 ? sigsq / w : (nu > 2 ? sigsq * nu / (nu - 2) : sigsq * 1e8);
}

// ... and after the state draw the complete-data response z_t = w_t (y_t - offset_t), 0 where
// the step is missing (update_complete_data_sufficient_statistics,
// StateSpaceStudentPosteriorSampler.cpp:113-124): the rows of the X'Wz GEMM
__global__ __launch_bounds__(256) void student_ss_suf_kernel(StudentParams P) {
  const int chain = (int)blockIdx.y, i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= P.n) return;
  const size_t at = (size_t)chain * P.n + i;
  if (!P.observed[i]) {
    P.w[at] = 0.0;
    P.z[at] = 0.0;
    return;
  }
  P.z[at] = P.w[at] * (P.y[i] - P.offset[(size_t)chain * P.offset_stride + i]);
}

namespace {

template <bool SS>
struct StuSlice {
  const StudentParams *P;
  const double *u;   // this chain's u_i
  double n_log_sigma;
  double *s_red;
  double margin;
  double nobs;   // (SS: the observed steps; else unused, n)
  // log f(nu): the prior's logp, then (unless that is -inf) the observed-data likelihood
  __device__ double logf(double nu) {
    double lp;
    if (P->nu_kind == STUDENT_NU_UNIFORM) {
      lp = (nu > P->nu_b || nu < P->nu_a) ? -__builtin_inf() : log(1.0 / (P->nu_b - P->nu_a));
    } else {
      const double a = P->nu_a, b = P->nu_b;
      lp = !(nu > 0) ? -__builtin_inf() : a * log(b) - lgamma(a) + (a - 1) * log(nu) - b * nu;
    }
    if (lp <= -__builtin_inf()) return lp;
    double part = 0.0;
    const double inv = 1.0 / nu;
    for (int i = threadIdx.x; i < P->n; i += STUDENT_SN_BLOCK) part += log1p(u[i] * inv);
    const double s = stu_block_sum(part, s_red);
    const double nn = SS ? nobs : (double)P->n;
    const double c = lgamma(0.5 * (nu + 1)) - lgamma(0.5 * nu) - 0.5 * log(nu * 3.141592653589793);
    return lp + (nn * c - n_log_sigma) - 0.5 * (nu + 1) * s;
  }
  __device__ void note(double a, double b) {
    if (!isfinite(a) || !isfinite(b)) return;
    const double den = fmax(fmax(fabs(a), fabs(b)), 1e-300);
    margin = fmin(margin, fabs(a - b) / den);
  }
};

}  // namespace

// SS: the state space Student family -- residuals y_t - offset_t - x_t'beta over the observed
// steps only (the observation model holds the observed steps' data with the time series
// residual as its response, StateSpaceStudentPosteriorSampler.cpp:90-124): DF = observed + prior df,
// the nu likelihood over the observed steps (a missing step's u_t = 0 adds log1p(0) = 0).
template <bool SS>
__global__ __launch_bounds__(STUDENT_SN_BLOCK) void student_sigma_nu_kernel(StudentParams P) {
  const int chain = (int)blockIdx.x, tid = (int)threadIdx.x;
  __shared__ int s_status;
  __shared__ double s_red[4];
  if (tid == 0) s_status = __atomic_load_n(P.status + chain, __ATOMIC_RELAXED);
  __syncthreads();
  if (s_status != CHAIN_OK) return;
  __shared__ int s_idx[STUDENT_KMAX];
  __shared__ double s_beta[STUDENT_KMAX];
  const int k = included_coefficients<STUDENT_KMAX>(P.gamma, P.beta, P.p, chain, s_idx, s_beta);
  if (k > STUDENT_KMAX) {
    if (tid == 0) P.status[chain] = CHAIN_MODEL_TOO_LARGE;
    return;
  }
  const int n = P.n;
  const double *w = P.w + (size_t)chain * n;
  double *u = P.u + (size_t)chain * n;
  // 1. residuals at the new beta, the weighted sum of squared errors
  double part = 0.0, cnt = 0.0;
  for (int i = tid; i < n; i += STUDENT_SN_BLOCK) {
    if (SS && !P.observed[i]) { u[i] = 0.0; continue; }
    double eta = 0.0;
    for (int m = 0; m < k; ++m) eta += P.X[(size_t)s_idx[m] * n + i] * s_beta[m];
    double yi = P.y[i];
    if (SS) { yi -= P.offset[(size_t)chain * P.offset_stride + i]; cnt += 1.0; }
    const double r = yi - eta;
    u[i] = r;
    part += w[i] * (r * r);
  }
  const double wsse = stu_block_sum(part, s_red);
  const double nobs = SS ? stu_block_sum(cnt, s_red) : (double)n;
  // 2. sigma^2 (GenericGaussianVarianceSampler::draw: n observations, not sum w)
  SeqRng rng = SeqRng::slot(PhiloxKey{P.seed_lo, P.seed_hi, (uint32_t)(P.chain_offset + chain), STUDENT_SN_STREAM},
                            P.sweep, STUDENT_SN_STRIDE, slot_serve(P.slot_limit, STUDENT_SN_STRIDE));
  int bad = 0;
  const double sigsq = d_draw_variance(rng, nobs + P.prior_df, wsse + P.prior_ss, P.sigma_max, &bad);
  if (bad) {
    if (tid == 0) P.status[chain] = CHAIN_RNG_BRANCH;
    return;
  }
  const double sigma = sqrt(sigsq);
  // 3. u_i = (r_i / sigma)^2 (dstudent's (x - mu) / sigma, squared as dt squares it)
  for (int i = tid; i < n; i += STUDENT_SN_BLOCK) {
    const double t = u[i] / sigma;
    u[i] = t * t;
  }
  __syncthreads();   // (every thread reads every u_i from here on)
  // 4. nu: ScalarSliceSampler::draw with lower limit 0 (find_limits -> find_upper_limit)
  StuSlice<SS> S{&P, u, nobs * log(sigma), s_red, __builtin_inf(), nobs};
  const double x = P.nu[chain];
  const double sigsq_in = P.sigsq[chain];   // (the sweep's: its summaries hold this one)
  double dx = P.dx[chain];
  double nu = x;
  int err = slice_draw_lower0(S, rng, false, x, dx, nu);
  if (rng.overran()) err = 2;
  if (tid == 0) {
    P.sigsq[chain] = sigsq;
    if (P.acc) {
      // the summaries' sigma^2 moments are those of the draws, not of the sweeps' inputs
      double *a = P.acc + (size_t)chain * ACC_COUNT;
      a[ACC_SIGSQ] = (a[ACC_SIGSQ] - sigsq_in) + sigsq;
      a[ACC_SIGSQ2] = (a[ACC_SIGSQ2] - sigsq_in * sigsq_in) + sigsq * sigsq;
    }
    if (err) {
      P.status[chain] = err == 2 ? CHAIN_RNG_BRANCH : STUDENT_SLICE_ERROR;
    } else {
      P.nu[chain] = nu;
      P.dx[chain] = dx;
    }
    P.margin[chain] = fmin(P.margin[chain], S.margin);
    if (P.trace_stride > 0) {
      const int row = P.trace_idx[chain] - 1;
      if (row >= 0 && row < P.trace_stride) {
        P.trace_sigsq[(size_t)chain * P.trace_stride + row] = sigsq;
        P.trace_nu[(size_t)chain * P.trace_stride + row] = nu;
      }
    }
  }
}

// impute, X'Wz and the diagonal of V = slab precision + X'WX for every chain
hipError_t launch_student_impute(hipStream_t stream, const StudentParams &P, const double *Xsq,
                                 const double *slab_precision, double *xtz, double *v_diag, double *planes) {
  hipError_t err;
  {
    KtScope kt(stream, KT_STUDENT_IMPUTE);
    hipLaunchKernelGGL(student_impute_kernel<false>, dim3((P.n + 255) / 256, P.chains), dim3(256), 0, stream, P);
    err = hipGetLastError();
  }
  if (err != hipSuccess) return err;
  return launch_latent_products(stream, P.z, P.w, P.chains, P.X, Xsq, (int64_t)P.n, P.p, slab_precision, xtz, v_diag,
                                planes);
}

hipError_t launch_student_sigma_nu(hipStream_t stream, const StudentParams &P) {
  KtScope kt(stream, KT_STUDENT_SIGMA_NU);
  if (P.offset) hipLaunchKernelGGL(student_sigma_nu_kernel<true>, dim3(P.chains), dim3(STUDENT_SN_BLOCK), 0, stream, P);
  else hipLaunchKernelGGL(student_sigma_nu_kernel<false>, dim3(P.chains), dim3(STUDENT_SN_BLOCK), 0, stream, P);
  return hipGetLastError();
}

// the state space Student family's weight step: w_t and H_t (draw = 0: H_t from the weights as they stand)
hipError_t launch_student_ss_weights(hipStream_t stream, const StudentParams &P, int draw) {
  KtScope kt(stream, KT_SS_STUDENT);
  const dim3 grid((P.n + 255) / 256, P.chains);
  if (draw) hipLaunchKernelGGL(student_impute_kernel<true>, grid, dim3(256), 0, stream, P);
  else hipLaunchKernelGGL(student_ss_h_kernel, grid, dim3(256), 0, stream, P);
  return hipGetLastError();
}

// ... and its complete-data statistics after a state draw: z, X'Wz and the diagonal of
// V = slab precision + X'WX
hipError_t launch_student_ss_suf(hipStream_t stream, const StudentParams &P, const double *Xsq,
                                 const double *slab_precision, double *xtz, double *v_diag, double *planes) {
  hipError_t err;
  {
    KtScope kt(stream, KT_SS_STUDENT);
    hipLaunchKernelGGL(student_ss_suf_kernel, dim3((P.n + 255) / 256, P.chains), dim3(256), 0, stream, P);
    err = hipGetLastError();
  }
  if (err != hipSuccess) return err;
  return launch_latent_products(stream, P.z, P.w, P.chains, P.X, Xsq, (int64_t)P.n, P.p, slab_precision, xtz, v_diag,
                                planes);
}

}  // namespace boom_amd
