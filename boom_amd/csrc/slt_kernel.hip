// StudentLocalLinearTrendStateModel (bsts AddStudentLocalLinearTrend) for many chains: the two
// kernels the general structural kernel's QT instances (ssm_kernel.hip) leave to this file.
//   StudentLocalLinearTrendStateModel::observe_state   (Models/StateSpace/StateModels/
//                                                        StudentLocalLinearTrend.cpp:87-120)
//   StudentLocalLinearTrendPosteriorSampler::draw      (Models/StateSpace/PosteriorSamplers/
//                                                        StudentLocalLinearTrendPosteriorSampler.cpp)
//   GenericGaussianVarianceSampler::draw, ScalarSliceSampler::draw (unimodal)
//
// The block is a local linear trend whose level and slope errors of the step t -> t + 1 have the
// variances sigma_c^2 / w_c[t] (c = level, slope); w_c[t] ~ Gamma(nu_c / 2, nu_c / 2) a priori, so
// the errors are Student-t with nu_c degrees of freedom.
//
// slt_weights_kernel -- observe_state over a state draw, after the state kernel.  One workgroup per
// chain, thread i of its 256 walks the pairs (t, c) = (i / 2, i % 2), i + 256, ...: residual
// r = now - T then of the step t -> t + 1, kept for the robust nu posterior; the
// WeightedGaussianSuf with the OLD weight (n = T - 1, sumsq = sum r^2 w_old -> var_n, var_ss); the new
// weight w ~ Gamma((nu + 1) / 2, rate (nu + r^2 / sigma^2) / 2) from stream SLT_WEIGHT_STREAM at slot
// (s T + t) 2 + c of SLT_WEIGHT_STRIDE, s = the state draws the chain has observed before; the
// GammaSuf (n, sum w, sum log w) of the new weights.  Entry T - 1 is never drawn.  The sums are
// workgroup reductions in a fixed order (one workgroup per chain rather than a grid over the steps:
// the statistics are then the same bits whatever runs beside the launch).  A weight that is not
// finite and positive stops the chain with STUDENT_BAD_WEIGHT (13).
//
// slt_params_kernel -- the sampler's draw(), before the state kernel.  One workgroup per chain,
// every thread reads the same numbers from SLT_PARAM_STREAM, in sequence from the chain's position:
// sigma_level^2, nu_level, sigma_slope^2, nu_slope.  sigma^2 by d_draw_variance on (n, sumsq); nu by
// the slice sampler of latent_device.h with unimodal = true, lower limit 0 and width 1.0 (a NEW
// ScalarSliceSampler per draw), on NuPosteriorFast (the GammaSuf) while the current nu <= 10 and on
// NuPosteriorRobust (sum of dstudent over the kept residuals, sigma the value just drawn: a
// workgroup reduction per evaluation) above.
#include <hip/hip_runtime.h>

#include "ktimer.h"

#include "device_rng.h"
#include "kalman_params.h"
#include "latent_device.h"
#include "student_params.h"

namespace boom_amd {

namespace {

__device__ __forceinline__ bool slt_skip(const SsParams &P, int chain) {
  if (P.status[chain] != CHAIN_OK) return true;
  return P.only_ran && P.only_ran[chain] == 0;
}

struct SltSlice {
  int kind;          // the prior
  double a, b;
  bool robust;
  // NuPosteriorFast: the GammaSuf of the weights
  double n, sumw, sumlog;
  // NuPosteriorRobust: the residuals and sigma
  const double *res;
  int nres;
  double sigma;
  double *s_red;
  double margin;
  __device__ double logf(double nu) {
    double lp;
    if (kind == STUDENT_NU_UNIFORM) {
      lp = (nu > b || nu < a) ? -__builtin_inf() : log(1.0 / (b - a));
    } else {
      lp = !(nu > 0) ? -__builtin_inf() : a * log(b) - lgamma(a) + (a - 1) * log(nu) - b * nu;
    }
    if (!robust) {
      if (lp <= -__builtin_inf()) return lp;   // (the sums below are finite for nu > 0: the reference's sum is -inf too)
      const double nu2 = nu / 2.0;
      double ans = lp;
      ans += n * (nu2 * log(nu2) - lgamma(nu2));
      ans += (nu2 - 1) * sumlog;
      ans -= nu2 * sumw;
      return ans;
    }
    if (!isfinite(lp)) return lp;
    // sum_t dstudent(r_t, 0, sigma, nu, log): dt in closed form, as student_kernel.hip's
    double part = 0.0;
    const double inv = 1.0 / nu;
    for (int i = threadIdx.x; i < nres; i += SLT_BLOCK) {
      const double t = res[i] / sigma;
      part += log1p((t * t) * inv);
    }
    const double s = stu_block_sum(part, s_red);
    const double c = lgamma(0.5 * (nu + 1)) - lgamma(0.5 * nu) - 0.5 * log(nu * 3.141592653589793);
    return lp + ((double)nres * c - (double)nres * log(sigma)) - 0.5 * (nu + 1) * s;
  }
  __device__ void note(double x, double y) {
    if (!isfinite(x) || !isfinite(y)) return;
    const double den = fmax(fmax(fabs(x), fabs(y)), 1e-300);
    margin = fmin(margin, fabs(x - y) / den);
  }
};

}  // namespace

__global__ __launch_bounds__(SLT_BLOCK) void slt_weights_kernel(SsParams P, SltParams U) {
  const int chain = (int)blockIdx.x + P.chain_first, tid = (int)threadIdx.x;
  if ((int)blockIdx.x >= P.chain_count) return;
  if (slt_skip(P, chain)) return;
  __shared__ double s_red[4];
  const SsmParams &M = P.ssm;
  const SsgBlock &K = M.spec->blk[M.spec->student_block - 1];
  const int T = P.T, m = M.m, f = K.first, c = tid & 1;
  const size_t at = (size_t)chain * SSG_MAX_VAR + K.var0;
  const double *gst = M.work + (size_t)chain * M.work_stride + (size_t)m * T;   // the state draw, T x m
  double *w = U.w + ((size_t)chain * 2 + c) * T;
  double *res = U.res + ((size_t)chain * 2 + c) * T;
  const double nu = U.nu[(size_t)chain * 2 + c], sigsq = M.var_sigsq[at + c];
  const uint64_t s = U.count[chain];
  double ss = 0.0, sumw = 0.0, sumlog = 0.0;
  int bad = 0, badw = 0;
  for (int i = tid; i < 2 * (T - 1); i += SLT_BLOCK) {
    const int t = i >> 1;   // the step t -> t + 1
    const double *then = gst + (size_t)t * m + f, *now = then + m;
    const double r = c == 0 ? now[0] - (then[0] + then[1]) : now[1] - then[1];
    res[t] = r;
    ss += (r * r) * w[t];
    SeqRng rng = SeqRng::slot(PhiloxKey{P.seed_lo, P.seed_hi, (uint32_t)(P.chain_offset + chain), SLT_WEIGHT_STREAM},
                              (s * (uint64_t)T + (uint64_t)t) * 2 + (uint64_t)c, SLT_WEIGHT_STRIDE,
                              slot_serve(P.slot_limit, SLT_WEIGHT_STRIDE));
    // rgamma(alpha, beta): shape (1 + nu) / 2 > 1 / 2, so the small-shape branch is never taken
    const double wn = d_rgamma_scale(rng, .5 * (1 + nu), 1.0 / (.5 * (nu + r * r / sigsq)), &bad);
    if (rng.overran()) bad = 1;
    if (!(wn > 0.0) || !isfinite(wn)) badw = 1;
    w[t] = wn;
    sumw += wn;
    sumlog += log(wn);
  }
  const double ss0 = stu_block_sum(c == 0 ? ss : 0.0, s_red), ss1 = stu_block_sum(c == 1 ? ss : 0.0, s_red);
  const double sw0 = stu_block_sum(c == 0 ? sumw : 0.0, s_red), sw1 = stu_block_sum(c == 1 ? sumw : 0.0, s_red);
  const double sl0 = stu_block_sum(c == 0 ? sumlog : 0.0, s_red), sl1 = stu_block_sum(c == 1 ? sumlog : 0.0, s_red);
  const int anybad = __syncthreads_or(bad), anybadw = __syncthreads_or(badw);
  if (tid == 0) {
    M.var_n[at] = (double)(T - 1);
    M.var_n[at + 1] = (double)(T - 1);
    M.var_ss[at] = ss0;
    M.var_ss[at + 1] = ss1;
    double *g = U.wsuf + (size_t)chain * 6;
    g[0] = (double)(T - 1); g[1] = sw0; g[2] = sl0;
    g[3] = (double)(T - 1); g[4] = sw1; g[5] = sl1;
    U.count[chain] = s + 1;
    if (anybadw) P.status[chain] = STUDENT_BAD_WEIGHT;
    else if (anybad) P.status[chain] = CHAIN_RNG_BRANCH;
  }
}

__global__ __launch_bounds__(SLT_BLOCK) void slt_params_kernel(SsParams P, SltParams U) {
  const int chain = (int)blockIdx.x + P.chain_first, tid = (int)threadIdx.x;
  if ((int)blockIdx.x >= P.chain_count) return;
  if (slt_skip(P, chain)) return;
  __shared__ double s_red[4];
  const SsmParams &M = P.ssm;
  const SsgSpec &Q = *M.spec;
  const SsgBlock &K = Q.blk[Q.student_block - 1];
  const int T = P.T;
  const size_t at = (size_t)chain * SSG_MAX_VAR + K.var0;
  SeqRng rng{PhiloxKey{P.seed_lo, P.seed_hi, (uint32_t)(P.chain_offset + chain), SLT_PARAM_STREAM}, U.pos[chain]};
  double sig2[2], nus[2];
  int status = CHAIN_OK;
  for (int c = 0; c < 2 && status == CHAIN_OK; ++c) {
    const int vi = K.var0 + c;
    const double n = M.var_n[at + c];
    int bad = 0;
    sig2[c] = d_draw_variance(rng, n + Q.prior_df[vi], M.var_ss[at + c] + Q.prior_ss[vi], Q.sigma_max[vi], &bad);
    if (bad) { status = CHAIN_RNG_BRANCH; break; }
    const double x = U.nu[(size_t)chain * 2 + c];
    const double *g = U.wsuf + (size_t)chain * 6 + 3 * c;
    // (the residuals kept are those of the last state draw: none before the first)
    SltSlice S{U.nu_kind[c], U.nu_a[c], U.nu_b[c], x > 10, g[0], g[1], g[2],
               U.res + ((size_t)chain * 2 + c) * T, (int)n, sqrt(sig2[c]), s_red, __builtin_inf()};
    double dx = 1.0;
    nus[c] = x;
    if (slice_draw_lower0(S, rng, true, x, dx, nus[c])) status = STUDENT_SLICE_ERROR;
  }
  __syncthreads();   // (everybody has read the statistics and the old position)
  if (tid == 0) {
    if (status != CHAIN_OK) {
      P.status[chain] = status;
    } else {
      M.var_sigsq[at] = sig2[0];
      M.var_sigsq[at + 1] = sig2[1];
      U.nu[(size_t)chain * 2] = nus[0];
      U.nu[(size_t)chain * 2 + 1] = nus[1];
      U.pos[chain] = rng.pos;
    }
  }
}

hipError_t launch_slt_weights(hipStream_t stream, const SsParams &P, const SltParams &U) {
  KtScope kt(stream, KT_SS_STUDENT_TREND);
  hipLaunchKernelGGL(slt_weights_kernel, dim3(P.chain_count), dim3(SLT_BLOCK), 0, stream, P, U);
  return hipGetLastError();
}

hipError_t launch_slt_params(hipStream_t stream, const SsParams &P, const SltParams &U) {
  KtScope kt(stream, KT_SS_STUDENT_TREND);
  hipLaunchKernelGGL(slt_params_kernel, dim3(P.chain_count), dim3(SLT_BLOCK), 0, stream, P, U);
  return hipGetLastError();
}

}  // namespace boom_amd
