// MLVS -- multinomial logit spike and slab (mlm.spike's data-augmentation move) -- for many
// chains: the kernels of a draw() that the logit path does not already have.
//   MLVS::draw                                 (Models/Glm/PosteriorSamplers/MLVS.cpp:71-75)
//   MlvsDataImputer::impute_latent_data_point  (Models/Glm/PosteriorSamplers/MLVS_data_imputer.cpp:51-73)
//   MlvsDataImputer::unmix                     (the same file, :76-82)
//   rlexp_mt                                   (distributions/rlexp.cpp:25-31)
//   lse, lse2                                  (cpputil/lse.cpp:27-40, cpputil/lse.hpp:31-39)
//   rmulti_mt                                  (distributions/rmulti.cpp:41-78)
//   MultinomialLogitCompleteDataSufficientStatistics::update
//                                              (Models/Glm/MultinomialLogitCompleteDataSuf.cpp:41-50)
//
// mlogit_expand_kernel: the expanded design of ChoiceData::write_x(false)
// (Models/Glm/ChoiceData.cpp:93-115), N = n M rows by D = (M - 1) psub + pch columns, and its
// element-wise square.  Row i M + m holds xsubject_i in columns [(m - 1) psub, m psub) for
// m >= 1 (nothing for the baseline choice 0) and xchoice_{i, m} in the last pch columns.
//
// mlogit_impute_kernel: one thread per (chain, observation), the grid of
// quantile_impute_kernel.  The Fruhwirth-Schnatter / Fruhwirth utilities of the M choices --
// u_y = -logzmin, logzmin = rlexp(lse(eta)); u_m = -lse2(logzmin, rlexp(eta_m)) for m != y --
// and, for every m, the component k of the ten-component normal mixture for the extreme value
// distribution given u_m - eta_m; then u_m -= mu_k and w_m = sigsq_inv_k.  The uniforms come
// from the chain's stream MLOGIT_IMPUTE_STREAM at slot (s n + i) in the reference's order.
// The kernel writes u, w and z = w u per expanded row and the workgroup's share of
// weighted_sum_of_squares = sum w u^2; mlogit_wss_kernel adds the shares in block order (no
// floating-point atomics: the empty model's value in the sweep is reproducible bit for bit).
// X'Wu and the diagonal of Omega^{-1} + X'WX are the logit path's rows-times-columns GEMMs.
#include <hip/hip_runtime.h>

#include "ktimer.h"

#include "device_rng.h"
#include "latent_device.h"
#include "mlogit_params.h"
#include "products.h"
#include "ssvs_params.h"

namespace boom_amd {

namespace {

// rlexp_mt: log(-log(U)) - loglam, U redrawn while the double logarithm is not finite (the
// reference has no bound on the redraws; 32 in a row do not happen -- *bad if they do)
__device__ __forceinline__ double ml_rlexp(SeqRng &rng, double loglam, bool *bad) {
  double ans = log(-log(rng()));
  for (int t = 0; !isfinite(ans) && t < 32; ++t) ans = log(-log(rng()));
  if (!isfinite(ans)) *bad = true;
  return ans - loglam;
}

// lse2 (cpputil/lse.hpp:31-39)
__device__ __forceinline__ double ml_lse2(double x, double y) {
  if (x < y) { const double t = x; x = y; y = t; }
  return x + log1p(exp(y - x));
}

// unmix (MLVS_data_imputer.cpp:76-82): the component's index, -1 when the scan of rmulti_mt
// falls off its end
__device__ __forceinline__ int ml_unmix(const MlogitParams &P, SeqRng &rng, double v) {
  double pp[MLOGIT_NCOMP], mx = -__builtin_huge_val(), nc = 0.0;
#pragma unroll
  for (int c = 0; c < MLOGIT_NCOMP; ++c) {
    // dnorm(v, mu, sd, true) = -(M_LN_SQRT_2PI + 0.5 x^2 + log(sd)), x = (v - mu) / sd
    const double xs = (v - P.mix_mu[c]) / P.mix_sd[c];
    pp[c] = P.mix_logw[c] + -(0.918938533204672741780329736406 + 0.5 * xs * xs + P.mix_logsd[c]);
    mx = pp[c] > mx ? pp[c] : mx;
  }
  // Vector::normalize_logprob (LinAlg/Vector.cpp:390-407)
#pragma unroll
  for (int c = 0; c < MLOGIT_NCOMP; ++c) { pp[c] = exp(pp[c] - mx); nc += pp[c]; }
  double probsum = 0.0;
#pragma unroll
  for (int c = 0; c < MLOGIT_NCOMP; ++c) { pp[c] /= nc; probsum += pp[c]; }
  // rmulti_mt (distributions/rmulti.cpp:41-78)
  const double tmp = d_runif(rng, 0.0, probsum);
  double psum = 0.0;
  int ind = -1;
#pragma unroll
  for (int c = 0; c < MLOGIT_NCOMP; ++c) {
    psum += pp[c];
    if (ind < 0 && tmp <= psum) ind = c;
  }
  return ind;
}

}  // namespace

__global__ __launch_bounds__(256) void mlogit_expand_kernel(int64_t n, int M, int psub, int pch, const double *Xs,
                                                            const double *Xc, double *X, double *Xsq) {
  const int64_t N = n * (int64_t)M;
  const int64_t D = (int64_t)(M - 1) * psub + pch;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * D) return;
  const int64_t c = e / N, r = e - c * N;
  const int64_t i = r / M;
  const int m = (int)(r - i * M);
  const int64_t nsub = (int64_t)(M - 1) * psub;
  double v = 0.0;
  if (c < nsub) {
    const int64_t blk = c / psub, jj = c - blk * psub;
    if ((int64_t)m == blk + 1) v = Xs[jj * n + i];
  } else {
    v = Xc[(c - nsub) * N + r];
  }
  X[e] = v;
  Xsq[e] = v * v;
}

__global__ __launch_bounds__(256) void mlogit_impute_kernel(MlogitParams P) {
  const int chain = (int)blockIdx.y, i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int M = P.nchoices;
  __shared__ int s_status;
  __shared__ double s_part[4];
  if (threadIdx.x == 0) s_status = __atomic_load_n(P.status + chain, __ATOMIC_RELAXED);
  __syncthreads();
  if (s_status != CHAIN_OK) return;
  __shared__ int s_idx[MLOGIT_KMAX];
  __shared__ double s_beta[MLOGIT_KMAX];
  const int k = included_coefficients<MLOGIT_KMAX>(P.gamma, P.beta, P.p, chain, s_idx, s_beta);
  if (k > MLOGIT_KMAX) {
    if (threadIdx.x == 0 && blockIdx.x == 0) P.status[chain] = CHAIN_MODEL_TOO_LARGE;
    return;
  }
  const bool active = i < P.n;
  const size_t N = (size_t)P.n * (size_t)M;
  const size_t row0 = (size_t)(active ? i : 0) * (size_t)M;
  double wss = 0.0;
  if (active) {
    // eta_m = row (i, m) of the expanded design times beta, over the included coefficients:
    // one walk of the list, the M rows side by side (registers: every index is a constant)
    double eta[MLOGIT_MAX_CHOICES];
#pragma unroll
    for (int m = 0; m < MLOGIT_MAX_CHOICES; ++m) eta[m] = 0.0;
    for (int j = 0; j < k; ++j) {
      const double *col = P.X + (size_t)s_idx[j] * N + row0;
      const double b = s_beta[j];
#pragma unroll
      for (int m = 0; m < MLOGIT_MAX_CHOICES; ++m)
        if (m < M) eta[m] += col[m] * b;
    }
    const int y = P.y[i];
    // lse_safe (cpputil/lse.cpp:27-40)
    double mx = -__builtin_huge_val();
#pragma unroll
    for (int m = 0; m < MLOGIT_MAX_CHOICES; ++m)
      if (m < M) mx = eta[m] > mx ? eta[m] : mx;
    double tot = 0.0;
#pragma unroll
    for (int m = 0; m < MLOGIT_MAX_CHOICES; ++m)
      if (m < M) tot += exp(eta[m] - mx);
    const double loglam = mx + log(tot);
    bool bad = !isfinite(loglam);   // (a non-finite eta_m makes it so: NaN, +inf, or all -inf)
#pragma unroll
    for (int m = 0; m < MLOGIT_MAX_CHOICES; ++m)
      if (m < M) bad = bad || !isfinite(eta[m]);
    SeqRng rng = SeqRng::slot(PhiloxKey{P.seed_lo, P.seed_hi, (uint32_t)(P.chain_offset + chain), MLOGIT_IMPUTE_STREAM},
                              P.sweep * (uint64_t)P.n + (uint64_t)i, MLOGIT_IMPUTE_STRIDE,
                              slot_serve(P.slot_limit, MLOGIT_IMPUTE_STRIDE));
    double logzmin = 0.0;
    if (!bad) logzmin = ml_rlexp(rng, loglam, &bad);
    double *wo = P.w + (size_t)chain * N + row0, *zo = P.z + (size_t)chain * N + row0,
           *uo = P.u + (size_t)chain * N + row0;
#pragma unroll
    for (int m = 0; m < MLOGIT_MAX_CHOICES; ++m) {
      if (m < M) {
        double um = 0.0, wm = 0.0;
        if (!bad) {
          um = -logzmin;
          if (m != y) um = -ml_lse2(logzmin, ml_rlexp(rng, eta[m], &bad));
          if (!isfinite(um)) bad = true;
        }
        if (!bad) {
          const int c = ml_unmix(P, rng, um - eta[m]);
          if (c < 0) bad = true;
          double muc = 0.0;
#pragma unroll
          for (int q = 0; q < MLOGIT_NCOMP; ++q)
            if (q == c) { muc = P.mix_mu[q]; wm = P.mix_prec[q]; }
          um -= muc;
        }
        if (bad || rng.overran()) { um = 0.0; wm = 0.0; }
        wo[m] = wm;
        uo[m] = um;
        zo[m] = wm * um;
        wss += wm * (um * um);
      }
    }
    if (rng.overran()) P.status[chain] = CHAIN_RNG_BRANCH;
    else if (bad) P.status[chain] = MLOGIT_IMPUTE_ERROR;   // (w = z = 0 from there on: no NaN reaches the GEMM)
  }
  // the workgroup's share of sum w u^2: a fixed tree over the lanes, the four waves in order
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) wss += __shfl_down(wss, off, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = wss;
  __syncthreads();
  if (threadIdx.x == 0)
    P.wss_part[(size_t)chain * gridDim.x + blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// weighted_sum_of_squares of every chain: the workgroups' shares in block order
__global__ __launch_bounds__(256) void mlogit_wss_kernel(MlogitParams P, int nblocks) {
  const int chain = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (chain >= P.chains) return;
  if (P.status[chain] != CHAIN_OK) return;
  const double *part = P.wss_part + (size_t)chain * nblocks;
  double a = 0.0;
  for (int b = 0; b < nblocks; ++b) a += part[b];
  P.wss[chain] = a;
}

hipError_t launch_mlogit_expand(hipStream_t stream, int64_t n, int M, int psub, int pch, const double *Xs,
                                const double *Xc, double *X, double *Xsq) {
  const int64_t total = n * M * ((int64_t)(M - 1) * psub + pch);
  hipLaunchKernelGGL(mlogit_expand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, n, M, psub,
                     pch, Xs, Xc, X, Xsq);
  return hipGetLastError();
}

// impute, weighted_sum_of_squares, X'Wu and the diagonal of V = slab precision + X'WX for
// every chain
hipError_t launch_mlogit_impute(hipStream_t stream, const MlogitParams &P, const double *Xsq,
                                const double *slab_precision, double *xtz, double *v_diag, double *planes) {
  hipError_t err;
  const int nblocks = (P.n + 255) / 256;
  {
    KtScope kt(stream, KT_MLOGIT_IMPUTE);
    hipLaunchKernelGGL(mlogit_impute_kernel, dim3(nblocks, P.chains), dim3(256), 0, stream, P);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(mlogit_wss_kernel, dim3((P.chains + 255) / 256), dim3(256), 0, stream, P, nblocks);
    err = hipGetLastError();
  }
  if (err != hipSuccess) return err;
  const int64_t N = (int64_t)P.n * P.nchoices;
  return launch_latent_products(stream, P.z, P.w, P.chains, P.X, Xsq, N, P.p, slab_precision, xtz, v_diag,
                                planes);
}

}  // namespace boom_amd
