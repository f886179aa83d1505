// ArSpikeSlabSampler (bsts AddAutoAr) for many chains: the sampler of an autoregression state model
// whose coefficients have a spike-and-slab prior.  To the structural kernels the block is an
// ordinary autoregression whose excluded coefficients are 0; this kernel is its sampler, launched
// ahead of the state kernel (which passes the block's sampler by: SsgBlock::ar_spike).
//   ArSpikeSlabSampler::draw            (Models/TimeSeries/PosteriorSamplers/ArSpikeSlabSampler.cpp)
//   SpikeSlabSampler::draw_model_indicators, draw_beta, log_model_prob
//                                        (Models/Glm/PosteriorSamplers/SpikeSlabSampler.cpp)
//   VariableSelectionPrior::logp, make_valid (Models/Glm/VariableSelectionPrior.cpp:271-300)
//
// One wavefront per (chain, block).  Vectors sit one component per lane (lane i < L), the L x L
// matrices in LDS at leading dimension AR_MAX; every lane reads the same random numbers, from the
// block's sampler stream (SsgBlock::sid[0]) at the chain's position (pos_var), in sequence:
//   1. draw_model_indicators -- the Fisher-Yates shuffle (random_int(0, i), i = L - 1 .. 1), then
//      min(L, max_flips) Metropolis flips, one uniform each;
//   2. draw_phi -- up to 100 proposals of draw_beta (n normals each, n the model's size), accepted
//      when not truncating or stationary; after 100 failures draw_phi_univariate;
//   3. sigma^2 from (n, relative_sse) with the sigma upper limit.
// The included set is compacted by ballot and prefix count: lane k < n holds the k-th included
// lag; log_model_prob and the coefficient draw factor the selected sub-matrix with ar_chol and
// solve with ar_lsolve / ar_ltsolve (ar_sampler_device.h).
#include <hip/hip_runtime.h>

#include "ktimer.h"

#include "device_rng.h"
#include "kalman_params.h"
#include "ssg_device.h"

namespace boom_amd {

namespace {

struct ArSpikeLds {
  double X[AR_MAX * AR_MAX];    // xtx
  double O[AR_MAX * AR_MAX];    // the slab's precision
  double A[AR_MAX * AR_MAX];    // a selected sub-matrix
  double Lc[AR_MAX * AR_MAX];   // its Cholesky factor
  int idx[AR_MAX];              // the k-th included lag
};

// the included lags, in order, into W.idx; returns how many
__device__ __forceinline__ int asp_compact(ArSpikeLds &W, unsigned mask, int lane) {
  wave_lds_sync();   // (the last selection's readers are done)
  if (lane < AR_MAX && ((mask >> lane) & 1u)) W.idx[__popc(mask & ((1u << lane) - 1u))] = lane;
  wave_lds_sync();
  return __popc(mask);
}
// lane k < n: component idx[k] of a vector held by lag
__device__ __forceinline__ double asp_select(const ArSpikeLds &W, double v, int n, int lane) {
  const double s = __shfl(v, lane < n ? W.idx[lane] : 0);
  return lane < n ? s : 0.0;
}
// A = O_gamma [+ X_gamma / sigsq]
__device__ __forceinline__ void asp_fill(ArSpikeLds &W, int n, bool data, double sigsq, int lane) {
  wave_lds_sync();
  for (int e = lane; e < n * n; e += WAVE) {
    const int r = e / n, c = e - r * n;
    const int at = W.idx[r] * AR_MAX + W.idx[c];
    double a = W.O[at];
    if (data) a += W.X[at] / sigsq;
    W.A[r * AR_MAX + c] = a;
  }
  wave_lds_sync();
}
// sum_k log Lc[k][k]
__device__ __forceinline__ double asp_sum_log_diag(const ArSpikeLds &W, int n, int lane) {
  return row_total(lane < n ? log(W.Lc[lane * AR_MAX + lane]) : 0.0);
}
// A v for a selected vector (lane k < n)
__device__ __forceinline__ double asp_matvec(const ArSpikeLds &W, double v, int n, int lane) {
  double acc = 0.0;
  for (int j = 0; j < n; ++j) {
    const double vj = rl(v, j);
    if (lane < n) acc += W.A[lane * AR_MAX + j] * vj;
  }
  return acc;
}

// VariableSelectionPrior::logp
__device__ __forceinline__ double asp_spike_logp(const ArSpikePrior &R, unsigned mask, int L) {
  double ans = 0.0;
  for (int i = 0; i < L; ++i) {
    ans += ((mask >> i) & 1u) ? R.log_pi[i] : R.log_1mpi[i];
    if (!isfinite(ans)) return -__builtin_inf();
  }
  return ans;
}

// SpikeSlabSampler::log_model_prob; mu_l, xty_l: the lane's lag
__device__ __forceinline__ double asp_log_model_prob(ArSpikeLds &W, const ArSpikePrior &R, unsigned mask, int L,
                                                     double mu_l, double xty_l, double sigsq, int lane) {
  double numerator = asp_spike_logp(R, mask, L);
  if (numerator == -__builtin_inf() || mask == 0u) return numerator;
  const int n = asp_compact(W, mask, lane);
  asp_fill(W, n, false, sigsq, lane);
  if (!ar_chol(W.A, 1.0, W.Lc, n, lane)) return -__builtin_inf();   // (logdet of a matrix that is not positive definite)
  wave_lds_sync();
  numerator += .5 * (2.0 * asp_sum_log_diag(W, n, lane));
  if (numerator == -__builtin_inf()) return numerator;
  const double mu = asp_select(W, mu_l, n, lane);
  const double precision_mu = asp_matvec(W, mu, n, lane);
  numerator -= .5 * row_total(lane < n ? mu * precision_mu : 0.0);
  asp_fill(W, n, true, sigsq, lane);
  if (!ar_chol(W.A, 1.0, W.Lc, n, lane)) return -__builtin_inf();
  wave_lds_sync();
  double denominator = asp_sum_log_diag(W, n, lane);
  const double S = asp_select(W, xty_l, n, lane) / sigsq + precision_mu;
  const double s = ar_lsolve(W.Lc, S, n, lane);
  denominator -= .5 * row_total(lane < n ? s * s : 0.0);
  return numerator - denominator;
}

// ArSpikeSlabSampler::shrink_phi on a selected vector: check_stationary of the SELECTED vector
__device__ __forceinline__ bool asp_shrink(double &phi, int n, int lane) {
  int attempts = 0;
  const int max_attempts = 20;
  while (attempts++ < max_attempts && !ar_stationary(phi, n, lane)) phi *= .95;
  return attempts < max_attempts;
}

}  // namespace

__global__ __launch_bounds__(64) void ar_spike_kernel(SsParams P, ArSpikeParams U) {
  const int chain = (int)(blockIdx.x / (unsigned)U.nspike) + P.chain_first, lane = (int)threadIdx.x;
  const int which = (int)(blockIdx.x % (unsigned)U.nspike);
  if ((int)(blockIdx.x / (unsigned)U.nspike) >= P.chain_count) return;
  // (a chain with several such blocks: a sibling wave may be writing a failure status while this one
  // reads it, so whether this block is still drawn in the failing round depends on timing -- the
  // chain is stopped either way and nothing reads its draws)
  if (P.status[chain] != CHAIN_OK) return;
  if (P.only_ran && P.only_ran[chain] == 0) return;
  __shared__ ArSpikeLds W;
  const SsmParams &M = P.ssm;
  const SsgSpec &Q = *M.spec;
  const SsgBlock &K = Q.blk[U.block[which]];
  const ArSpikePrior &R = U.prior[K.ar_index];
  const int L = K.lags, vi = K.var0;
  const size_t at = (size_t)chain * SSG_MAX_VAR + vi;
  const size_t slot = (size_t)chain * SSG_MAX_AR + K.ar_index;
  double *gphi = M.ar_phi + slot * AR_MAX;
  uint8_t *ggam = U.gamma + slot * AR_MAX;
  const double *suf = M.ar_suf + slot * AR_SUF_STRIDE;
  for (int e = lane; e < AR_MAX * AR_MAX; e += WAVE) {
    W.X[e] = suf[e];
    W.O[e] = R.siginv[e];
  }
  const double xty = (lane < L) ? suf[AR_SUF_XTY + lane] : 0.0;
  const double yty = suf[AR_SUF_YTY], nobs = suf[AR_SUF_N];
  const double mu = (lane < L) ? R.mu[lane] : 0.0;
  const double phi0 = (lane < L) ? gphi[lane] : 0.0;
  double sigsq = M.var_sigsq[at];
  unsigned mask = (unsigned)__ballot(lane < L && ggam[lane < L ? lane : 0] != 0) & 0xffffu;
  SeqRng rng{PhiloxKey{P.seed_lo, P.seed_hi, (uint32_t)(P.chain_offset + chain), (uint32_t)K.sid[0]}, M.pos_var[at]};
  wave_lds_sync();
  int status = CHAIN_OK;

  // ---- draw_model_indicators
  if (R.select) {
    int order = lane;   // lane i: indx[i]
    for (int i = L - 1; i > 0; --i) {
      const int j = d_random_int(rng, 0, i);
      if (j != i) {
        const int oi = __shfl(order, i), oj = __shfl(order, j);
        if (lane == i) order = oj;
        if (lane == j) order = oi;
      }
    }
    double logp = asp_log_model_prob(W, R, mask, L, mu, xty, sigsq, lane);
    if (!isfinite(logp)) {
      // make_valid
      for (int i = 0; i < L; ++i) {
        if (R.pi[i] <= 0.0 && ((mask >> i) & 1u)) mask ^= 1u << i;
        if (R.pi[i] >= 1.0 && !((mask >> i) & 1u)) mask ^= 1u << i;
      }
      logp = asp_log_model_prob(W, R, mask, L, mu, xty, sigsq, lane);
    }
    if (!isfinite(logp)) {
      status = CHAIN_ILLEGAL_START;
    } else {
      int nflips = L;
      if (R.max_flips > 0) nflips = min(nflips, R.max_flips);
      for (int i = 0; i < nflips; ++i) {
        const int v = __builtin_amdgcn_readfirstlane(__shfl(order, i));
        const unsigned cand = mask ^ (1u << v);
        const double logp_new = asp_log_model_prob(W, R, cand, L, mu, xty, sigsq, lane);
        const double u = d_runif(rng, 0.0, 1.0);
        if (!(log(u) > logp_new - logp)) {
          mask = cand;
          logp = logp_new;
        }
      }
    }
  }

  // ---- draw_phi; set_inc has zeroed the coefficients that left the model
  const bool inc = lane < L && ((mask >> lane) & 1u);
  const double original = inc ? phi0 : 0.0;
  double phi = original;
  const int n = __popc(mask);
  if (status == CHAIN_OK && n > 0) {
    asp_compact(W, mask, lane);
    asp_fill(W, n, false, sigsq, lane);
    const double pmu = asp_matvec(W, asp_select(W, mu, n, lane), n, lane) + asp_select(W, xty, n, lane) / sigsq;
    asp_fill(W, n, true, sigsq, lane);
    if (!ar_chol(W.A, 1.0, W.Lc, n, lane)) {
      status = CHAIN_NOT_PD;
    } else {
      wave_lds_sync();
      const double mean = ar_ltsolve(W.Lc, ar_lsolve(W.Lc, pmu, n, lane), n, lane);   // (by selected position)
      const int rank = __popc(mask & ((1u << (lane & 15)) - 1u));
      bool ok = false;
      for (int attempt = 0; attempt < 100 && !ok; ++attempt) {
        double z = 0.0;
        for (int i = 0; i < n; ++i) {
          const double zi = d_rnorm(rng, 0.0, 1.0);
          if (lane == i) z = zi;
        }
        const double draw = ar_ltsolve(W.Lc, z, n, lane) + mean;
        const double full = __shfl(draw, rank);
        const double cand = inc ? full : 0.0;
        if (!isfinite(row_total(inc ? cand : 0.0))) { status = AR_SPIKE_BAD_DRAW; break; }
        ok = !R.truncate || ar_stationary(cand, L, lane);
        if (ok) phi = cand;
      }
      if (!ok && status == CHAIN_OK) {
        // draw_phi_univariate, on the selected vector; an error inside leaves the original phi
        double ph = asp_select(W, original, n, lane);
        bool fine = true;
        if (!ar_stationary(original, L, lane)) fine = asp_shrink(ph, n, lane);
        for (int i = 0; i < n && fine; ++i) {
          if (n == 1) continue;
          // coefficient i given the others under N(mean, A^-1): the swept precision's row
          const double pii = W.A[i * AR_MAX + i];
          const double beta = (lane < n && lane != i) ? -W.A[i * AR_MAX + lane] / pii : 0.0;
          const double cmean = row_total(beta * (ph - mean)) + rl(mean, i);
          const double csd = sqrt(-1.0 / -pii);
          const double initial_phi = rl(ph, i);
          double lo = -1, hi = 1;
          int attempts = 0;
          for (;;) {
            if (attempts++ > 1000) { fine = false; break; }
            int bad = 0;
            const double candidate = ar_rtrun_norm_2(rng, cmean, csd, lo, hi, &bad);
            if (bad) { fine = false; break; }
            if (lane == i) ph = candidate;
            const double full = __shfl(ph, rank);
            if (ar_stationary(inc ? full : 0.0, L, lane)) break;
            if (candidate > initial_phi) hi = candidate; else lo = candidate;
          }
        }
        if (fine) {
          const double full = __shfl(ph, rank);
          phi = inc ? full : 0.0;
        } else {
          phi = original;
        }
      }
    }
  }

  // ---- draw_sigma_full_conditional
  if (status == CHAIN_OK) {
    double ss = yty;
    if (n > 0) {
      // RegSuf::relative_sse(GlmCoefs): yty + (phi'xtx phi - 2 phi'xty) over the included coefficients
      double row = 0.0;
      for (int j = 0; j < L; ++j) {
        const double pj = rl(phi, j);
        if (lane < L) row += W.X[lane * AR_MAX + j] * pj;
      }
      const double quad = row_total((lane < L) ? phi * row : 0.0);
      const double lin = row_total((lane < L) ? phi * xty : 0.0);
      ss = yty + (quad - 2 * lin);
    }
    int bad = 0;
    sigsq = d_draw_variance(rng, nobs + Q.prior_df[vi], ss + Q.prior_ss[vi], Q.sigma_max[vi], &bad);
    if (bad) status = CHAIN_RNG_BRANCH;
    else if (!isfinite(sigsq)) status = AR_SPIKE_BAD_DRAW;
  }
  if (status != CHAIN_OK) {
    if (lane == 0) P.status[chain] = status;
    return;
  }
  if (lane < L) {
    gphi[lane] = phi;
    ggam[lane] = inc ? 1 : 0;
  }
  if (lane == 0) {
    M.var_sigsq[at] = sigsq;
    M.pos_var[at] = rng.pos;
  }
}

hipError_t launch_ar_spike(hipStream_t stream, const SsParams &P, const ArSpikeParams &U) {
  KtScope kt(stream, KT_SS_AUTOAR);
  hipLaunchKernelGGL(ar_spike_kernel, dim3((unsigned)(P.chain_count * U.nspike)), dim3(64), 0, stream, P, U);
  return hipGetLastError();
}

}  // namespace boom_amd
