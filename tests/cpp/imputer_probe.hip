// Test-only probe of the GLM imputation kernels, for tests/test_imputer_kernels_gpu.py.
//
// This file includes the product's probit_kernel.hip itself -- the kernels launched here are
// the product's, compiled with the product's flags, and nothing of them is restated:
//   probit_impute_kernel, logit_impute_kernel<false|true>, logit_pg_impute_kernel,
//   poisson_impute_kernel<false|true>, latent_ss_h_kernel, latent_ss_suf_kernel.
// The file's host launchers refer to four functions of the product library (the kernel timer's
// two and two GEMM launchers); the probe never calls those launchers, and the four names are
// resolved by stubs below, so nothing of the product library is linked.
//
// One exported entry point per kernel instance, all with the same arguments: the fields of
// ProbitParams as plain values and host arrays with explicit lengths (in elements).  Every
// entry point checks ON THE HOST that every index the kernel will form is in range
// (IP_BAD_REQUEST instead of a launch where one is not), allocates device buffers of exactly
// those lengths, copies everything in -- the outputs too, which the caller has filled with a
// sentinel and extended by guard bands --, launches with the product's geometry (grid
// ((n + 255) / 256, chains), block 256) on the null stream, synchronises, copies every
// writable buffer back whole and returns the hipError_t.
//
// z, w, value, h: `nout` doubles each, the chains x n block starts `guard` elements in.
#include "../../boom_amd/csrc/probit_kernel.hip"

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "probe_dev.h"

namespace boom_amd {
// (never called: the probe launches the kernels itself)
void kt_mark(hipStream_t, int, bool) {}
bool kt_active() { return false; }
hipError_t launch_rows_times_columns(hipStream_t, const double *, int, const double *, int64_t, int, const double *,
                                     double *, double *) {
  return hipErrorNotSupported;
}
hipError_t launch_latent_products(hipStream_t, const double *, const double *, int, const double *, const double *,
                                  int64_t, int, const double *, double *, double *, double *) {
  return hipErrorNotSupported;
}
}  // namespace boom_amd

using namespace boom_amd;

namespace {

enum : int { IP_BAD_REQUEST = -1 };
enum Kind : int { K_PROBIT, K_LOGIT, K_LOGIT_SS, K_PG, K_POISSON, K_POISSON_SS, K_SS_H, K_SS_SUF };

#define IP_ARGS                                                                                                     \
  int n, int p, int chains, int slot_limit, int64_t chain_offset, const double *X, size_t nX, const uint8_t *gamma, \
      const double *beta, size_t ngb, uint32_t seed_lo, uint32_t seed_hi, uint64_t sweep, int32_t *status,          \
      size_t nstatus, int clt_threshold, const double *y, const double *ntrials, size_t ny,                         \
      const int32_t *mix_off, size_t nmix, const double *mix_mu, const double *mix_sigma, const double *mix_logw,   \
      size_t ncomp, const int32_t *obs_mix, int mix_one, const uint8_t *observed, const double *offset,             \
      size_t noffset, int64_t offset_stride, double *z, double *w, double *value, double *h, size_t nout,           \
      size_t guard
#define IP_PASS                                                                                                   \
  n, p, chains, slot_limit, chain_offset, X, nX, gamma, beta, ngb, seed_lo, seed_hi, sweep, status, nstatus,      \
      clt_threshold, y, ntrials, ny, mix_off, nmix, mix_mu, mix_sigma, mix_logw, ncomp, obs_mix, mix_one,         \
      observed, offset, noffset, offset_stride, z, w, value, h, nout, guard

// mix_off: nmix + 1 offsets into ncomp components
int run(Kind kind, IP_ARGS) {
  const bool ss = kind == K_LOGIT_SS || kind == K_POISSON_SS || kind == K_SS_H || kind == K_SS_SUF;
  const bool poisson = kind == K_POISSON || kind == K_POISSON_SS;
  const bool draws = kind != K_SS_H && kind != K_SS_SUF;
  if (n < 1 || p < 1 || chains < 1 || chains > 65535 || clt_threshold < 0 || clt_threshold > 64) return IP_BAD_REQUEST;
  const size_t cn = (size_t)chains * (size_t)n;
  if (!X || !gamma || !beta || !status || !y || !ntrials || !z || !w || !value || !h) return IP_BAD_REQUEST;
  if (nX < (size_t)n * (size_t)p || ngb < (size_t)chains * (size_t)p || nstatus < (size_t)chains || ny < (size_t)n ||
      nout < 2 * guard + cn)
    return IP_BAD_REQUEST;
  if (draws) {
    for (int i = 0; i < n; ++i) {
      if (!std::isfinite(y[i]) || !std::isfinite(ntrials[i]) || y[i] < 0 || ntrials[i] < 0 || y[i] > 1e6 ||
          ntrials[i] > 1e6)
        return IP_BAD_REQUEST;
      if (!poisson && y[i] > ntrials[i]) return IP_BAD_REQUEST;
    }
  }
  if (poisson) {
    if (!mix_off || !mix_mu || !mix_sigma || !mix_logw || !obs_mix || nmix < 1 || mix_one < 0 ||
        (size_t)mix_one >= nmix)
      return IP_BAD_REQUEST;
    for (size_t m = 0; m < nmix; ++m) {
      const int64_t c0 = mix_off[m], c1 = mix_off[m + 1];
      if (c0 < 0 || c1 <= c0 || c1 - c0 > POISSON_MAX_COMP || (size_t)c1 > ncomp) return IP_BAD_REQUEST;
    }
    for (int i = 0; i < n; ++i)
      if (obs_mix[i] < -1 || (obs_mix[i] >= 0 && (size_t)obs_mix[i] >= nmix)) return IP_BAD_REQUEST;
  }
  if (ss) {
    if (!observed || !offset || offset_stride < n || noffset < (size_t)(chains - 1) * (size_t)offset_stride + (size_t)n)
      return IP_BAD_REQUEST;
  }
  Dev<double> dX(X, nX), dB(beta, ngb), dY(y, ny), dN(ntrials, ny), dZ(z, nout), dW(w, nout), dV(value, nout),
      dH(h, nout), dMu(poisson ? mix_mu : nullptr, ncomp), dSg(poisson ? mix_sigma : nullptr, ncomp),
      dLw(poisson ? mix_logw : nullptr, ncomp), dOff(ss ? offset : nullptr, noffset);
  Dev<uint8_t> dG(gamma, ngb), dObs(ss ? observed : nullptr, ny);
  Dev<int32_t> dS(status, nstatus), dMo(poisson ? mix_off : nullptr, nmix + 1), dOm(poisson ? obs_mix : nullptr, ny);
  IP_TRY(dX.err); IP_TRY(dB.err); IP_TRY(dY.err); IP_TRY(dN.err); IP_TRY(dZ.err); IP_TRY(dW.err); IP_TRY(dV.err);
  IP_TRY(dH.err); IP_TRY(dMu.err); IP_TRY(dSg.err); IP_TRY(dLw.err); IP_TRY(dOff.err); IP_TRY(dG.err);
  IP_TRY(dObs.err); IP_TRY(dS.err); IP_TRY(dMo.err); IP_TRY(dOm.err);
  ProbitParams P{};
  P.n = n; P.p = p; P.chains = chains; P.slot_limit = slot_limit; P.chain_offset = chain_offset;
  P.X = dX.ptr; P.gamma = dG.ptr; P.beta = dB.ptr;
  P.z = dZ.ptr + guard; P.w = dW.ptr + guard;
  P.seed_lo = seed_lo; P.seed_hi = seed_hi; P.sweep = sweep; P.status = dS.ptr;
  P.clt_threshold = clt_threshold; P.y = dY.ptr; P.ntrials = dN.ptr; P.xtz = nullptr;
  P.mix_off = dMo.ptr; P.mix_mu = dMu.ptr; P.mix_sigma = dSg.ptr; P.mix_logw = dLw.ptr; P.obs_mix = dOm.ptr;
  P.mix_one = mix_one;
  P.observed = dObs.ptr; P.offset = dOff.ptr; P.offset_stride = offset_stride;
  P.value = dV.ptr + guard; P.h = dH.ptr + guard;
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)chains), block(256);
  switch (kind) {
    case K_PROBIT: hipLaunchKernelGGL(probit_impute_kernel, grid, block, 0, nullptr, P); break;
    case K_LOGIT: hipLaunchKernelGGL(logit_impute_kernel<false>, grid, block, 0, nullptr, P); break;
    case K_LOGIT_SS: hipLaunchKernelGGL(logit_impute_kernel<true>, grid, block, 0, nullptr, P); break;
    case K_PG: hipLaunchKernelGGL(logit_pg_impute_kernel, grid, block, 0, nullptr, P); break;
    case K_POISSON: hipLaunchKernelGGL(poisson_impute_kernel<false>, grid, block, 0, nullptr, P); break;
    case K_POISSON_SS: hipLaunchKernelGGL(poisson_impute_kernel<true>, grid, block, 0, nullptr, P); break;
    case K_SS_H:   // (clt_threshold: 0 the Poisson family's missing variance, else the logit family's)
      hipLaunchKernelGGL(latent_ss_h_kernel, grid, block, 0, nullptr, P,
                         clt_threshold ? LOGIT_MISSING_VARIANCE : POISSON_MISSING_VARIANCE);
      break;
    case K_SS_SUF: hipLaunchKernelGGL(latent_ss_suf_kernel, grid, block, 0, nullptr, P); break;
  }
  IP_TRY(hipGetLastError());
  IP_TRY(hipDeviceSynchronize());
  IP_TRY(dZ.back()); IP_TRY(dW.back()); IP_TRY(dV.back()); IP_TRY(dH.back());
  return (int)dS.back();
}

}  // namespace

extern "C" {

int ip_chain_ok() { return CHAIN_OK; }
int ip_chain_rng_branch() { return CHAIN_RNG_BRANCH; }
int ip_chain_model_too_large() { return CHAIN_MODEL_TOO_LARGE; }
int ip_chain_forecast_variance() { return CHAIN_FORECAST_VARIANCE; }
int ip_kmax() { return PROBIT_KMAX; }
double ip_logit_missing_variance() { return LOGIT_MISSING_VARIANCE; }
double ip_poisson_missing_variance() { return POISSON_MISSING_VARIANCE; }

int ip_probit(IP_ARGS) { return run(K_PROBIT, IP_PASS); }
int ip_logit(IP_ARGS) { return run(K_LOGIT, IP_PASS); }
int ip_logit_ss(IP_ARGS) { return run(K_LOGIT_SS, IP_PASS); }
int ip_logit_pg(IP_ARGS) { return run(K_PG, IP_PASS); }
int ip_poisson(IP_ARGS) { return run(K_POISSON, IP_PASS); }
int ip_poisson_ss(IP_ARGS) { return run(K_POISSON_SS, IP_PASS); }
// latent_ss_h_kernel: clt_threshold chooses the family (0 Poisson, else logit); reads w
int ip_latent_ss_h(IP_ARGS) { return run(K_SS_H, IP_PASS); }
// latent_ss_suf_kernel: reads value, offset and w
int ip_latent_ss_suf(IP_ARGS) { return run(K_SS_SUF, IP_PASS); }

}  // extern "C"
