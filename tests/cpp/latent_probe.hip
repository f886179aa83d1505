// Test-only probe of the Student, quantile and multinomial logit latent-data kernels, for
// tests/test_latent_kernels_gpu.py.
//
// This file includes the product's student_kernel.hip, quantile_kernel.hip and mlogit_kernel.hip
// themselves -- the kernels launched here are the product's, compiled with the product's flags,
// and nothing of them is restated:
//   student_impute_kernel<false|true>, student_ss_h_kernel, student_ss_suf_kernel,
//   student_sigma_nu_kernel<false|true>, quantile_impute_kernel, mlogit_expand_kernel,
//   mlogit_impute_kernel, mlogit_wss_kernel.
// The files' host launchers refer to three functions of the product library (the kernel timer's
// two and one GEMM launcher); the probe never calls those launchers, and the three names are
// resolved by stubs below, so nothing of the product library is linked.
//
// One exported entry point per kernel instance, as imputer_probe.hip has them: the fields of the
// family's parameter struct as plain values and host arrays with explicit lengths (in elements).
// Every entry point checks ON THE HOST that every index the kernel will form is in range
// (LP_BAD_REQUEST instead of a launch where one is not), allocates device buffers of exactly
// those lengths, copies everything in -- the outputs too, which the caller has filled with a
// sentinel and extended by guard bands --, launches with the product's geometry on the null
// stream, synchronises, copies every writable buffer back whole and returns the hipError_t.
//
// Per-row arrays (z, w, u, h, X, Xsq): `nout` doubles each, the block the kernel addresses starts
// `guard` elements in.  Per-chain arrays (status, sigsq, nu, dx, margin, trace rows, acc, wss,
// wss_part) start at element 0 and are followed by their guard band.
#include "../../boom_amd/csrc/student_kernel.hip"
#include "../../boom_amd/csrc/quantile_kernel.hip"
#include "../../boom_amd/csrc/mlogit_kernel.hip"

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "probe_dev.h"

namespace boom_amd {
// (never called: the probe launches the kernels itself)
void kt_mark(hipStream_t, int, bool) {}
bool kt_active() { return false; }
hipError_t launch_latent_products(hipStream_t, const double *, const double *, int, const double *, const double *,
                                  int64_t, int, const double *, double *, double *, double *) {
  return hipErrorNotSupported;
}
}  // namespace boom_amd

using namespace boom_amd;

namespace {

enum : int { LP_BAD_REQUEST = -1 };

// the common head of the three parameter structs, as plain values
#define LP_HEAD                                                                                                    \
  int n, int p, int chains, int slot_limit, int64_t chain_offset, const double *X, size_t nX, const uint8_t *gamma, \
      const double *beta, size_t ngb, uint32_t seed_lo, uint32_t seed_hi, uint64_t sweep, int32_t *status,         \
      size_t nstatus
#define LP_HEAD_PASS n, p, chains, slot_limit, chain_offset, X, nX, gamma, beta, ngb, seed_lo, seed_hi, sweep, status, nstatus

// rows: the rows of X per observation index (1; the multinomial logit's M)
bool head_ok(LP_HEAD, size_t rows) {
  if (n < 1 || p < 1 || chains < 1 || chains > 65535 || rows < 1) return false;
  if (!X || !gamma || !beta || !status) return false;
  return nX >= (size_t)n * rows * (size_t)p && ngb >= (size_t)chains * (size_t)p && nstatus >= (size_t)chains;
}

void fill_head(LatentParams &P, LP_HEAD, const double *dX, const uint8_t *dG, const double *dB, int32_t *dS) {
  (void)X; (void)nX; (void)gamma; (void)beta; (void)ngb; (void)status; (void)nstatus;
  P.n = n; P.p = p; P.chains = chains; P.slot_limit = slot_limit; P.chain_offset = chain_offset;
  P.X = dX; P.gamma = dG; P.beta = dB;
  P.seed_lo = seed_lo; P.seed_hi = seed_hi; P.sweep = sweep; P.status = dS;
}

// ---- Student ---------------------------------------------------------------------------------------
enum StudentKind : int { S_IMPUTE, S_IMPUTE_SS, S_SS_H, S_SS_SUF, S_SIGMA_NU, S_SIGMA_NU_SS };

// sigsq, nu, dx, margin: nchain doubles each; observed: nobserved; trace_idx: ntidx; trace_sigsq,
// trace_nu: ntrace each (chains x trace_stride, then the guard); acc: nacc (chains x ACC_COUNT, then the guard) or null
#define LP_STUDENT_ARGS                                                                                            \
  LP_HEAD, const double *y, size_t ny, double *sigsq, double *nu, double *dx, double *margin, size_t nchain,       \
      double prior_df, double prior_ss, double sigma_max, int nu_kind, double nu_a, double nu_b,                   \
      const uint8_t *observed, size_t nobserved, const double *offset, size_t noffset, int64_t offset_stride,       \
      double *z, double *w, double *u, double *h, size_t nout, size_t guard, const int32_t *trace_idx,             \
      size_t ntidx, double *trace_sigsq, double *trace_nu, size_t ntrace, int trace_stride, double *acc,           \
      size_t nacc
#define LP_STUDENT_PASS                                                                                            \
  LP_HEAD_PASS, y, ny, sigsq, nu, dx, margin, nchain, prior_df, prior_ss, sigma_max, nu_kind, nu_a, nu_b, observed, \
      nobserved, offset, noffset, offset_stride, z, w, u, h, nout, guard, trace_idx, ntidx, trace_sigsq, trace_nu, \
      ntrace, trace_stride, acc, nacc

int run_student(StudentKind kind, LP_STUDENT_ARGS) {
  const bool ss = kind == S_IMPUTE_SS || kind == S_SS_H || kind == S_SS_SUF || kind == S_SIGMA_NU_SS;
  const bool sn = kind == S_SIGMA_NU || kind == S_SIGMA_NU_SS;
  if (!head_ok(LP_HEAD_PASS, 1)) return LP_BAD_REQUEST;
  const size_t cn = (size_t)chains * (size_t)n;
  if (!y || !sigsq || !nu || !dx || !margin || !z || !w || !u || !h) return LP_BAD_REQUEST;
  if (ny < (size_t)n || nchain < (size_t)chains || nout < 2 * guard + cn) return LP_BAD_REQUEST;
  if (nu_kind != STUDENT_NU_UNIFORM && nu_kind != STUDENT_NU_GAMMA) return LP_BAD_REQUEST;
  if (ss) {
    if (!observed || nobserved < (size_t)n || !offset || offset_stride < n ||
        noffset < (size_t)(chains - 1) * (size_t)offset_stride + (size_t)n)
      return LP_BAD_REQUEST;
  }
  if (trace_stride < 0) return LP_BAD_REQUEST;
  if (sn && trace_stride > 0) {
    // (the kernel itself keeps the row inside [0, trace_stride))
    if (!trace_idx || ntidx < (size_t)chains || !trace_sigsq || !trace_nu ||
        ntrace < (size_t)chains * (size_t)trace_stride)
      return LP_BAD_REQUEST;
  }
  if (sn && acc && nacc < (size_t)chains * (size_t)ACC_COUNT) return LP_BAD_REQUEST;
  Dev<double> dX(X, nX), dB(beta, ngb), dY(y, ny), dSig(sigsq, nchain), dNu(nu, nchain), dDx(dx, nchain),
      dMg(margin, nchain), dOff(ss ? offset : nullptr, noffset), dZ(z, nout), dW(w, nout), dU(u, nout), dH(h, nout),
      dTs(sn && trace_stride > 0 ? trace_sigsq : nullptr, ntrace), dTn(sn && trace_stride > 0 ? trace_nu : nullptr, ntrace),
      dAcc(sn ? acc : nullptr, nacc);
  Dev<uint8_t> dG(gamma, ngb), dObs(ss ? observed : nullptr, nobserved);
  Dev<int32_t> dS(status, nstatus), dTi(sn && trace_stride > 0 ? trace_idx : nullptr, ntidx);
  IP_TRY(dX.err); IP_TRY(dB.err); IP_TRY(dY.err); IP_TRY(dSig.err); IP_TRY(dNu.err); IP_TRY(dDx.err); IP_TRY(dMg.err);
  IP_TRY(dOff.err); IP_TRY(dZ.err); IP_TRY(dW.err); IP_TRY(dU.err); IP_TRY(dH.err); IP_TRY(dTs.err); IP_TRY(dTn.err);
  IP_TRY(dAcc.err); IP_TRY(dG.err); IP_TRY(dObs.err); IP_TRY(dS.err); IP_TRY(dTi.err);
  StudentParams P{};
  fill_head(P, LP_HEAD_PASS, dX.ptr, dG.ptr, dB.ptr, dS.ptr);
  P.z = dZ.ptr + guard; P.w = dW.ptr + guard; P.u = dU.ptr + guard; P.h = dH.ptr + guard;
  P.prior_df = prior_df; P.prior_ss = prior_ss; P.sigma_max = sigma_max;
  P.nu_kind = nu_kind; P.nu_a = nu_a; P.nu_b = nu_b;
  P.y = dY.ptr; P.sigsq = dSig.ptr; P.nu = dNu.ptr; P.dx = dDx.ptr; P.margin = dMg.ptr;
  P.trace_idx = dTi.ptr; P.trace_sigsq = dTs.ptr; P.trace_nu = dTn.ptr; P.trace_stride = sn ? trace_stride : 0;
  P.acc = dAcc.ptr;
  P.offset = dOff.ptr; P.offset_stride = offset_stride; P.observed = dObs.ptr;
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)chains), block(256);
  switch (kind) {
    case S_IMPUTE: hipLaunchKernelGGL(student_impute_kernel<false>, grid, block, 0, nullptr, P); break;
    case S_IMPUTE_SS: hipLaunchKernelGGL(student_impute_kernel<true>, grid, block, 0, nullptr, P); break;
    case S_SS_H: hipLaunchKernelGGL(student_ss_h_kernel, grid, block, 0, nullptr, P); break;
    case S_SS_SUF: hipLaunchKernelGGL(student_ss_suf_kernel, grid, block, 0, nullptr, P); break;
    case S_SIGMA_NU:
      hipLaunchKernelGGL(student_sigma_nu_kernel<false>, dim3((unsigned)chains), dim3(STUDENT_SN_BLOCK), 0, nullptr, P);
      break;
    case S_SIGMA_NU_SS:
      hipLaunchKernelGGL(student_sigma_nu_kernel<true>, dim3((unsigned)chains), dim3(STUDENT_SN_BLOCK), 0, nullptr, P);
      break;
  }
  IP_TRY(hipGetLastError());
  IP_TRY(hipDeviceSynchronize());
  IP_TRY(dZ.back()); IP_TRY(dW.back()); IP_TRY(dU.back()); IP_TRY(dH.back());
  IP_TRY(dSig.back()); IP_TRY(dNu.back()); IP_TRY(dDx.back()); IP_TRY(dMg.back());
  IP_TRY(dTs.back()); IP_TRY(dTn.back()); IP_TRY(dAcc.back());
  return (int)dS.back();
}

// ---- multinomial logit ----------------------------------------------------------------------------
// mix: the five vectors of MlogitParams in its order (mu, sd, prec, logw, logsd), MLOGIT_NCOMP each
#define LP_MLOGIT_ARGS                                                                                             \
  LP_HEAD, int nchoices, const int32_t *y, size_t ny, const double *mix, size_t nmix, double *u, double *w,        \
      double *z, size_t nout, size_t guard, double *wss_part, size_t npart, double *wss, size_t nwss
#define LP_MLOGIT_PASS LP_HEAD_PASS, nchoices, y, ny, mix, nmix, u, w, z, nout, guard, wss_part, npart, wss, nwss

int run_mlogit(bool impute, LP_MLOGIT_ARGS) {
  if (nchoices < 2 || nchoices > MLOGIT_MAX_CHOICES) return LP_BAD_REQUEST;
  if (!head_ok(LP_HEAD_PASS, (size_t)nchoices)) return LP_BAD_REQUEST;
  const size_t cN = (size_t)chains * (size_t)n * (size_t)nchoices;
  const int nblocks = (n + 255) / 256;
  if (!y || !mix || !u || !w || !z || !wss_part || !wss) return LP_BAD_REQUEST;
  if (ny < (size_t)n || nmix != 5 * (size_t)MLOGIT_NCOMP || nout < 2 * guard + cN ||
      npart < (size_t)chains * (size_t)nblocks || nwss < (size_t)chains)
    return LP_BAD_REQUEST;
  for (int i = 0; i < n; ++i)
    if (y[i] < 0 || y[i] >= nchoices) return LP_BAD_REQUEST;
  Dev<double> dX(X, nX), dB(beta, ngb), dU(u, nout), dW(w, nout), dZ(z, nout), dPart(wss_part, npart), dWss(wss, nwss);
  Dev<uint8_t> dG(gamma, ngb);
  Dev<int32_t> dS(status, nstatus), dY(y, ny);
  IP_TRY(dX.err); IP_TRY(dB.err); IP_TRY(dU.err); IP_TRY(dW.err); IP_TRY(dZ.err); IP_TRY(dPart.err); IP_TRY(dWss.err);
  IP_TRY(dG.err); IP_TRY(dS.err); IP_TRY(dY.err);
  MlogitParams P{};
  fill_head(P, LP_HEAD_PASS, dX.ptr, dG.ptr, dB.ptr, dS.ptr);
  P.z = dZ.ptr + guard; P.w = dW.ptr + guard; P.u = dU.ptr + guard;
  P.nchoices = nchoices; P.y = dY.ptr; P.wss_part = dPart.ptr; P.wss = dWss.ptr;
  for (int c = 0; c < MLOGIT_NCOMP; ++c) {
    P.mix_mu[c] = mix[c]; P.mix_sd[c] = mix[MLOGIT_NCOMP + c]; P.mix_prec[c] = mix[2 * MLOGIT_NCOMP + c];
    P.mix_logw[c] = mix[3 * MLOGIT_NCOMP + c]; P.mix_logsd[c] = mix[4 * MLOGIT_NCOMP + c];
  }
  if (impute)
    hipLaunchKernelGGL(mlogit_impute_kernel, dim3((unsigned)nblocks, (unsigned)chains), dim3(256), 0, nullptr, P);
  else
    hipLaunchKernelGGL(mlogit_wss_kernel, dim3((unsigned)((chains + 255) / 256)), dim3(256), 0, nullptr, P, nblocks);
  IP_TRY(hipGetLastError());
  IP_TRY(hipDeviceSynchronize());
  IP_TRY(dU.back()); IP_TRY(dW.back()); IP_TRY(dZ.back()); IP_TRY(dPart.back()); IP_TRY(dWss.back());
  return (int)dS.back();
}

}  // namespace

extern "C" {

int lp_chain_ok() { return CHAIN_OK; }
int lp_chain_rng_branch() { return CHAIN_RNG_BRANCH; }
int lp_chain_model_too_large() { return CHAIN_MODEL_TOO_LARGE; }
int lp_student_slice_error() { return STUDENT_SLICE_ERROR; }
int lp_student_bad_weight() { return STUDENT_BAD_WEIGHT; }
int lp_quantile_weight_error() { return QUANTILE_WEIGHT_ERROR; }
int lp_mlogit_impute_error() { return MLOGIT_IMPUTE_ERROR; }
int lp_kmax(int family) { return family == 0 ? STUDENT_KMAX : family == 1 ? QUANTILE_KMAX : MLOGIT_KMAX; }
int lp_stream(int which) {
  return which == 0 ? (int)STUDENT_IMPUTE_STREAM : which == 1 ? (int)STUDENT_SN_STREAM
       : which == 2 ? (int)QUANTILE_IMPUTE_STREAM : (int)MLOGIT_IMPUTE_STREAM;
}
int lp_stride(int which) {
  return which == 0 ? STUDENT_IMPUTE_STRIDE : which == 1 ? STUDENT_SN_STRIDE
       : which == 2 ? QUANTILE_IMPUTE_STRIDE : MLOGIT_IMPUTE_STRIDE;
}
int lp_acc_count() { return ACC_COUNT; }
int lp_acc_sigsq() { return ACC_SIGSQ; }
int lp_acc_sigsq2() { return ACC_SIGSQ2; }
int lp_max_choices() { return MLOGIT_MAX_CHOICES; }

int lp_student_impute(LP_STUDENT_ARGS) { return run_student(S_IMPUTE, LP_STUDENT_PASS); }
int lp_student_impute_ss(LP_STUDENT_ARGS) { return run_student(S_IMPUTE_SS, LP_STUDENT_PASS); }
// student_ss_h_kernel: reads w
int lp_student_ss_h(LP_STUDENT_ARGS) { return run_student(S_SS_H, LP_STUDENT_PASS); }
// student_ss_suf_kernel: reads w
int lp_student_ss_suf(LP_STUDENT_ARGS) { return run_student(S_SS_SUF, LP_STUDENT_PASS); }
// student_sigma_nu_kernel: reads w
int lp_student_sigma_nu(LP_STUDENT_ARGS) { return run_student(S_SIGMA_NU, LP_STUDENT_PASS); }
int lp_student_sigma_nu_ss(LP_STUDENT_ARGS) { return run_student(S_SIGMA_NU_SS, LP_STUDENT_PASS); }

int lp_quantile_impute(LP_HEAD, const double *y, size_t ny, double shift, double *z, double *w, size_t nout,
                       size_t guard) {
  if (!head_ok(LP_HEAD_PASS, 1)) return LP_BAD_REQUEST;
  const size_t cn = (size_t)chains * (size_t)n;
  if (!y || !z || !w || ny < (size_t)n || nout < 2 * guard + cn) return LP_BAD_REQUEST;
  Dev<double> dX(X, nX), dB(beta, ngb), dY(y, ny), dZ(z, nout), dW(w, nout);
  Dev<uint8_t> dG(gamma, ngb);
  Dev<int32_t> dS(status, nstatus);
  IP_TRY(dX.err); IP_TRY(dB.err); IP_TRY(dY.err); IP_TRY(dZ.err); IP_TRY(dW.err); IP_TRY(dG.err); IP_TRY(dS.err);
  QuantileParams P{};
  fill_head(P, LP_HEAD_PASS, dX.ptr, dG.ptr, dB.ptr, dS.ptr);
  P.z = dZ.ptr + guard; P.w = dW.ptr + guard; P.y = dY.ptr; P.shift = shift;
  hipLaunchKernelGGL(quantile_impute_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)chains), dim3(256), 0, nullptr, P);
  IP_TRY(hipGetLastError());
  IP_TRY(hipDeviceSynchronize());
  IP_TRY(dZ.back()); IP_TRY(dW.back());
  return (int)dS.back();
}

// Xs: n x psub column-major, Xc: n M x pch column-major (null where there are no such columns);
// X, Xsq: nout doubles each, the N x D block starts guard elements in
int lp_mlogit_expand(int64_t n, int M, int psub, int pch, const double *Xs, size_t nXs, const double *Xc, size_t nXc,
                     double *X, double *Xsq, size_t nout, size_t guard) {
  if (n < 1 || n > (1 << 24) || M < 2 || M > MLOGIT_MAX_CHOICES || psub < 0 || pch < 0 || psub > 4096 || pch > 4096)
    return LP_BAD_REQUEST;
  const size_t N = (size_t)n * (size_t)M, D = (size_t)(M - 1) * (size_t)psub + (size_t)pch;
  if (D < 1 || N * D > ((size_t)1 << 31) || !X || !Xsq || nout < 2 * guard + N * D) return LP_BAD_REQUEST;
  if ((psub > 0 && (!Xs || nXs < (size_t)n * (size_t)psub)) || (pch > 0 && (!Xc || nXc < N * (size_t)pch)))
    return LP_BAD_REQUEST;
  Dev<double> dXs(psub > 0 ? Xs : nullptr, nXs), dXc(pch > 0 ? Xc : nullptr, nXc), dX(X, nout), dXsq(Xsq, nout);
  IP_TRY(dXs.err); IP_TRY(dXc.err); IP_TRY(dX.err); IP_TRY(dXsq.err);
  const int64_t total = (int64_t)(N * D);
  hipLaunchKernelGGL(mlogit_expand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, n, M, psub,
                     pch, dXs.ptr, dXc.ptr, dX.ptr + guard, dXsq.ptr + guard);
  IP_TRY(hipGetLastError());
  IP_TRY(hipDeviceSynchronize());
  IP_TRY(dX.back());
  return (int)dXsq.back();
}

int lp_mlogit_impute(LP_MLOGIT_ARGS) { return run_mlogit(true, LP_MLOGIT_PASS); }
// mlogit_wss_kernel: reads wss_part and the status words
int lp_mlogit_wss(LP_MLOGIT_ARGS) { return run_mlogit(false, LP_MLOGIT_PASS); }

}  // extern "C"
