// Test-only probe of the hierarchical regression holiday's draw, for tests/test_hier_draw_probe_gpu.py.
//
// The product's hier_holiday_kernel.hip is included whole -- rhh_draw_kernel and, through it,
// mvn_wishart_device.h -- and compiled with the product's flags; nothing is restated.  The file's host
// launcher names the kernel timer's two functions; the probe never calls that launcher and resolves the two
// names by stubs, so nothing of the product library is linked.
//
// hp_draw launches rhh_draw_kernel for `chains` chains on one model in slot `slot` of the list whose
// coefficients start at flat index `base`: H holidays of width d.  The conventions are dist_probe.hip's:
// host arrays with explicit lengths (in doubles / words), checked ON THE HOST against what the kernel reads
// and writes for these arguments (HP_BAD_REQUEST instead of a launch where they do not fit), device buffers
// of exactly those lengths, everything copied in and the writable ones copied back whole.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "hier_holiday_kernel.hip"

namespace boom_amd {
// (never called: the probe launches the kernel itself)
void kt_mark(hipStream_t, int, bool) {}
bool kt_active() { return false; }
}  // namespace boom_amd

using namespace boom_amd;

namespace {

enum : int { HP_BAD_REQUEST = -1 };

template <class T>
struct Dev {
  T *ptr = nullptr;
  T *host;
  size_t bytes;
  hipError_t err = hipSuccess;
  Dev(const T *h, size_t count) : host(const_cast<T *>(h)), bytes(count * sizeof(T)) {
    if (!h || !count) return;
    err = hipMalloc((void **)&ptr, bytes);
    if (err == hipSuccess) err = hipMemcpy(ptr, h, bytes, hipMemcpyHostToDevice);
  }
  hipError_t back() { return ptr ? hipMemcpy(host, ptr, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
  ~Dev() {
    if (ptr) (void)hipFree(ptr);
  }
  Dev(const Dev &) = delete;
};

#define HP_TRY(expr)                              \
  do {                                            \
    hipError_t e__ = (expr);                      \
    if (e__ != hipSuccess) return (int)e__;       \
  } while (0)

}  // namespace

extern "C" {

int hp_max_coef() { return RH_MAX_COEF; }
int hp_max_models() { return RH_MAX_MODELS; }
int hp_max_width() { return RHH_MAX_WIDTH; }
int hp_hyper_stride() { return RHH_HYPER_STRIDE; }
int hp_stream() { return (int)RHH_STREAM; }
int hp_bad_draw() { return RHH_BAD_DRAW; }

// hyper: RH_MAX_MODELS x RHH_HYPER_STRIDE (the slot's block is read); sigsq: chains; counts: RH_MAX_COEF;
// totals, coef: chains x RH_MAX_COEF; mu: chains x RH_MAX_MODELS x 16; omega: chains x RH_MAX_MODELS x 256;
// pos: chains; status: chains.  coef, mu, omega, pos and status come back.
int hp_draw(int chains, int slot, int base, int d, int H, double nu0, uint32_t seed_lo, uint32_t seed_hi, int64_t chain_offset,
            const double *hyper, size_t nhyper, const double *sigsq, size_t nsigsq, const double *counts, size_t ncounts,
            const double *totals, size_t ntotals, double *coef, size_t ncoef, double *mu, size_t nmu, double *omega,
            size_t nomega, uint64_t *pos, size_t npos, int32_t *status, size_t nstatus) {
  if (!hyper || !sigsq || !counts || !totals || !coef || !mu || !omega || !pos || !status) return HP_BAD_REQUEST;
  if (chains < 1 || chains > 64 || slot < 0 || slot >= RH_MAX_MODELS) return HP_BAD_REQUEST;
  if (d < 1 || d > RHH_MAX_WIDTH || H < 1 || base < 0 || (int64_t)base + (int64_t)H * d > RH_MAX_COEF) return HP_BAD_REQUEST;
  if (!(nu0 > (double)(d - 1)) || !std::isfinite(nu0)) return HP_BAD_REQUEST;   // (a gamma shape that is positive)
  const size_t C = (size_t)chains, W = RHH_MAX_WIDTH;
  if (nhyper != (size_t)RH_MAX_MODELS * RHH_HYPER_STRIDE || nsigsq != C || ncounts != (size_t)RH_MAX_COEF ||
      ntotals != C * RH_MAX_COEF || ncoef != C * RH_MAX_COEF || nmu != C * RH_MAX_MODELS * W ||
      nomega != C * RH_MAX_MODELS * W * W || npos != C || nstatus != C)
    return HP_BAD_REQUEST;
  Dev<double> dH(hyper, nhyper), dS(sigsq, nsigsq), dN(counts, ncounts), dT(totals, ntotals), dC(coef, ncoef), dM(mu, nmu),
      dO(omega, nomega);
  Dev<uint64_t> dP(pos, npos);
  Dev<int32_t> dSt(status, nstatus);
  HP_TRY(dH.err); HP_TRY(dS.err); HP_TRY(dN.err); HP_TRY(dT.err); HP_TRY(dC.err); HP_TRY(dM.err); HP_TRY(dO.err);
  HP_TRY(dP.err); HP_TRY(dSt.err);
  SsParams P{};
  P.chains = chains;
  P.chain_first = 0;
  P.chain_count = chains;
  P.chain_offset = chain_offset;
  P.sigsq = dS.ptr;
  P.seed_lo = seed_lo;
  P.seed_hi = seed_hi;
  P.status = dSt.ptr;
  P.only_ran = nullptr;
  RhParams R{};
  R.nmodels = slot + 1;
  R.ncoef = base + H * d;
  R.counts = dN.ptr;
  R.coef = dC.ptr;
  R.totals = dT.ptr;
  for (int k = 0; k <= RH_MAX_MODELS; ++k) R.first[k] = k <= slot ? (k == slot ? base : 0) : base + H * d;
  RhhParams Q{};
  Q.nmodels = slot + 1;
  Q.mask = 1 << slot;
  Q.width[slot] = d;
  Q.nhol[slot] = H;
  Q.nu0[slot] = nu0;
  Q.hyper = dH.ptr;
  Q.mu = dM.ptr;
  Q.omega = dO.ptr;
  Q.pos = dP.ptr;
  hipLaunchKernelGGL(rhh_draw_kernel, dim3((unsigned)chains), dim3(WAVE), 0, nullptr, P, R, Q);
  HP_TRY(hipGetLastError());
  HP_TRY(hipDeviceSynchronize());
  HP_TRY(dC.back()); HP_TRY(dM.back()); HP_TRY(dO.back()); HP_TRY(dP.back());
  return (int)dSt.back();
}

}  // extern "C"
