// Host-only probe of the product library's kernel launchers, for tests/test_split_k_products_gpu.py.
//
// The launchers of xtwx_cols_kernel.hip and predict_kernel.hip are ordinary exported functions
// of libboomamd.so, declared in boom_amd/csrc/products.h.  Every wrapper takes host arrays with
// explicit lengths (in elements), allocates device buffers of exactly those lengths, copies
// everything in -- outputs and workspaces too, which the caller has filled with a sentinel and
// extended by a guard band --, launches on the null
// stream, synchronises, copies every writable buffer back whole and returns the hipError_t.
// No device code of its own.
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "../../boom_amd/csrc/products.h"

namespace {

// a device copy of a host array of exactly `count` elements (null host pointer: no buffer)
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

#define KP_TRY(expr)                              \
  do {                                            \
    hipError_t e__ = (expr);                      \
    if (e__ != hipSuccess) return (int)e__;       \
  } while (0)

}  // namespace

extern "C" {

int kp_planes(int64_t n) { return boom_amd::xtwx_cols_planes(n); }
int kp_xte_planes(int64_t n) { return boom_amd::xte_planes(n); }

// out[r, j] = sum_i U[r, i] B[j, i] (+ diag_base[j, j])
int kp_rows_times_columns(const double *U, size_t nU, int R, const double *B, size_t nB, int64_t n, int p,
                          const double *diag_base, size_t ndiag, double *out, size_t nout, double *planes,
                          size_t nplanes) {
  Dev<double> dU(U, nU), dB(B, nB), dD(diag_base, ndiag), dO(out, nout), dP(planes, nplanes);
  KP_TRY(dU.err); KP_TRY(dB.err); KP_TRY(dD.err); KP_TRY(dO.err); KP_TRY(dP.err);
  KP_TRY(boom_amd::launch_rows_times_columns(nullptr, dU.ptr, R, dB.ptr, n, p, dD.ptr, dO.ptr, dP.ptr));
  KP_TRY(hipDeviceSynchronize());
  KP_TRY(dO.back());
  return (int)dP.back();
}

// the same with rows of U ldu apart and planes of 128 rows; out may be null (planes only)
int kp_xte_tiled(const double *U, size_t nU, int64_t ldu, int R, const double *B, size_t nB, int64_t n, int p,
                 double *out, size_t nout, double *planes, size_t nplanes) {
  Dev<double> dU(U, nU), dB(B, nB), dO(out, nout), dP(planes, nplanes);
  KP_TRY(dU.err); KP_TRY(dB.err); KP_TRY(dO.err); KP_TRY(dP.err);
  KP_TRY(boom_amd::launch_xte_tiled(nullptr, dU.ptr, ldu, R, dB.ptr, n, p, dO.ptr, dP.ptr));
  KP_TRY(hipDeviceSynchronize());
  KP_TRY(dO.back());
  return (int)dP.back();
}

// V_c[., g] = base[., g] + X'(w_c o x_g) for the R requests (c, g) of req
int kp_xtwx_cols(const double *X, size_t nX, int64_t n, int p, const double *w, size_t nw, const int32_t *req,
                 int R, const double *base, size_t nbase, double *V, size_t nV, uint32_t *valid, size_t nvalid,
                 int words, double *planes, size_t nplanes) {
  Dev<double> dX(X, nX), dW(w, nw), dBase(base, nbase), dV(V, nV), dP(planes, nplanes);
  Dev<int32_t> dReq(req, 2 * (size_t)R);
  Dev<uint32_t> dValid(valid, nvalid);
  KP_TRY(dX.err); KP_TRY(dW.err); KP_TRY(dBase.err); KP_TRY(dV.err); KP_TRY(dP.err); KP_TRY(dReq.err);
  KP_TRY(dValid.err);
  KP_TRY(boom_amd::launch_xtwx_cols(nullptr, dX.ptr, n, p, dW.ptr, dReq.ptr, R, dBase.ptr, dV.ptr, dValid.ptr,
                                    words, dP.ptr));
  KP_TRY(hipDeviceSynchronize());
  KP_TRY(dV.back());
  KP_TRY(dValid.back());
  return (int)dP.back();
}

// the request list of a sweep's start; req holds nreq int32 (two per request + guard)
int kp_xtwx_cols_start(const uint8_t *gamma, size_t ngamma, int chains, int p, int32_t *req, size_t nreq,
                       int32_t *count, uint32_t *valid, size_t nvalid, int words) {
  Dev<uint8_t> dG(gamma, ngamma);
  Dev<int32_t> dReq(req, nreq), dCnt(count, 1);
  Dev<uint32_t> dValid(valid, nvalid);
  KP_TRY(dG.err); KP_TRY(dReq.err); KP_TRY(dCnt.err); KP_TRY(dValid.err);
  KP_TRY(boom_amd::launch_xtwx_cols_start(nullptr, dG.ptr, chains, p, dReq.ptr, dCnt.ptr, dValid.ptr, words));
  KP_TRY(hipDeviceSynchronize());
  KP_TRY(dReq.back());
  KP_TRY(dCnt.back());
  return (int)dValid.back();
}

int kp_square(const double *x, size_t count, double *out, size_t nout) {
  Dev<double> dX(x, count), dO(out, nout);
  KP_TRY(dX.err); KP_TRY(dO.err);
  KP_TRY(boom_amd::launch_square(nullptr, dX.ptr, count, dO.ptr));
  KP_TRY(hipDeviceSynchronize());
  return (int)dO.back();
}

// predictions from a record given as it lies on the device: trace_k (chains x stride), rec_idx and
// rec_beta (chains x stride x cap), newX column-major nnew x p
int kp_predict(const double *trace_k, size_t nk, const uint16_t *rec_idx, size_t nidx, const double *rec_beta,
               size_t nbeta, int stride, int cap, int first_draw, int ndraws, int chains, int p,
               const double *newX, size_t nX, int nnew, double *out, size_t nout) {
  Dev<double> dK(trace_k, nk), dB(rec_beta, nbeta), dX(newX, nX), dO(out, nout);
  Dev<uint16_t> dI(rec_idx, nidx);
  KP_TRY(dK.err); KP_TRY(dB.err); KP_TRY(dX.err); KP_TRY(dO.err); KP_TRY(dI.err);
  KP_TRY(boom_amd::launch_predict(nullptr, dK.ptr, dI.ptr, dB.ptr, stride, cap, first_draw, ndraws, chains, p,
                                  dX.ptr, nnew, dO.ptr));
  KP_TRY(hipDeviceSynchronize());
  return (int)dO.back();
}

}  // extern "C"
