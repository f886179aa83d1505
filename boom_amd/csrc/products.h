// The product launchers (xtwx_cols_kernel.hip, predict_kernel.hip): their one declaration, for
// the host files (engine_internal.h), the files that define them, the imputation kernel files
// that call them, and the host-only probe of tests/cpp.  No device code.
#pragma once
#include <hip/hip_runtime_api.h>

#include <stddef.h>
#include <stdint.h>

namespace boom_amd {

// ---- xtwx_cols_kernel.hip
// planes of the split-K workspace for rows of n: of the column and rows products, of the X'e product
int xtwx_cols_planes(int64_t n);
int xte_planes(int64_t n);
// the vectors of V named by req[0, R): V_c[., g] = base[., g] + X'(w_c o x_g); planes = workspace
// of xtwx_cols_planes(n) R p doubles
hipError_t launch_xtwx_cols(hipStream_t stream, const double *X, int64_t n, int p, const double *w,
                            const int32_t *req, int R, const double *base, double *V,
                            uint32_t *valid, int words, double *planes);
// the request list of a sweep's start: the included variables of every chain
hipError_t launch_xtwx_cols_start(hipStream_t stream, const uint8_t *gamma, int chains, int p,
                                  int32_t *req, int32_t *count, uint32_t *valid, int words);
// out (R x p, row-major) = U B with U: R rows of n, B: p K-contiguous columns of n
// (+ diag_base[j, j] on every row when given)
hipError_t launch_rows_times_columns(hipStream_t stream, const double *U, int R, const double *B, int64_t n,
                                     int p, const double *diag_base, double *out, double *planes);
// the same for short rows ldu doubles apart, planes of xte_planes(n); out may be null (planes only)
hipError_t launch_xte_tiled(hipStream_t stream, const double *U, int64_t ldu, int R, const double *B, int64_t n,
                            int p, double *out, double *planes);
hipError_t launch_square(hipStream_t stream, const double *x, size_t count, double *out);
// The tail of every imputation launch of the column service's families: X'Wz (xtz = z X, z
// already weighted) and then the diagonal of V = slab precision + X'WX (v_diag = w Xsq +
// diag(slab_precision)), both for `rows` chains of n observations.
hipError_t launch_latent_products(hipStream_t stream, const double *z, const double *w, int rows,
                                  const double *X, const double *Xsq, int64_t n, int p,
                                  const double *slab_precision, double *xtz, double *v_diag, double *planes);

// ---- predict_kernel.hip
hipError_t launch_predict(hipStream_t stream, const double *trace_k, const uint16_t *rec_idx,
                          const double *rec_beta, int stride, int cap, int first_draw, int ndraws,
                          int chains, int p, const double *newX, int nnew, double *out);

}  // namespace boom_amd
