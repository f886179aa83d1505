// Per-kernel-class device time of an engine's launches (ba_set_kernel_timing /
// ba_get_kernel_times): with timing enabled a launcher brackets its kernel with a
// pair of HIP events ON THE STREAM THE KERNEL IS LAUNCHED ON; disabled (the default)
// a KtScope is two loads of a thread-local pointer.  Measurement only -- no draw
// depends on it.  bench.py uses it for the roofline objects of the configurations
// whose sweep round is several kernels.
#ifndef BOOM_AMD_KTIMER_H
#define BOOM_AMD_KTIMER_H

#include <hip/hip_runtime.h>

namespace boom_amd {

enum KernelClass {
  KT_SSVS = 0,      // ssvs_sweep_kernel
  KT_SSVS_BIG,      // ssvs_big_kernel
  KT_SSVS_ADAPTIVE, // ssvs_adaptive_kernel
  KT_KALMAN,        // kalman_simsmooth_kernel
  KT_SSM,           // ssm_simsmooth_kernel
  KT_XTE_GEMM,      // xtwx_cols_kernel<false, XTE_KCHUNK> + plain_reduce_kernel (launch_xte_tiled: X'e of every chain)
  KT_PROBIT_IMPUTE, // probit_impute_kernel
  KT_LOGIT_IMPUTE,  // logit_impute_kernel
  KT_ROWS_GEMM,     // xtwx_cols_kernel<false> + plain_reduce_kernel (X'z, diagonal)
  KT_COLS_GEMM,     // xtwx_cols_kernel<true> + xtwx_cols_reduce_kernel (vectors of V)
  KT_SUF,           // xtx_mfma_kernel + plane_sum_kernel + col_reduce_kernel
  KT_POISSON_IMPUTE,// poisson_impute_kernel
  KT_KALMAN_PREPARE,// kalman_prepare_kernel (level variance + normals, second stream)
  KT_SS_ROUND,      // ss_round_kernel (the local-level bsts rounds of a call, one persistent launch)
  KT_STUDENT_IMPUTE,   // student_impute_kernel
  KT_STUDENT_SIGMA_NU, // student_sigma_nu_kernel
  KT_QUANTILE_IMPUTE,  // quantile_impute_kernel
  KT_MLOGIT_IMPUTE,    // mlogit_impute_kernel + mlogit_wss_kernel
  KT_SS_STUDENT,       // student_impute_kernel<true> / student_ss_h_kernel / student_ss_suf_kernel (bsts family = student)
  KT_SS_POISSON,       // poisson_impute_kernel<true> / latent_ss_h_kernel / latent_ss_suf_kernel (bsts family = poisson)
  KT_SS_LOGIT,         // logit_impute_kernel<true> / latent_ss_h_kernel / latent_ss_suf_kernel (bsts family = logit)
  KT_SS_STUDENT_TREND, // slt_params_kernel / slt_weights_kernel (the Student local linear trend state model)
  KT_SS_FILTER,        // ss_filter_kernel (ba_ss_prediction_errors: the forward-only filter of the chains' current draw)
  KT_SS_AUTOAR,        // ar_spike_kernel (the spike-and-slab autoregression state model's sampler)
  KT_SS_REGHOLIDAY,    // rh_draw_kernel / rh_observe_kernel (the regression holiday state model)
  KT_CLASSES
};

void kt_mark(hipStream_t stream, int cls, bool begin);   // engine.hip
bool kt_active();

struct KtScope {
  hipStream_t s;
  int c;
  bool on;
  KtScope(hipStream_t stream, int cls) : s(stream), c(cls), on(kt_active()) {
    if (on) kt_mark(s, c, true);
  }
  ~KtScope() {
    if (on) kt_mark(s, c, false);
  }
};

}  // namespace boom_amd
#endif
