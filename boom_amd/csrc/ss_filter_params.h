// Launch parameters of the one-step prediction error kernel (ss_filter_kernel.hip), shared
// with the host side (engine_ss_observe.hip: ba_ss_prediction_errors, ba_ss_holdout_prediction_errors).
#pragma once
#include <stdint.h>

#include "kalman_params.h"

namespace boom_amd {

// Where a chain's parameters are read: a base pointer per array and the distance, in
// elements, from one chain's values to the next chain's.  The live arrays have the strides
// p, p, 1, SSG_MAX_VAR, SSG_MAX_AR * AR_MAX (the local-level path: its level variance at
// stride 1); one row of the look-ahead's record has the base of chain 0's row and the strides
// L p, L p, L, L nvar, L nphi.  Within a chain the variances sit at their slot index and an
// autoregression slot's coefficients at slot * AR_MAX, in both.
struct SsFilterSource {
  const uint8_t *gamma;
  const double *beta, *sigsq, *var, *phi;   // (phi: nullptr when the list has no autoregression slot)
  int64_t gamma_stride, beta_stride, sigsq_stride, var_stride, phi_stride;
};

struct SsFilterParams {
  int32_t T, p, m, nblocks, nvar, nar;
  int32_t ld;                 // leading dimension of the state variance in LDS: odd, > m (column m carries the state mean)
  int32_t chain_first, chain_count, standardize;
  const SsgSpec *spec;        // device copy (the local-level path: a one-block list)
  const double *y, *X;        // T; T x p column-major
  const uint8_t *observed;    // T
  SsFilterSource src;
  // the Student local linear trend's weights (nullptr: no such block): the level's T, then the slope's T
  const double *qw;
  int64_t qw_stride;
  double *errors;             // chain_count x T (never null: it carries y* into the serial pass)
  double *variances;          // chain_count x T, or nullptr
  double *loglik;             // chain_count
  int32_t *flag;              // the smallest chain of the launch whose forecast variance was not positive (else untouched)
  // the packed calendar of the random-walk holidays and the calendar seasonals (SsParams::cal), at least
  // T entries; nullptr: no such block
  const uint64_t *cal;
  // the dynamic regressions' predictors (SsParams::dyn), at least T rows of dyn_cols; nullptr: no such block
  const double *dyn;
  int32_t dyn_cols, dyn_pad;
  // y is every chain's own series, y_stride doubles apart (SsParams::y_stride: a list with regression
  // holiday models); 0: the one series shared by the chains
  int64_t y_stride;
  // ---- the holdout instance only (launch_ss_filter_holdout: ba_ss_holdout_prediction_errors).  There T is the
  // number of holdout rows h -- y the caller's h responses (y_stride 0), X its h x p predictors, column-major
  // at leading dimension h, errors and variances chain_count x h; observed, loglik and qw are not read --
  // and the filter runs on the time indices time0 .. time0 + h - 1:
  int32_t time0, time0_pad;   // the series' length: the time of the first holdout row
  // component k of chain c's state draw at time time0 - 1 sits at state[c * state_stride + k]
  const double *state;
  int64_t state_stride;
};

hipError_t launch_ss_filter(hipStream_t stream, const SsFilterParams &P);
hipError_t launch_ss_filter_holdout(hipStream_t stream, const SsFilterParams &P);
size_t ss_filter_lds(int m, int ld);

}  // namespace boom_amd
