// The state space families with latent data: bsts family = "student", "poisson" and "logit".
#include "engine_internal.h"

// ---- what the sweeps of the three families share
namespace boom_amd {

// the trace of a call (ba_enable_trace): the call within its length, every chain's write position back at 0
static int family_trace_begin(ba_engine *e, int32_t nsweeps) {
  if (e->trace_stride <= 0) return BA_OK;
  if (nsweeps > e->trace_stride) return fail(BA_E_INVALID, "nsweeps exceeds the enabled trace length");
  HIP_TRY(hipMemsetAsync(e->dtrace_idx.ptr, 0, (size_t)e->cfg.chains * 4, e->stream));
  return BA_OK;
}

// Step 1 of a round: the observation model's sampler with fix_latent_data(true) -- the columns of
// V the chains' models start from, the sweep, and park-and-replay for vectors asked for mid-sweep
static int family_observation_draw(ba_engine *e, const SsvsParams &P) {
  HIP_TRY(launch_xtwx_cols_start(e->stream, e->dgamma.ptr, e->cfg.chains, e->p, e->cols.req.ptr, e->cols.count.ptr,
                                 e->cols.valid.ptr, e->cols.words));
  int32_t R = 0;
  HIP_TRY(hipMemcpyAsync(&R, e->cols.count.ptr, 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int rc = build_columns(e, R);
  if (rc) return rc;
  HIP_TRY(launch_sweeps(e, P, 1));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return check_chain_status(e);
}

// a call's end: the regression sweeps' tables and factors are not these chains' any more
static int family_sweep_end(ba_engine *e) {
  e->table_ok = false;
  e->model_ok = false;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return check_chain_status(e);
}

}  // namespace boom_amd

// ---- bsts family = "student": StateSpaceStudentRegressionModel + StateSpaceStudentPosteriorSampler
// (Models/StateSpace/StateSpaceStudentRegressionModel.cpp, PosteriorSamplers/
// StateSpaceStudentPosteriorSampler.cpp:56-126, StateSpacePosteriorSampler.cpp:41-63).  The
// observation model is the Student path's (student_kernel.hip: weights, sigma^2, nu; the
// SpikeSlabSampler sweep on every chain's own V = slab precision + X'WX through the column
// service), the state draw the general structural kernel with H_t = sigma^2 / w_t.

namespace boom_amd {

// the buffers of the kind beyond ss_prepare's and the Student path's: H_t; new weights are 1
// (the first impute_state of StateSpacePosteriorSampler::draw runs before any weight is drawn)
static int sst_buffers(ba_engine *e) {
  int rc = student_prepare(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, T = (size_t)e->T;
  const bool fresh = e->lat.w.count != C * T || e->dsst_h.count != C * T;
  rc = column_buffers(e);
  if (rc) return rc;
  if (e->dstu_u.count != C * T) HIP_TRY(e->dstu_u.resize(C * T));
  if (fresh) {
    HIP_TRY(e->dsst_h.resize(C * T));
    std::vector<double> one(C * T, 1.0);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->lat.w.ptr, one.data(), C * T * 8, hipMemcpyHostToDevice));
    e->sst_ready = false;
  }
  return BA_OK;
}

static int sst_prepare(ba_engine *e) {
  int rc = sweep_refusal(e, DATA_SS_STUDENT);
  if (rc) return rc;
  if (!e->ssm_set)
    return fail(BA_E_STATE, e->ss_level_set
                                ? "the Student-t state-space family takes a list of state models: call ba_ss_add_state_model "
                                  "(a local level is the one-block list), not ba_ss_set_local_level"
                                : "call ba_ss_add_state_model first");
  if (!e->have_slab) return fail(BA_E_STATE, "call ba_sss_set_slab first");
  if (!e->sss_slab_scales)
    return fail(BA_E_INVALID, "the Student-t state-space sampler takes a slab whose precision scales with sigma^2 (scales_with_sigsq = 1)");
  rc = switch_mode(e, 1, 1.0);
  if (rc) return rc;
  rc = ss_prepare(e, DATA_SS_STUDENT);
  if (rc) return rc;
  if (!e->ss_initialized) e->sst_ready = false;
  return sst_buffers(e);
}

static void fill_sst_params(ba_engine *e, SsParams &S, StudentParams &U) {
  fill_ss_params(e, S);
  S.ssm.tpl_trend = S.ssm.tpl_nseasons = S.ssm.tpl_ar_lags = 0;   // always the general kernel
  S.h = e->dsst_h.ptr;
  S.h_stride = e->T;
  fill_student_params(e, U);
  U.offset = S.scratch + S.T;   // (array 1 of a chain's scratch block: the kernel's last pass leaves Z_t'alpha_t there)
  U.offset_stride = S.scratch_stride;
  U.observed = e->dss_obs.ptr;
  U.h = e->dsst_h.ptr;
}

// Base::impute_state with the weights in hand: H_t, the state draw (the state models' parameters
// as they stand when draw == 0), then the offsets' consequences -- z, X'Wz, the diagonal of V
static int sst_impute_state(ba_engine *e, const SsParams &S, const StudentParams &U, int draw) {
  HIP_TRY(launch_student_ss_weights(e->stream, U, 0));
  HIP_TRY(launch_ssm_simsmooth(e->stream, S, draw));
  HIP_TRY(launch_student_ss_suf(e->stream, U, e->lat.Xsq.ptr, e->dA.ptr, e->dxty_c.ptr, e->cols.vdiag.ptr,
                                e->cols.planes.ptr));
  e->ss_initialized = true;
  e->sst_ready = true;
  return BA_OK;
}

}  // namespace boom_amd

extern "C" {

int ba_ss_student_set_data(ba_engine *e, int32_t T, int32_t p, const double *y, const double *X,
                           const uint8_t *observed) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!y || !X) return fail(BA_E_INVALID, "null argument");
  if (T <= 0 || p <= 0) return fail(BA_E_INVALID, "T and p must be positive");
  for (int32_t t = 0; t < T; ++t)
    if ((!observed || observed[t]) && !std::isfinite(y[t])) return fail(BA_E_INVALID, "observed responses must be finite");
  int rc = ba_ss_set_data(e, T, p, y, X, observed);
  if (rc) return rc;
  // the Student path's view of the same data (n = T): X, y, X squared
  std::vector<double> yo((size_t)T);
  for (int32_t t = 0; t < T; ++t) yo[(size_t)t] = (!observed || observed[t]) ? y[t] : 0.0;
  rc = upload_latent_data(e, T, p, X, yo.data(), nullptr, /*squared=*/true, 0);
  if (rc) return rc;
  // a new TRegressionModel and a sampler whose latent data are not initialised
  e->dstu_u.release();
  e->dstu_nu.release();
  e->dstu_dx.release();
  e->dstu_margin.release();
  e->lat.w.release();
  e->dsst_h.release();
  e->sst_round = 0;
  e->sst_ready = false;
  e->data_kind = DATA_SS_STUDENT;
  return BA_OK;
}

int ba_ss_student_get_weights(ba_engine *e, int64_t chain, double *w) {
  ENGINE_PROLOGUE(e);
  if (!w) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != DATA_SS_STUDENT) return fail(BA_E_STATE, set_data_first(DATA_SS_STUDENT));
  return read_chain_row(e, chain, e->lat.w, (size_t)e->T, w, [&] { return sst_buffers(e); });
}

int ba_ss_student_set_weights(ba_engine *e, int64_t chain, const double *w) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!w) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != DATA_SS_STUDENT) return fail(BA_E_STATE, set_data_first(DATA_SS_STUDENT));
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  const size_t T = (size_t)e->T;
  for (size_t t = 0; t < T; ++t)
    if (!(w[t] >= 0.0) || !std::isfinite(w[t])) return fail(BA_E_INVALID, "Weights must be finite and non-negative.");
  int rc = sst_buffers(e);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  rc = write_chain_rows(e, e->lat.w.ptr, chain, T, w);
  if (rc) return rc;
  e->sst_ready = false;   // (the statistics in hand are not these weights': the next call draws the state first)
  return BA_OK;
}

int ba_ss_student_impute_state(ba_engine *e) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  int rc = sst_prepare(e);
  if (rc) return rc;
  SsParams S;
  StudentParams U;
  fill_sst_params(e, S, U);
  rc = sst_impute_state(e, S, U, 0);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return check_chain_status(e);
}

// nsweeps x StateSpacePosteriorSampler::draw (StateSpacePosteriorSampler.cpp:41-63) with the
// Student observation model, every chain
int ba_ss_student_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (nsweeps < 0) return fail(BA_E_INVALID, "nsweeps must be non-negative");
  int rc = sst_prepare(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains;
  rc = family_trace_begin(e, nsweeps);
  if (rc) return rc;
  if (e->trace_stride > 0 && e->dstu_nu_rec.count != C * e->trace_stride) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(e->dstu_nu_rec.resize(C * e->trace_stride));
  }
  SsvsParams P;
  fill_params(e, P);
  SsParams S;
  StudentParams U;
  fill_sst_params(e, S, U);
  if (nsweeps == 0) return BA_OK;
  if (!e->sst_ready) {
    // the sampler's first draw(): impute_state with the weights as they stand (1 unless the
    // caller set them), then -- latent data not initialised yet -- impute_nonstate_latent_data.
    // Those weights are replaced by the round's own before any statistic reads them (the
    // statistics are taken at impute_state): they go to the z buffer, which the X'Wz GEMM has
    // finished with, and w stays what the statistics in hand were built from.
    const bool first = !e->ss_initialized;
    rc = sst_impute_state(e, S, U, 0);
    if (rc) return rc;
    if (first) {
      StudentParams W = U;
      W.w = e->lat.z.ptr;
      W.sweep = e->lat.draws++;
      HIP_TRY(launch_student_ss_weights(e->stream, W, 1));
    }
  }
  for (int i = 0; i < nsweeps; ++i) {
    // 1. the observation model's sampler with fix_latent_data(true)
    // (TRegressionSpikeSlabSampler::draw, TRegressionSpikeSlabSampler.cpp:41-47): indicators and
    // beta on the statistics of the last impute_state ...
    rc = family_observation_draw(e, P);
    if (rc) return rc;
    // 2. ... sigma^2, nu
    U.sweep = e->sst_round++;
    HIP_TRY(launch_student_sigma_nu(e->stream, U));
    // 3. - 5. impute_nonstate_latent_data, then the state models' samplers and impute_state (one
    // kernel: the samplers read their own streams and the statistics of the last state draw, so
    // their place before or after the weights does not show)
    U.sweep = e->lat.draws++;
    HIP_TRY(launch_student_ss_weights(e->stream, U, 1));
    HIP_TRY(launch_ssm_simsmooth(e->stream, S, 1));
    // 6. the complete-data statistics of the next round's observation draw
    HIP_TRY(launch_student_ss_suf(e->stream, U, e->lat.Xsq.ptr, e->dA.ptr, e->dxty_c.ptr, e->cols.vdiag.ptr,
                                  e->cols.planes.ptr));
    fill_params(e, P);
  }
  return family_sweep_end(e);
}

}  // extern "C"

// ---- bsts family = "poisson" and family = "logit": StateSpacePoissonModel + StateSpacePoissonPosteriorSampler
// (Models/StateSpace/StateSpacePoissonModel.cpp, PosteriorSamplers/StateSpacePoissonPosteriorSampler.cpp:
// 79-147), StateSpaceLogitModel + StateSpaceLogitPosteriorSampler (StateSpaceLogitModel.cpp,
// StateSpaceLogitPosteriorSampler.cpp:49-123), both under StateSpacePosteriorSampler.cpp:42-64.  The
// observation model is the family's regression path's (probit_kernel.hip: the auxiliary-mixture
// imputation; the SpikeSlabSampler sweep at sigma^2 = 1 on every chain's own V = slab precision +
// X'QX through the column service), the state draw the general structural kernel on every chain's
// own series v_t with H_t = 1 / q_t.  One set of helpers serves both kinds; what differs is here:

namespace boom_amd {

// the kind's family number for the launchers (probit_kernel.hip), its name in a refusal, and the
// precision a new model gives an observed step: 1 (AugmentedPoissonRegressionData::add_data), or
// 4 / n_t (AugmentedBinomialRegressionData::add_data, StateSpaceLogitModel.cpp:67-74)
static int ssp_family(const ba_engine *e) { return e->data_kind == DATA_SS_LOGIT ? 1 : 0; }
static double ssp_initial_precision(const ba_engine *e, size_t t) {
  return e->data_kind == DATA_SS_LOGIT ? 4.0 / e->ssp_trials[t] : 1.0;
}

// the buffers of the kind beyond ss_prepare's and the column service's: v_t and H_t; new latent
// data are v = 0, q = the family's initial precision (0 where the step is missing)
static int ssp_buffers(ba_engine *e) {
  int rc = alloc_chain_state(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, T = (size_t)e->T;
  const bool fresh = e->lat.w.count != C * T || e->dssp_value.count != C * T || e->dssp_h.count != C * T;
  rc = column_buffers(e);
  if (rc) return rc;
  if (fresh) {
    HIP_TRY(e->dssp_value.resize(C * T));
    HIP_TRY(e->dssp_h.resize(C * T));
    std::vector<double> q(C * T);
    for (size_t c = 0; c < C; ++c)
      for (size_t t = 0; t < T; ++t) q[c * T + t] = e->ssp_observed[t] ? ssp_initial_precision(e, t) : 0.0;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->lat.w.ptr, q.data(), C * T * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(e->dssp_value.ptr, 0, C * T * 8));
    e->ssp_ready = false;
  }
  return BA_OK;
}

static int ssp_prepare(ba_engine *e, DataKind kind) {
  int rc = sweep_refusal(e, kind);
  if (rc) return rc;
  const bool logit = kind == DATA_SS_LOGIT;
  if (!logit && !e->poisson_mix_set) return fail(BA_E_STATE, "call ba_poisson_set_mixtures first");
  if (!e->ssm_set) {
    if (!e->ss_level_set) return fail(BA_E_STATE, "call ba_ss_add_state_model first");
    return fail(BA_E_STATE, logit ? "the logit state-space family takes a list of state models: call ba_ss_add_state_model "
                                    "(a local level is the one-block list), not ba_ss_set_local_level"
                                  : "the Poisson state-space family takes a list of state models: call ba_ss_add_state_model "
                                    "(a local level is the one-block list), not ba_ss_set_local_level");
  }
  if (!e->have_slab) return fail(BA_E_STATE, "call ba_sss_set_slab first");
  if (e->sss_slab_scales)
    return fail(BA_E_INVALID, logit ? "the logit state-space sampler takes a fixed-precision slab (scales_with_sigsq = 0)"
                                    : "the Poisson state-space sampler takes a fixed-precision slab (scales_with_sigsq = 0)");
  rc = switch_mode(e, 1, 1.0);
  if (rc) return rc;
  rc = ss_prepare(e, kind);
  if (rc) return rc;
  rc = set_unit_sigsq(e);   // (the latent data have unit variance, as in logit_family_sweep)
  if (rc) return rc;
  if (!e->ss_initialized) e->ssp_ready = false;
  return ssp_buffers(e);
}

static void fill_ssp_params(ba_engine *e, SsParams &S, ProbitParams &Q) {
  fill_ss_params(e, S);
  S.ssm.tpl_trend = S.ssm.tpl_nseasons = S.ssm.tpl_ar_lags = 0;   // always the general kernel
  S.h = e->dssp_h.ptr;
  S.h_stride = e->T;
  S.y = e->dssp_value.ptr;   // (v itself: the kernel subtracts x'beta)
  S.y_stride = e->T;
  fill_probit_params(e, Q);
  Q.offset = S.scratch + S.T;   // (array 1 of a chain's scratch block: the kernel's last pass leaves Z_t'alpha_t there)
  Q.offset_stride = S.scratch_stride;
  Q.observed = e->dss_obs.ptr;
  Q.value = e->dssp_value.ptr;
  Q.h = e->dssp_h.ptr;
}

// Base::impute_state with the latent data in hand: H_t, the state draw (the state models'
// parameters as they stand when draw == 0), then the offsets' consequences -- z, X'Qz, the diagonal of V
static int ssp_impute_state(ba_engine *e, const SsParams &S, const ProbitParams &Q, int draw) {
  const int family = ssp_family(e);
  HIP_TRY(launch_latent_ss_h(e->stream, Q, family, 0));
  HIP_TRY(launch_ssm_simsmooth(e->stream, S, draw));
  HIP_TRY(launch_latent_ss_suf(e->stream, Q, family, e->lat.Xsq.ptr, e->dA.ptr, e->cols.vdiag.ptr, e->cols.planes.ptr));
  e->ss_initialized = true;
  e->ssp_ready = true;
  return BA_OK;
}

// ba_ss_poisson_get_latent / ba_ss_logit_get_latent
static int ssp_get_latent(ba_engine *e, DataKind kind, int64_t chain, double *value, double *precision) {
  if (!value || !precision) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != kind) return fail(BA_E_STATE, set_data_first(kind));
  int rc = read_chain_row(e, chain, e->dssp_value, (size_t)e->T, value, [&] { return ssp_buffers(e); });
  if (rc) return rc;
  return read_chain_row(e, chain, e->lat.w, (size_t)e->T, precision, [&] { return BA_OK; });
}

// ba_ss_poisson_set_latent / ba_ss_logit_set_latent
static int ssp_set_latent(ba_engine *e, DataKind kind, int64_t chain, const double *value, const double *precision) {
  if (!value || !precision) return fail(BA_E_INVALID, "null argument");
  if (e->data_kind != kind) return fail(BA_E_STATE, set_data_first(kind));
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  const size_t T = (size_t)e->T;
  std::vector<double> v(T, 0.0), q(T, 0.0);   // (a missing step's entries are not read)
  for (size_t t = 0; t < T; ++t) {
    if (!e->ssp_observed[t]) continue;
    if (precision[t] < 0) return fail(BA_E_INVALID, "precision must be non-negative.");
    // (the reference takes these and then filters with a variance of -infinity)
    if (!(precision[t] > 0) || !std::isfinite(precision[t]))
      return fail(BA_E_INVALID, "the precision of an observed step must be positive and finite");
    if (!std::isfinite(value[t])) return fail(BA_E_INVALID, "the latent value of an observed step must be finite");
    v[t] = value[t];
    q[t] = precision[t];
  }
  int rc = ssp_buffers(e);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  rc = write_chain_rows(e, e->dssp_value.ptr, chain, T, v.data());
  if (!rc) rc = write_chain_rows(e, e->lat.w.ptr, chain, T, q.data());
  if (rc) return rc;
  e->ssp_ready = false;   // (the statistics in hand are not these data's: the next call draws the state first)
  return BA_OK;
}

// ba_ss_poisson_impute_state / ba_ss_logit_impute_state
static int ssp_impute_state_entry(ba_engine *e, DataKind kind) {
  int rc = ssp_prepare(e, kind);
  if (rc) return rc;
  SsParams S;
  ProbitParams Q;
  fill_ssp_params(e, S, Q);
  rc = ssp_impute_state(e, S, Q, 0);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return check_chain_status(e);
}

// ba_ss_poisson_sweep / ba_ss_logit_sweep: nsweeps x StateSpacePosteriorSampler::draw
// (StateSpacePosteriorSampler.cpp:42-64) with the kind's observation model, every chain
static int ssp_sweep(ba_engine *e, DataKind kind, int32_t nsweeps) {
  if (nsweeps < 0) return fail(BA_E_INVALID, "nsweeps must be non-negative");
  int rc = ssp_prepare(e, kind);
  if (rc) return rc;
  const int family = ssp_family(e);
  rc = family_trace_begin(e, nsweeps);
  if (rc) return rc;
  SsvsParams P;
  fill_params(e, P);
  SsParams S;
  ProbitParams Q;
  fill_ssp_params(e, S, Q);
  if (nsweeps == 0) return BA_OK;
  if (!e->ssp_ready) {
    // the sampler's first draw(): impute_state with the latent data as they stand (v = 0, q = the
    // family's initial precision unless the caller set them), then -- latent data not initialised
    // yet -- impute_nonstate_latent_data.  Every value that imputation writes is overwritten by the
    // round's own (step 3 below) before anything reads it -- the statistics are taken at
    // impute_state -- so it is not launched; only its slots of the imputation stream (11 Poisson,
    // 9 logit) are used up: the counter moves on, and round r of a fresh sampler imputes with
    // s = r + 1.
    const bool first = !e->ss_initialized;
    rc = ssp_impute_state(e, S, Q, 0);
    if (rc) return rc;
    if (first) ++e->lat.draws;
  }
  for (int i = 0; i < nsweeps; ++i) {
    // 1. the observation model's sampler with fix_latent_data(true)
    // (PoissonRegressionSpikeSlabSampler::draw, PoissonRegressionSpikeSlabSampler.cpp:55-59;
    // BinomialLogitSpikeSlabSampler::draw): indicators and beta at sigma^2 = 1 on the statistics
    // of the last impute_state
    rc = family_observation_draw(e, P);
    if (rc) return rc;
    // 2. - 4. impute_nonstate_latent_data at the new beta and the last state draw, then the state
    // models' samplers and impute_state (one kernel: the samplers read their own streams and the
    // statistics of the last state draw, so their place before or after the imputation does not show)
    Q.sweep = e->lat.draws++;
    HIP_TRY(launch_latent_ss_h(e->stream, Q, family, 1));
    HIP_TRY(launch_ssm_simsmooth(e->stream, S, 1));
    // 5. the complete-data statistics of the next round's observation draw
    HIP_TRY(launch_latent_ss_suf(e->stream, Q, family, e->lat.Xsq.ptr, e->dA.ptr, e->cols.vdiag.ptr, e->cols.planes.ptr));
    fill_params(e, P);
  }
  return family_sweep_end(e);
}

}  // namespace boom_amd

extern "C" {

int ba_ss_poisson_set_data(ba_engine *e, int32_t T, int32_t p, const double *counts, const double *exposure,
                           const double *X, const uint8_t *observed) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!counts || !exposure || !X) return fail(BA_E_INVALID, "null argument");
  if (T <= 0 || p <= 0) return fail(BA_E_INVALID, "T and p must be positive");
  // (a missing step's count and exposure are never read: 0 and 1 stand in for them on the device)
  std::vector<double> yo((size_t)T, 0.0), ex((size_t)T, 1.0);
  std::vector<uint8_t> obs((size_t)T, 1);
  for (int32_t t = 0; t < T; ++t) {
    if (observed && !observed[t]) { obs[(size_t)t] = 0; continue; }
    if (!(counts[t] >= 0) || counts[t] != std::floor(counts[t])) return fail(BA_E_INVALID, "counts must be non-negative integers");
    if (!(exposure[t] > 0)) return fail(BA_E_INVALID, "exposures must be positive");
    yo[(size_t)t] = counts[t];
    ex[(size_t)t] = exposure[t];
  }
  int rc = ba_ss_set_data(e, T, p, yo.data(), X, observed);
  if (rc) return rc;
  // the Poisson path's view of the same data (n = T): X, counts, exposures, X squared
  rc = upload_latent_data(e, T, p, X, yo.data(), ex.data(), /*squared=*/true, 0);
  if (rc) return rc;
  e->poisson_y.resize((size_t)T);
  for (int32_t t = 0; t < T; ++t) e->poisson_y[(size_t)t] = (int64_t)std::llround(yo[(size_t)t]);   // (missing: 0, "unused")
  e->poisson_mix_set = false;
  // a new model (v = 0, q = 1) and a sampler whose latent data are not initialised
  e->ssp_observed = obs;
  e->lat.w.release();
  e->dssp_value.release();
  e->dssp_h.release();
  e->ssp_ready = false;
  e->data_kind = DATA_SS_POISSON;
  return BA_OK;
}

int ba_ss_poisson_get_latent(ba_engine *e, int64_t chain, double *value, double *precision) {
  ENGINE_PROLOGUE(e);
  return ssp_get_latent(e, DATA_SS_POISSON, chain, value, precision);
}

int ba_ss_poisson_set_latent(ba_engine *e, int64_t chain, const double *value, const double *precision) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  return ssp_set_latent(e, DATA_SS_POISSON, chain, value, precision);
}

int ba_ss_poisson_impute_state(ba_engine *e) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  return ssp_impute_state_entry(e, DATA_SS_POISSON);
}

int ba_ss_poisson_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  return ssp_sweep(e, DATA_SS_POISSON, nsweeps);
}

// ---- bsts family = "logit"
int ba_ss_logit_set_data(ba_engine *e, int32_t T, int32_t p, const double *successes, const double *trials,
                         const double *X, const uint8_t *observed, int32_t clt_threshold) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!successes || !trials || !X) return fail(BA_E_INVALID, "null argument");
  if (T <= 0 || p <= 0) return fail(BA_E_INVALID, "T and p must be positive");
  // (as in ba_logit_set_data: two uniforms per trial of the step's substream of LOGIT_STRIDE)
  if (clt_threshold < 1 || 4 * clt_threshold > LOGIT_STRIDE)
    return fail(BA_E_INVALID, "clt_threshold must be between 1 and 64");
  // (a missing step's successes and trials are never read: 0 and 1 stand in for them on the device)
  std::vector<double> yo((size_t)T, 0.0), nt((size_t)T, 1.0);
  std::vector<uint8_t> obs((size_t)T, 1);
  for (int32_t t = 0; t < T; ++t) {
    if (observed && !observed[t]) { obs[(size_t)t] = 0; continue; }
    // (the reference takes n_t = 0 and then filters with a latent value that is not a number)
    if (!(trials[t] >= 1) || trials[t] != std::floor(trials[t]) || !(trials[t] <= 2147483647.0))
      return fail(BA_E_INVALID, "trials must be integers of at least 1 at the observed steps");
    if (!(successes[t] >= 0) || successes[t] != std::floor(successes[t]))
      return fail(BA_E_INVALID, "successes must be non-negative integers");
    if (successes[t] > trials[t]) return fail(BA_E_INVALID, "The number of successes must not exceed the number of trials.");
    yo[(size_t)t] = successes[t];
    nt[(size_t)t] = trials[t];
  }
  int rc = ba_ss_set_data(e, T, p, yo.data(), X, observed);
  if (rc) return rc;
  // the logit path's view of the same data (n = T): X, successes, trials, X squared
  rc = upload_latent_data(e, T, p, X, yo.data(), nt.data(), /*squared=*/true, clt_threshold);
  if (rc) return rc;
  // a new model (v = 0, q = 4 / n_t) and a sampler whose latent data are not initialised
  e->ssp_observed = obs;
  e->ssp_trials = nt;
  e->lat.w.release();
  e->dssp_value.release();
  e->dssp_h.release();
  e->ssp_ready = false;
  e->data_kind = DATA_SS_LOGIT;
  return BA_OK;
}

int ba_ss_logit_get_latent(ba_engine *e, int64_t chain, double *value, double *precision) {
  ENGINE_PROLOGUE(e);
  return ssp_get_latent(e, DATA_SS_LOGIT, chain, value, precision);
}

int ba_ss_logit_set_latent(ba_engine *e, int64_t chain, const double *value, const double *precision) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  return ssp_set_latent(e, DATA_SS_LOGIT, chain, value, precision);
}

int ba_ss_logit_impute_state(ba_engine *e) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  return ssp_impute_state_entry(e, DATA_SS_LOGIT);
}

int ba_ss_logit_sweep(ba_engine *e, int32_t nsweeps) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  return ssp_sweep(e, DATA_SS_LOGIT, nsweeps);
}

}  // extern "C"
