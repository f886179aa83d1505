// What is computed from the chains' current draw without moving them: the forecasts (Gaussian and
// the three families') and the one-step prediction errors.
#include "engine_internal.h"

extern "C" {

int ba_ss_forecast(ba_engine *e, int32_t horizon, const double *newX, double *out) {
  ENGINE_PROLOGUE(e);
  if (ss_refused(e, e->data_kind, SSG_USE_FORECAST)) return BA_E_STATE;
  if (!newX || !out || horizon <= 0) return fail(BA_E_INVALID, "bad argument");
  if (e->data_kind != DATA_STATE_SPACE || e->dss_scratch.count == 0 || !e->ss_initialized)
    return fail(BA_E_STATE, "no state draw yet: run ba_ss_sweep or ba_ss_impute_state first");
  int rc = hol_prepare(e, horizon);   // (a random-walk holiday: the calendar's entries T .. T + horizon - 1)
  if (rc) return rc;
  rc = ba_sync(e);
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p, h = (size_t)horizon;
  DevBuf<double> dnx, dout;
  HIP_TRY(dnx.resize(h * p));
  HIP_TRY(dout.resize(C * h));
  HIP_TRY(hipMemcpyAsync(dnx.ptr, newX, h * p * 8, hipMemcpyHostToDevice, e->stream));
  SsParams S;
  fill_ss_params(e, S);
  if (e->ssm_set) {
    RhParams R;
    fill_rh_params(e, R);   // (a regression holiday: its coefficient active at T + i on top)
    HIP_TRY(launch_ssm_forecast(e->stream, S, R, horizon, dnx.ptr, e->dpos_forecast.ptr, dout.ptr));
  }
  else
    HIP_TRY(launch_ss_forecast(e->stream, S, horizon, dnx.ptr, e->dpos_forecast.ptr, dout.ptr));
  HIP_TRY(hipMemcpyAsync(out, dout.ptr, C * h * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return BA_OK;
}

// One-step prediction errors, forecast variances and the log likelihood of the chains' current
// draw (ss_filter_kernel.hip).  An observer: it enqueues its own kernel and copies, and changes
// no stream position, state path, sufficient statistic or snapshot.  While ba_ss_draw_next
// serves a batch the parameters are the served row of the record, and the filter runs on a
// stream of its own behind the batch's event -- beside the batch that is running ahead.
int ba_ss_prediction_errors(ba_engine *e, int64_t chain_first, int64_t chain_count, int32_t standardize,
                            double *errors, double *variances, double *log_likelihood) {
  ENGINE_PROLOGUE_NOJOIN(e);
  {
    int rcj = pipe_join(e);
    if (rcj) return rcj;
  }
  if (ss_refused(e, e->data_kind, SSG_USE_PREDICTION_ERRORS)) return BA_E_STATE;
  if (e->data_kind != DATA_STATE_SPACE) return fail(BA_E_STATE, set_data_first(DATA_STATE_SPACE));
  if (!errors && !variances && !log_likelihood) return fail(BA_E_INVALID, "null argument");
  if (chain_first < 0 || chain_count <= 0 || chain_first >= e->cfg.chains || chain_count > e->cfg.chains - chain_first)
    return fail(BA_E_INVALID, "chain range out of bounds");
  const bool served = ss_la_serving(e);
  int rc = BA_OK;
  if (served) {
    rc = ss_la_wait(e);
  } else {
    rc = ss_prepare(e);
    if (!rc) rc = ba_sync(e);   // (a stopped chain: its error, as ba_ss_forecast)
  }
  if (rc) return rc;
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p, T = (size_t)e->T, n = (size_t)chain_count;
  hipStream_t s = e->stream;
  if (served) {
    if (!e->ssf_stream) HIP_TRY(hipStreamCreateWithFlags(&e->ssf_stream, hipStreamNonBlocking));
    s = e->ssf_stream;   // (ss_la_wait has waited for the batch's event on the host)
  }
  if (e->dssf_err.count < n * T) HIP_TRY(e->dssf_err.resize(n * T));
  if (variances && e->dssf_var.count < n * T) HIP_TRY(e->dssf_var.resize(n * T));
  if (e->dssf_ll.count < n) HIP_TRY(e->dssf_ll.resize(n));
  if (e->dssf_flag.count == 0) HIP_TRY(e->dssf_flag.resize(1));
  SsFilterParams F{};
  F.T = e->T;
  F.p = e->p;
  F.chain_first = (int32_t)chain_first;
  F.chain_count = (int32_t)chain_count;
  F.standardize = standardize ? 1 : 0;
  F.y = e->dss_y.ptr;
  if (e->ssm_set && !e->rh_models.empty()) {
    // regression holiday models: the chains' series less their effects, written from the coefficients as
    // they are now (a look-ahead above 1 is refused with such a model: always live)
    SsParams S;
    fill_ss_params(e, S);
    RhParams R;
    fill_rh_params(e, R);
    HIP_TRY(launch_rh_draw(s, S, R, 0));
    F.y = e->drh_y.ptr;
    F.y_stride = (int64_t)e->T;
  }
  F.X = e->dss_X.ptr;
  F.observed = e->dss_obs.ptr;
  if (e->ssm_set) {
    F.spec = reinterpret_cast<const SsgSpec *>(e->dssg_spec.ptr);
    F.m = e->ssg.m;
    F.nblocks = e->ssg.nblocks;
    F.nvar = e->ssg.nvar;
    F.nar = e->ssg.nar;
    if (e->ssg.student_block) {
      F.qw = e->dslt_w.ptr;   // (a look-ahead above 1 is refused with such a block: always live)
      F.qw_stride = 2 * (int64_t)T;
    }
    if (ssg_has(e->ssg, SSG_HAS_CALENDAR)) F.cal = e->dhol_cal.ptr;   // (one table for every draw: the record needs none)
    if (ssg_has(e->ssg, SSG_HAS_DYNREG)) {   // (the same: the predictors are shared by the chains and the draws)
      F.dyn = e->ddyn.ptr;
      F.dyn_cols = ssg_dyn_columns(e->ssg);
    }
  } else {
    // the local-level path: the same kernel on a one-block list
    SsgSpec one{};
    one.m = one.nblocks = one.nvar = 1;
    one.blk[0].kind = SSG_LOCAL_LEVEL;
    one.blk[0].dim = 1;
    one.blk[0].nvar = 1;
    one.blk[0].duration = 1;
    one.blk[0].ar_index = -1;
    one.a0[0] = e->ss_a0;
    one.P0[0] = e->ss_P0;
    if (e->dssf_spec.count == 0) HIP_TRY(e->dssf_spec.resize(sizeof(SsgSpec)));
    HIP_TRY(hipMemcpy(e->dssf_spec.ptr, &one, sizeof(SsgSpec), hipMemcpyHostToDevice));
    F.spec = reinterpret_cast<const SsgSpec *>(e->dssf_spec.ptr);
    F.m = F.nblocks = F.nvar = 1;
    F.nar = 0;
  }
  F.ld = (F.m + 1) | 1;
  if (served) {
    // the draw being served: row served - 1 of every chain, [slot][chain][round][...]
    const ba_engine::SsLa &A = e->ssla;
    const size_t L = (size_t)A.len, at0 = (size_t)A.slot * C * L + (size_t)A.served - 1;
    F.src.gamma = A.rgamma.ptr + at0 * p;
    F.src.beta = A.rbeta.ptr + at0 * p;
    F.src.sigsq = A.rsig.ptr + at0;
    F.src.var = A.rvar.ptr + at0 * A.nvar;
    F.src.phi = A.nphi ? A.rphi.ptr + at0 * A.nphi : nullptr;
    F.src.gamma_stride = F.src.beta_stride = (int64_t)(L * p);
    F.src.sigsq_stride = (int64_t)L;
    F.src.var_stride = (int64_t)(L * A.nvar);
    F.src.phi_stride = (int64_t)(L * A.nphi);
  } else {
    F.src.gamma = e->dgamma.ptr;
    F.src.beta = e->dbeta.ptr;
    F.src.sigsq = e->dsigsq.ptr;
    F.src.gamma_stride = F.src.beta_stride = (int64_t)p;
    F.src.sigsq_stride = 1;
    if (e->ssm_set) {
      F.src.var = e->dssm_sigsq.ptr;
      F.src.var_stride = SSG_MAX_VAR;
      F.src.phi = e->ssg.nar > 0 ? e->dar_phi.ptr : nullptr;
      F.src.phi_stride = SSG_MAX_AR * AR_MAX;
    } else {
      F.src.var = e->dlev_sigsq.ptr;   // (between calls the live value is the one the last state draw used)
      F.src.var_stride = 1;
    }
  }
  F.errors = e->dssf_err.ptr;
  F.variances = variances ? e->dssf_var.ptr : nullptr;
  F.loglik = e->dssf_ll.ptr;
  F.flag = e->dssf_flag.ptr;
  int32_t flag = 0;
  HIP_TRY(hipMemsetAsync(e->dssf_flag.ptr, 0x7f, 4, s));
  HIP_TRY(launch_ss_filter(s, F));
  if (errors) HIP_TRY(hipMemcpyAsync(errors, e->dssf_err.ptr, n * T * 8, hipMemcpyDeviceToHost, s));
  if (variances) HIP_TRY(hipMemcpyAsync(variances, e->dssf_var.ptr, n * T * 8, hipMemcpyDeviceToHost, s));
  if (log_likelihood) HIP_TRY(hipMemcpyAsync(log_likelihood, e->dssf_ll.ptr, n * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&flag, e->dssf_flag.ptr, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (flag >= 0 && flag < e->cfg.chains) {
    char buf[64];
    std::snprintf(buf, sizeof buf, " (chain %lld)", (long long)(e->cfg.chain_offset + (int64_t)flag));
    return fail(BA_E_FORECAST_VARIANCE, std::string("Found a zero (or negative) forecast variance!") + buf);
  }
  return BA_OK;
}

// One-step prediction errors of `horizon` rows behind the series (bsts.prediction.errors; the holdout
// instance of ss_filter_kernel.hip): from every chain's drawn final state, at the live parameters.  It enters
// as ba_ss_forecast does -- a look-ahead is settled to the draw being served, the calendars and predictors
// must cover T .. T + horizon - 1 -- and observes as ba_ss_prediction_errors does.
int ba_ss_holdout_prediction_errors(ba_engine *e, int64_t chain_first, int64_t chain_count, int32_t standardize,
                                    int32_t horizon, const double *newX, const double *newY, double *errors,
                                    double *variances) {
  ENGINE_PROLOGUE(e);
  if (ss_refused(e, e->data_kind, SSG_USE_HOLDOUT_ERRORS)) return BA_E_STATE;
  if (e->data_kind != DATA_STATE_SPACE) return fail(BA_E_STATE, set_data_first(DATA_STATE_SPACE));
  if (horizon <= 0) return fail(BA_E_INVALID, "the horizon must be positive");
  if (!newY || !errors || (!newX && e->p > 0)) return fail(BA_E_INVALID, "null argument");
  for (int32_t i = 0; i < horizon; ++i)
    if (!std::isfinite(newY[i])) {
      char buf[96];
      std::snprintf(buf, sizeof buf, "holdout response %d is not finite: a holdout has no missing steps", (int)i);
      return fail(BA_E_INVALID, buf);
    }
  if (chain_first < 0 || chain_count <= 0 || chain_first >= e->cfg.chains || chain_count > e->cfg.chains - chain_first)
    return fail(BA_E_INVALID, "chain range out of bounds");
  if (e->dss_scratch.count == 0 || !e->ss_initialized || (e->ssm_set && e->dssm_work.count == 0))
    return fail(BA_E_STATE, "no state draw yet: run ba_ss_sweep or ba_ss_impute_state first");
  int rc = hol_prepare(e, horizon);   // (the calendars' entries and the predictors' rows T .. T + horizon - 1)
  if (rc) return rc;
  rc = ba_sync(e);
  if (rc) return rc;
  const size_t p = (size_t)e->p, T = (size_t)e->T, n = (size_t)chain_count, h = (size_t)horizon;
  hipStream_t s = e->stream;
  if (e->dssf_err.count < n * h) HIP_TRY(e->dssf_err.resize(n * h));
  if (variances && e->dssf_var.count < n * h) HIP_TRY(e->dssf_var.resize(n * h));
  if (e->dssf_flag.count == 0) HIP_TRY(e->dssf_flag.resize(1));
  if (e->dssf_newy.count < h) HIP_TRY(e->dssf_newy.resize(h));
  if (p > 0 && e->dssf_newx.count < h * p) HIP_TRY(e->dssf_newx.resize(h * p));
  HIP_TRY(hipMemcpyAsync(e->dssf_newy.ptr, newY, h * 8, hipMemcpyHostToDevice, s));
  if (p > 0) HIP_TRY(hipMemcpyAsync(e->dssf_newx.ptr, newX, h * p * 8, hipMemcpyHostToDevice, s));
  SsFilterParams F{};
  F.T = horizon;
  F.time0 = e->T;
  F.p = e->p;
  F.chain_first = (int32_t)chain_first;
  F.chain_count = (int32_t)chain_count;
  F.standardize = standardize ? 1 : 0;
  F.y = e->dssf_newy.ptr;
  F.X = e->dssf_newx.ptr;
  if (e->ssm_set) {
    F.spec = reinterpret_cast<const SsgSpec *>(e->dssg_spec.ptr);
    F.m = e->ssg.m;
    F.nblocks = e->ssg.nblocks;
    F.nvar = e->ssg.nvar;
    F.nar = e->ssg.nar;
    if (ssg_has(e->ssg, SSG_HAS_CALENDAR)) F.cal = e->dhol_cal.ptr;
    if (ssg_has(e->ssg, SSG_HAS_DYNREG)) {
      F.dyn = e->ddyn.ptr;
      F.dyn_cols = ssg_dyn_columns(e->ssg);
    }
    // the state draw: [T][m] behind the chain's first m T doubles of work (ssg_forecast_kernel's start)
    F.state = e->dssm_work.ptr + (size_t)e->ssg.m * T + (T - 1) * (size_t)e->ssg.m;
    F.state_stride = ssm_work_stride(*e);
    F.src.var = e->dssm_sigsq.ptr;
    F.src.var_stride = SSG_MAX_VAR;
    F.src.phi = e->ssg.nar > 0 ? e->dar_phi.ptr : nullptr;
    F.src.phi_stride = SSG_MAX_AR * AR_MAX;
  } else {
    // the local-level path: a one-block list, as ba_ss_prediction_errors builds it
    SsgSpec one{};
    one.m = one.nblocks = one.nvar = 1;
    one.blk[0].kind = SSG_LOCAL_LEVEL;
    one.blk[0].dim = 1;
    one.blk[0].nvar = 1;
    one.blk[0].duration = 1;
    one.blk[0].ar_index = -1;
    one.a0[0] = e->ss_a0;
    one.P0[0] = e->ss_P0;
    if (e->dssf_spec.count == 0) HIP_TRY(e->dssf_spec.resize(sizeof(SsgSpec)));
    HIP_TRY(hipMemcpy(e->dssf_spec.ptr, &one, sizeof(SsgSpec), hipMemcpyHostToDevice));
    F.spec = reinterpret_cast<const SsgSpec *>(e->dssf_spec.ptr);
    F.m = F.nblocks = F.nvar = 1;
    F.nar = 0;
    // (ss_forecast_kernel's start)
    F.state = e->dss_scratch.ptr + (size_t)SS_STATE_ARRAY * ss_pitch(*e) + (size_t)(ss_lane_major(*e) ? lm_at((int)T - 1) : (int)T - 1);
    F.state_stride = (int64_t)SS_SCRATCH_ARRAYS * (int64_t)ss_pitch(*e);
    F.src.var = e->dlev_sigsq.ptr;
    F.src.var_stride = 1;
  }
  F.ld = (F.m + 1) | 1;
  F.src.gamma = e->dgamma.ptr;
  F.src.beta = e->dbeta.ptr;
  F.src.sigsq = e->dsigsq.ptr;
  F.src.gamma_stride = F.src.beta_stride = (int64_t)p;
  F.src.sigsq_stride = 1;
  F.errors = e->dssf_err.ptr;
  F.variances = variances ? e->dssf_var.ptr : nullptr;
  F.flag = e->dssf_flag.ptr;
  int32_t flag = 0;
  HIP_TRY(hipMemsetAsync(e->dssf_flag.ptr, 0x7f, 4, s));
  HIP_TRY(launch_ss_filter_holdout(s, F));
  HIP_TRY(hipMemcpyAsync(errors, e->dssf_err.ptr, n * h * 8, hipMemcpyDeviceToHost, s));
  if (variances) HIP_TRY(hipMemcpyAsync(variances, e->dssf_var.ptr, n * h * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&flag, e->dssf_flag.ptr, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (flag >= 0 && flag < e->cfg.chains) {
    char buf[64];
    std::snprintf(buf, sizeof buf, " (chain %lld)", (long long)(e->cfg.chain_offset + (int64_t)flag));
    return fail(BA_E_FORECAST_VARIANCE, std::string("Found a zero (or negative) forecast variance!") + buf);
  }
  return BA_OK;
}

}  // extern "C"

// ---- forecasts of the three families: simulate_forecast of StateSpaceStudentRegressionModel,
// StateSpacePoissonModel and StateSpaceLogitModel for every chain's current draw
// (ss_family_forecast_kernel.hip)

namespace boom_amd {

// scale: the horizon's exposures (Poisson) or trial counts (logit), validated; nullptr: ones
// (and for the Student-t family, which has none)
static int ss_family_forecast(ba_engine *e, DataKind kind, int32_t horizon, const double *newX, const double *scale,
                              double *out) {
  if (e->data_kind != kind) return fail(BA_E_STATE, set_data_first(kind));
  if (!newX || !out || horizon <= 0) return fail(BA_E_INVALID, "bad argument");
  const size_t C = (size_t)e->cfg.chains, p = (size_t)e->p, h = (size_t)horizon;
  const bool student = kind == DATA_SS_STUDENT, logit = kind == DATA_SS_LOGIT;
  std::vector<double> sc(h, 1.0);
  for (size_t i = 0; scale && i < h; ++i) {
    if (!(scale[i] >= 0.0) || !std::isfinite(scale[i]))
      return fail(BA_E_INVALID, logit ? "trial counts of a forecast must be non-negative and finite"
                                      : "exposures of a forecast must be non-negative and finite");
    sc[i] = logit ? std::round(scale[i]) : scale[i];   // (lround(trials[i]), StateSpaceLogitModel.cpp:245)
  }
  if (!e->ssm_set || e->dssm_work.count == 0 || !e->ss_initialized || (student && e->dstu_nu.count != C))
    return fail(BA_E_STATE, student ? "no state draw yet: run ba_ss_student_sweep or ba_ss_student_impute_state first"
                            : logit ? "no state draw yet: run ba_ss_logit_sweep or ba_ss_logit_impute_state first"
                                    : "no state draw yet: run ba_ss_poisson_sweep or ba_ss_poisson_impute_state first");
  int rc = ba_sync(e);
  if (rc) return rc;
  DevBuf<double> dnx, dsc, dout;
  HIP_TRY(dnx.resize(h * p));
  HIP_TRY(dsc.resize(h));
  HIP_TRY(dout.resize(C * h));
  HIP_TRY(hipMemcpyAsync(dnx.ptr, newX, h * p * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(dsc.ptr, sc.data(), h * 8, hipMemcpyHostToDevice, e->stream));
  SsParams S;
  fill_ss_params(e, S);
  const int family = student ? SS_FORECAST_STUDENT : logit ? SS_FORECAST_LOGIT : SS_FORECAST_POISSON;
  HIP_TRY(launch_ss_family_forecast(e->stream, S, family, horizon, dnx.ptr, dsc.ptr, e->dstu_nu.ptr,
                                    e->dpos_forecast.ptr, dout.ptr));
  HIP_TRY(hipMemcpyAsync(out, dout.ptr, C * h * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));   // (sc and the pageable copies are done with)
  return BA_OK;
}

}  // namespace boom_amd

extern "C" {

int ba_ss_student_forecast(ba_engine *e, int32_t horizon, const double *newX, double *out) {
  ENGINE_PROLOGUE(e);
  return ss_family_forecast(e, DATA_SS_STUDENT, horizon, newX, nullptr, out);
}

int ba_ss_poisson_forecast(ba_engine *e, int32_t horizon, const double *newX, const double *exposure, double *out) {
  ENGINE_PROLOGUE(e);
  return ss_family_forecast(e, DATA_SS_POISSON, horizon, newX, exposure, out);
}

int ba_ss_logit_forecast(ba_engine *e, int32_t horizon, const double *newX, const double *trials, double *out) {
  ENGINE_PROLOGUE(e);
  return ss_family_forecast(e, DATA_SS_LOGIT, horizon, newX, trials, out);
}

}  // extern "C"
