// The list of state models of the structural state (ssg_spec.h holds its arithmetic): the entry points
// that build and read it, the calendars of the holidays and the calendar seasonals, and the Student
// trend's and the spike-and-slab autoregression's own entry points.
#include "engine_internal.h"

namespace boom_amd {

// The calendars of the random-walk holidays and the calendar seasonals: every such block needs one
// that covers the series and `extra` steps beyond it (a forecast's horizon); the packed table -- and
// the calendar seasonals' prefix counts -- go to the device when a calendar has changed.  Nothing
// runs on a default calendar.
// The dynamic regressions' predictors the same way: every block's rows cover the series and `extra`
// steps beyond it; the list's table goes to the device when a block's predictors have changed.
static int dyn_prepare(ba_engine *e, int64_t extra) {
  if (!e->ssm_set || !ssg_has(e->ssg, SSG_HAS_DYNREG)) return BA_OK;
  for (int b = 0; b < e->ssg.nblocks; ++b) {
    if (!e->ssg.blk[b].dynreg) continue;
    const int64_t n = (int64_t)e->dyn_predictors[b].size() / ssg_dyn_width(e->ssg.blk[b]);
    char buf[240];
    if (n < (int64_t)e->T) {
      std::snprintf(buf, sizeof buf, "the predictors of state model %d have %lld rows, the series has %d time points",
                    b, (long long)n, (int)e->T);
      return fail(BA_E_STATE, buf);
    }
    if (n < (int64_t)e->T + extra) {
      std::snprintf(buf, sizeof buf, "the predictors of state model %d have %lld rows: a forecast of horizon %lld needs %lld (the series' %d and the horizon)",
                    b, (long long)n, (long long)extra, (long long)((int64_t)e->T + extra), (int)e->T);
      return fail(BA_E_INVALID, buf);
    }
  }
  const int64_t rows = ssg_dyn_rows(e->ssg, e->dyn_predictors);   // (the shortest)
  const size_t count = (size_t)rows * (size_t)ssg_dyn_columns(e->ssg);
  if (e->dyn_rows == rows && e->ddyn.count == count) return BA_OK;
  const std::vector<double> table = ssg_pack_predictors(e->ssg, e->dyn_predictors, rows);
  HIP_TRY(hipStreamSynchronize(e->stream));   // (nothing in flight reads the table that is replaced)
  HIP_TRY(e->ddyn.resize(count));
  HIP_TRY(hipMemcpy(e->ddyn.ptr, table.data(), count * 8, hipMemcpyHostToDevice));
  e->dyn_rows = rows;
  return BA_OK;
}

// The regression holiday models' calendars the same way: every model's covers the series and `extra`
// steps beyond it; the shared table, the active steps and the counts go to the device, and every chain's
// series starts again from the data's, when a calendar or the data has changed.
static int rh_prepare(ba_engine *e, int64_t extra) {
  if (!e->ssm_set || e->rh_models.empty() || e->data_kind != DATA_STATE_SPACE) return BA_OK;
  int code = BA_OK;
  const std::string refused = rh_launch_refusal(e->rh_models, (int64_t)e->T, extra, &code);
  if (!refused.empty()) return fail(code, refused);
  const size_t C = (size_t)e->cfg.chains, T = (size_t)e->T;
  if (e->rh_count != 0 && e->drh_y.count == C * T) return BA_OK;
  const RhPacked K = rh_pack(e->rh_models, (int64_t)e->T, e->ss_observed.data());
  HIP_TRY(hipStreamSynchronize(e->stream));   // (nothing in flight reads the tables that are replaced)
  HIP_TRY(e->drh_table.resize(K.table.size()));
  HIP_TRY(e->drh_steps.resize(std::max<size_t>(K.steps.size(), 1)));
  HIP_TRY(e->drh_counts.resize(K.counts.size()));
  HIP_TRY(e->drh_y.resize(C * T));
  HIP_TRY(hipMemcpy(e->drh_table.ptr, K.table.data(), K.table.size() * 4, hipMemcpyHostToDevice));
  if (!K.steps.empty()) HIP_TRY(hipMemcpy(e->drh_steps.ptr, K.steps.data(), K.steps.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->drh_counts.ptr, K.counts.data(), K.counts.size() * 8, hipMemcpyHostToDevice));
  e->rh_count = K.count;
  e->rh_nsteps = (int32_t)K.steps.size();
  for (int k = 0; k <= RH_MAX_MODELS; ++k) e->rh_first[k] = K.first[k];
  e->rh_counts = K.counts;
  RhParams R;
  fill_rh_params(e, R);
  HIP_TRY(launch_rh_fill(e->stream, R, (int)e->T, (int)e->cfg.chains));
  return BA_OK;
}

int hol_prepare(ba_engine *e, int64_t extra) {
  if (int rc = dyn_prepare(e, extra)) return rc;
  if (int rc = rh_prepare(e, extra)) return rc;
  if (!e->ssm_set || !ssg_has(e->ssg, SSG_HAS_CALENDAR)) return BA_OK;
  for (int b = 0; b < e->ssg.nblocks; ++b) {
    const bool seas = ssg_is_calendar(e->ssg.blk[b]);
    if (!e->ssg.blk[b].holiday && !seas) continue;
    const int64_t n = seas ? (int64_t)e->season_calendar[b].size() : (int64_t)e->hol_calendar[b].size();
    const char *what = seas ? "season" : "holiday";
    char buf[240];
    if (n == 0) {
      if (seas)
        std::snprintf(buf, sizeof buf, "state model %d is a calendar seasonal without a calendar: call ba_ss_set_season_calendar first", b);
      else
        std::snprintf(buf, sizeof buf, "state model %d is a random-walk holiday without a calendar: call ba_ss_set_holiday_calendar first", b);
      return fail(BA_E_STATE, buf);
    }
    if (n < (int64_t)e->T) {
      std::snprintf(buf, sizeof buf, "the %s calendar of state model %d has %lld entries, the series has %d time points",
                    what, b, (long long)n, (int)e->T);
      return fail(BA_E_STATE, buf);
    }
    if (n < (int64_t)e->T + extra) {
      std::snprintf(buf, sizeof buf, "the %s calendar of state model %d has %lld entries: a forecast of horizon %lld needs %lld (the series' %d and the horizon)",
                    what, b, (long long)n, (long long)extra, (long long)((int64_t)e->T + extra), (int)e->T);
      return fail(BA_E_INVALID, buf);
    }
  }
  const int64_t count = ssg_calendar_count(e->ssg, e->hol_calendar, e->season_calendar);   // (the shortest)
  const size_t words = ssg_calendar_words(e->ssg, count);
  if (e->hol_cal_count == count && e->dhol_cal.count == words) return BA_OK;
  const std::vector<uint64_t> packed = ssg_pack_calendars(e->ssg, e->hol_calendar, e->season_calendar, count);
  HIP_TRY(hipStreamSynchronize(e->stream));   // (nothing in flight reads the tables that are replaced)
  HIP_TRY(e->dhol_cal.resize(words));
  HIP_TRY(hipMemcpy(e->dhol_cal.ptr, packed.data(), words * 8, hipMemcpyHostToDevice));
  e->hol_cal_count = count;
  return BA_OK;
}

// model->add_state(...) on the engine's copy of the specification (ssg_append, ssg_spec.h)
static int ssg_add(ba_engine *e, int32_t kind, const int32_t *iparams, const double *var_df,
                   const double *var_sigma_guess, const double *var_sigma_upper_limit,
                   const double *var_initial_sigma, const double *initial_phi,
                   const double *initial_state_mean, const double *initial_state_variance, int32_t dyn_xdim = 0) {
  const SsgInitial initial{e->ssg_initial_sigsq, e->ssg_initial_phi, e->ar_spike_prior,
                           e->slt_nu_kind, e->slt_nu_a, e->slt_nu_b, e->slt_initial_nu};
  const SsgModelArgs args{iparams, var_df, var_sigma_guess, var_sigma_upper_limit, var_initial_sigma,
                          initial_phi, initial_state_mean, initial_state_variance};
  // (dyn_xdim > 0: a dynamic regression of that many coefficients, ba_ss_add_dynamic_regression's)
  const SsgRefusal r = dyn_xdim > 0 ? ssg_append_dynreg(e->ssg, initial, ss_family(e->data_kind), dyn_xdim, args)
                                    : ssg_append(e->ssg, initial, ss_family(e->data_kind), kind, args);
  if (r.text) return fail(r.code, r.text);
  // (no calendar and no predictors yet)
  e->hol_calendar[e->ssg.nblocks - 1].clear();
  e->season_calendar[e->ssg.nblocks - 1].clear();
  e->dyn_predictors[e->ssg.nblocks - 1].clear();
  e->dynar_xdim[e->ssg.nblocks - 1] = 0;
  e->dyn_rows = 0;
  e->ssm_set = true;
  e->ss_level_set = false;
  e->dss_scratch.release();
  return BA_OK;
}
static void ssg_clear(ba_engine *e) {
  e->ssg = SsgSpec{};
  for (int b = 0; b < SSG_MAX_BLOCKS; ++b) { e->hol_calendar[b].clear(); e->season_calendar[b].clear(); e->dyn_predictors[b].clear(); e->dynar_xdim[b] = 0; }
  e->hol_cal_count = 0;
  e->dyn_rows = 0;
  e->rh_models.clear();   // (the regression holiday models belong to the list)
  e->rh_count = 0;
  for (int i = 0; i < 3; ++i) e->ssg_template_var[i] = -1;
  e->ssg_template_ar = -1;
  e->ssm_set = false;
  e->dss_scratch.release();
}

}  // namespace boom_amd

extern "C" {

int ba_ss_clear_state_models(ba_engine *e) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  ssg_clear(e);
  return BA_OK;
}

int ba_ss_add_state_model(ba_engine *e, int32_t kind, const int32_t *iparams, const double *var_df,
                          const double *var_sigma_guess, const double *var_sigma_upper_limit,
                          const double *var_initial_sigma, const double *initial_phi,
                          const double *initial_state_mean, const double *initial_state_variance) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (e->ss_level_set) ssg_clear(e);   // (a local-level specification is replaced, not extended)
  e->ss_level_set = false;
  return ssg_add(e, kind, iparams, var_df, var_sigma_guess, var_sigma_upper_limit, var_initial_sigma,
                 initial_phi, initial_state_mean, initial_state_variance);
}

int ba_ss_state_dimension(ba_engine *e, int32_t *state_dimension, int32_t *nblocks) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (state_dimension) *state_dimension = e->ssm_set ? e->ssg.m : (e->ss_level_set ? 1 : 0);
  if (nblocks) *nblocks = e->ssm_set ? e->ssg.nblocks : (e->ss_level_set ? 1 : 0);
  return BA_OK;
}

// a random-walk holiday's calendar: entry t is -1 (time t is not in the holiday's window) or the
// position of time t in the window, in [0, width)
int ba_ss_set_holiday_calendar(ba_engine *e, int32_t block, const int32_t *position, int64_t count) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!position || count <= 0) return fail(BA_E_INVALID, "bad argument");
  if (!e->ssm_set || block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  const SsgBlock &k = e->ssg.blk[block];
  if (ssg_is_calendar(k)) return fail(BA_E_INVALID, "not a random-walk holiday state model: a calendar seasonal's calendar goes through ba_ss_set_season_calendar");
  if (!k.holiday) return fail(BA_E_INVALID, "not a random-walk holiday state model");
  for (int64_t t = 0; t < count; ++t)
    if (position[t] < -1 || position[t] >= k.dim) {
      char buf[160];
      std::snprintf(buf, sizeof buf, "holiday calendar entry %lld is %d: it must be -1 (inactive) or a position in [0, %d)",
                    (long long)t, (int)position[t], (int)k.dim);
      return fail(BA_E_INVALID, buf);
    }
  e->hol_calendar[block].assign(position, position + count);
  e->hol_cal_count = 0;   // (packed again by the next call that launches)
  return BA_OK;
}

// position == nullptr: the count alone
int ba_ss_get_holiday_calendar(ba_engine *e, int32_t block, int32_t *position, int64_t *count) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (!e->ssm_set || block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  if (!e->ssg.blk[block].holiday) return fail(BA_E_INVALID, "not a random-walk holiday state model");
  const std::vector<int32_t> &c = e->hol_calendar[block];
  if (count) *count = (int64_t)c.size();
  if (position && !c.empty()) std::memcpy(position, c.data(), c.size() * sizeof(int32_t));
  return BA_OK;
}

// a calendar seasonal's calendar: entry t is 1 where time t starts a new season, else 0 (entry 0 is
// never read: no step leads into time 0)
int ba_ss_set_season_calendar(ba_engine *e, int32_t block, const uint8_t *new_season, int64_t count) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!new_season || count <= 0) return fail(BA_E_INVALID, "bad argument");
  if (!e->ssm_set || block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  if (!ssg_is_calendar(e->ssg.blk[block])) return fail(BA_E_INVALID, "not a calendar seasonal state model");
  for (int64_t t = 0; t < count; ++t)
    if (new_season[t] > 1) {
      char buf[160];
      std::snprintf(buf, sizeof buf, "season calendar entry %lld is %d: it must be 0 or 1 (time t starts a new season)",
                    (long long)t, (int)new_season[t]);
      return fail(BA_E_INVALID, buf);
    }
  e->season_calendar[block].assign(new_season, new_season + count);
  e->hol_cal_count = 0;   // (packed again by the next call that launches)
  return BA_OK;
}

// new_season == nullptr: the count alone
int ba_ss_get_season_calendar(ba_engine *e, int32_t block, uint8_t *new_season, int64_t *count) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (!e->ssm_set || block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  if (!ssg_is_calendar(e->ssg.blk[block])) return fail(BA_E_INVALID, "not a calendar seasonal state model");
  const std::vector<uint8_t> &c = e->season_calendar[block];
  if (count) *count = (int64_t)c.size();
  if (new_season && !c.empty()) std::memcpy(new_season, c.data(), c.size());
  return BA_OK;
}

// DynamicRegressionStateModel(X) with the independent random-walk sampler: a block of its own call,
// since it cannot exist without its data.  predictors: rows x xdim row-major, row t = x_t.
int ba_ss_add_dynamic_regression(ba_engine *e, int32_t xdim, const double *predictors, int64_t rows,
                                 const double *var_df, const double *var_sigma_guess,
                                 const double *var_sigma_upper_limit, const double *var_initial_sigma,
                                 const double *initial_state_mean, const double *initial_state_variance) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (!predictors) return fail(BA_E_INVALID, "null argument");
  if (xdim < 1) return fail(BA_E_INVALID, "a dynamic regression needs at least one predictor");
  if (rows <= 0) return fail(BA_E_INVALID, "a dynamic regression needs at least one row of predictors");
  if (ssg_dyn_check(predictors, rows, xdim) >= 0) return fail(BA_E_INVALID, "the predictors of a dynamic regression must be finite");
  if (e->ss_level_set) ssg_clear(e);   // (a local-level specification is replaced, not extended)
  e->ss_level_set = false;
  const int rc = ssg_add(e, SSG_DYNAMIC_REGRESSION, nullptr, var_df, var_sigma_guess, var_sigma_upper_limit,
                         var_initial_sigma, nullptr, initial_state_mean, initial_state_variance, xdim);
  if (rc) return rc;
  e->dyn_predictors[e->ssg.nblocks - 1].assign(predictors, predictors + (size_t)rows * (size_t)xdim);
  return BA_OK;
}

// DynamicRegressionArStateModel(X, lags) with DynamicRegressionArPosteriorSampler: xdim autoregression blocks
// with a row of data (ssg_append_dynreg_ar), all or none.  predictors: rows x xdim row-major, row t = x_t.
int ba_ss_add_dynamic_regression_ar(ba_engine *e, int32_t xdim, int32_t lags, const double *predictors, int64_t rows,
                                    const double *var_df, const double *var_sigma_guess,
                                    const double *var_sigma_upper_limit, const double *var_initial_sigma,
                                    const double *initial_phi, const double *initial_state_mean,
                                    const double *initial_state_variance, int32_t *first_block_out) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (!predictors) return fail(BA_E_INVALID, "null argument");
  if (xdim < 1) return fail(BA_E_INVALID, "a dynamic regression needs at least one predictor");
  if (rows <= 0) return fail(BA_E_INVALID, "a dynamic regression needs at least one row of predictors");
  if (ssg_dyn_check(predictors, rows, xdim) >= 0) return fail(BA_E_INVALID, "the predictors of a dynamic regression must be finite");
  // (a local-level specification is replaced, not extended -- once the append is known to go through)
  SsgSpec list = e->ss_level_set ? SsgSpec{} : e->ssg;
  const SsgInitial initial{e->ssg_initial_sigsq, e->ssg_initial_phi, e->ar_spike_prior,
                           e->slt_nu_kind, e->slt_nu_a, e->slt_nu_b, e->slt_initial_nu};
  const SsgModelArgs args{nullptr, var_df, var_sigma_guess, var_sigma_upper_limit, var_initial_sigma,
                          initial_phi, initial_state_mean, initial_state_variance};
  const SsgRefusal r = ssg_append_dynreg_ar(list, initial, ss_family(e->data_kind), xdim, lags, args);
  if (r.text) return fail(r.code, r.text);
  if (e->ss_level_set) ssg_clear(e);
  e->ss_level_set = false;
  e->ssg = list;
  const int first = e->ssg.nblocks - xdim;
  for (int i = 0; i < xdim; ++i) {
    const int b = first + i;
    e->hol_calendar[b].clear();
    e->season_calendar[b].clear();
    e->dyn_predictors[b].resize((size_t)rows);
    for (int64_t t = 0; t < rows; ++t) e->dyn_predictors[b][(size_t)t] = predictors[(size_t)t * xdim + i];
    e->dynar_first[b] = first;
    e->dynar_xdim[b] = xdim;
  }
  e->dyn_rows = 0;
  e->ssm_set = true;
  e->dss_scratch.release();
  if (first_block_out) *first_block_out = first;
  return BA_OK;
}

static const char *const dynar_not_first =
    "a block of an AR dynamic regression that is not the model's first: its predictors are set and read on the model's first block";

// replace a dynamic regression's predictors, or extend them (the rows past T serve forecasts: the
// reference's add_forecast_data)
int ba_ss_set_dynamic_predictors(ba_engine *e, int32_t block, const double *predictors, int64_t rows) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!predictors || rows <= 0) return fail(BA_E_INVALID, "bad argument");
  if (!e->ssm_set || block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  const SsgBlock &k = e->ssg.blk[block];
  if (!k.dynreg) return fail(BA_E_INVALID, "not a dynamic regression state model");
  if (const int xdim = e->dynar_xdim[block]) {   // (an AR dynamic regression: all its columns, on its first block)
    if (e->dynar_first[block] != block) return fail(BA_E_INVALID, dynar_not_first);
    if (ssg_dyn_check(predictors, rows, xdim) >= 0) return fail(BA_E_INVALID, "the predictors of a dynamic regression must be finite");
    for (int i = 0; i < xdim; ++i) {
      e->dyn_predictors[block + i].resize((size_t)rows);
      for (int64_t t = 0; t < rows; ++t) e->dyn_predictors[block + i][(size_t)t] = predictors[(size_t)t * xdim + i];
    }
    e->dyn_rows = 0;
    return BA_OK;
  }
  if (ssg_dyn_check(predictors, rows, k.dim) >= 0) return fail(BA_E_INVALID, "the predictors of a dynamic regression must be finite");
  e->dyn_predictors[block].assign(predictors, predictors + (size_t)rows * (size_t)k.dim);
  e->dyn_rows = 0;   // (packed again by the next call that launches)
  return BA_OK;
}

// predictors == nullptr: the row count alone
int ba_ss_get_dynamic_predictors(ba_engine *e, int32_t block, double *predictors, int64_t *rows) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (!e->ssm_set || block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  if (!e->ssg.blk[block].dynreg) return fail(BA_E_INVALID, "not a dynamic regression state model");
  const std::vector<double> &c = e->dyn_predictors[block];
  if (const int xdim = e->dynar_xdim[block]) {   // (an AR dynamic regression: rows x xdim, on its first block)
    if (e->dynar_first[block] != block) return fail(BA_E_INVALID, dynar_not_first);
    if (rows) *rows = (int64_t)c.size();
    if (predictors)
      for (int i = 0; i < xdim; ++i)
        for (size_t t = 0; t < c.size(); ++t) predictors[t * (size_t)xdim + i] = e->dyn_predictors[block + i][t];
    return BA_OK;
  }
  if (rows) *rows = (int64_t)c.size() / e->ssg.blk[block].dim;
  if (predictors && !c.empty()) std::memcpy(predictors, c.data(), c.size() * sizeof(double));
  return BA_OK;
}

// RegressionHolidayStateModel (ssg_regholiday.h): nholidays holidays of the given widths, one coefficient
// per day of each window, all under the prior N(prior_mean, prior_sd^2); no block of the list
int ba_ss_add_regression_holiday(ba_engine *e, int32_t nholidays, const int32_t *widths, double prior_mean,
                                 double prior_sd, const double *initial_coefficients, int32_t *model_out) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (const char *refused = rh_add_refusal(e->rh_models, e->ssm_set, nholidays, widths, prior_mean, prior_sd, initial_coefficients))
    return fail(BA_E_INVALID, refused);
  if (const char *refused = ssg_refusal(&e->ssg, ss_family(e->data_kind), SSG_USE_APPEND, SSG_REGRESSION_HOLIDAY))
    return fail(BA_E_STATE, refused);
  RhModel m;
  m.widths.assign(widths, widths + nholidays);
  m.prior_mean = prior_mean;
  m.prior_sd = prior_sd;
  m.initial.assign((size_t)m.ncoef(), 0.0);
  if (initial_coefficients) m.initial.assign(initial_coefficients, initial_coefficients + m.ncoef());
  e->rh_models.push_back(m);
  for (size_t k = 0; k < e->rh_models.size(); ++k) e->rh_first[k + 1] = e->rh_first[k] + e->rh_models[k].ncoef();
  for (size_t k = e->rh_models.size(); k < RH_MAX_MODELS; ++k) e->rh_first[k + 1] = e->rh_first[k];
  e->rh_count = 0;
  e->dss_scratch.release();   // (the chains start again, as after ba_ss_add_state_model)
  if (model_out) *model_out = (int32_t)e->rh_models.size() - 1;
  return BA_OK;
}

// a regression holiday model's calendar: entry t is -1 (no holiday of the model is active at time t) or
// the flat index offset_h + day of the coefficient that is
int ba_ss_set_regression_holiday_calendar(ba_engine *e, int32_t model, const int32_t *index, int64_t count) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!index || count <= 0) return fail(BA_E_INVALID, "bad argument");
  if (!e->ssm_set || model < 0 || model >= (int32_t)e->rh_models.size()) return fail(BA_E_INVALID, "regression holiday model index out of range");
  RhModel &m = e->rh_models[(size_t)model];
  const int64_t bad = rh_calendar_check(index, count, m.ncoef());
  if (bad >= 0) {
    char buf[200];
    std::snprintf(buf, sizeof buf, "regression holiday calendar entry %lld is %d: it must be -1 (inactive) or a coefficient index in [0, %d)",
                  (long long)bad, (int)index[bad], (int)m.ncoef());
    return fail(BA_E_INVALID, buf);
  }
  m.calendar.assign(index, index + count);
  e->rh_count = 0;   // (packed again by the next call that launches)
  return BA_OK;
}

// index == nullptr: the count alone
int ba_ss_get_regression_holiday_calendar(ba_engine *e, int32_t model, int32_t *index, int64_t *count) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (!e->ssm_set || model < 0 || model >= (int32_t)e->rh_models.size()) return fail(BA_E_INVALID, "regression holiday model index out of range");
  const std::vector<int32_t> &c = e->rh_models[(size_t)model].calendar;
  if (count) *count = (int64_t)c.size();
  if (index && !c.empty()) std::memcpy(index, c.data(), c.size() * sizeof(int32_t));
  return BA_OK;
}

static int rh_ready(ba_engine *e, int32_t model) {
  if (e->data_kind != DATA_STATE_SPACE) return fail(BA_E_STATE, set_data_first(DATA_STATE_SPACE));
  if (!e->ssm_set || e->rh_models.empty()) return fail(BA_E_STATE, "the list of state models holds no regression holiday model");
  if (model < 0 || model >= (int32_t)e->rh_models.size()) return fail(BA_E_INVALID, "regression holiday model index out of range");
  return ss_prepare(e);
}

// one chain's coefficients of model `model`, the totals its last observe_state left and the counts (the
// same for every chain); any output may be nullptr
int ba_ss_get_regression_holiday(ba_engine *e, int64_t chain, int32_t model, double *coefficients, double *totals,
                                 double *counts) {
  ENGINE_PROLOGUE(e);
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = rh_ready(e, model);
  if (rc) return rc;
  rc = ba_sync(e);
  if (rc) return rc;
  const size_t at = (size_t)chain * RH_MAX_COEF + (size_t)e->rh_first[model], n = (size_t)e->rh_models[(size_t)model].ncoef();
  if (coefficients) HIP_TRY(hipMemcpy(coefficients, e->drh_coef.ptr + at, n * 8, hipMemcpyDeviceToHost));
  if (totals) HIP_TRY(hipMemcpy(totals, e->drh_totals.ptr + at, n * 8, hipMemcpyDeviceToHost));
  if (counts) std::memcpy(counts, e->rh_counts.data() + e->rh_first[model], n * 8);
  return BA_OK;
}

// chain == -1: every chain
int ba_ss_set_regression_holiday(ba_engine *e, int64_t chain, int32_t model, const double *coefficients) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!coefficients) return fail(BA_E_INVALID, "null argument");
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = rh_ready(e, model);
  if (rc) return rc;
  const size_t n = (size_t)e->rh_models[(size_t)model].ncoef(), C = (size_t)e->cfg.chains;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(coefficients[i])) return fail(BA_E_INVALID, "the coefficients must be finite");
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t c = chain < 0 ? 0 : (size_t)chain; c < (chain < 0 ? C : (size_t)chain + 1); ++c)
    HIP_TRY(hipMemcpy(e->drh_coef.ptr + c * RH_MAX_COEF + (size_t)e->rh_first[model], coefficients, n * 8, hipMemcpyHostToDevice));
  return BA_OK;
}

// HierarchicalRegressionHolidayStateModel (ssg_regholiday.h: rhh_add_refusal): nholidays holidays of one
// width under beta_h ~ N(mu, Omega^-1) with mu and Omega drawn; one of the list's regression holiday models
int ba_ss_add_hierarchical_regression_holiday(ba_engine *e, int32_t nholidays, int32_t width,
                                              const double *mean_prior_mean, const double *mean_prior_variance,
                                              const double *variance_guess, double variance_guess_weight,
                                              const double *initial_coefficients, int32_t *model_out) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (const char *refused = rhh_add_refusal(e->rh_models, e->ssm_set, nholidays, width, mean_prior_mean, mean_prior_variance,
                                            variance_guess, variance_guess_weight, initial_coefficients))
    return fail(BA_E_INVALID, refused);
  if (const char *refused = ssg_refusal(&e->ssg, ss_family(e->data_kind), SSG_USE_APPEND, SSG_REGRESSION_HOLIDAY))
    return fail(BA_E_STATE, refused);
  e->rh_models.push_back(rhh_model(nholidays, width, mean_prior_mean, mean_prior_variance, variance_guess,
                                   variance_guess_weight, initial_coefficients));
  for (size_t k = 0; k < e->rh_models.size(); ++k) e->rh_first[k + 1] = e->rh_first[k] + e->rh_models[k].ncoef();
  for (size_t k = e->rh_models.size(); k < RH_MAX_MODELS; ++k) e->rh_first[k + 1] = e->rh_first[k];
  e->rh_count = 0;
  e->dss_scratch.release();   // (the chains start again, as after ba_ss_add_state_model)
  if (model_out) *model_out = (int32_t)e->rh_models.size() - 1;
  return BA_OK;
}

// one chain's hyper-mean (d) and hyper-precision (d x d, row-major) of model `model`; either may be nullptr
int ba_ss_get_hierarchical_regression_holiday(ba_engine *e, int64_t chain, int32_t model, double *mean, double *precision) {
  ENGINE_PROLOGUE(e);
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = rh_ready(e, model);
  if (rc) return rc;
  const RhModel &m = e->rh_models[(size_t)model];
  if (!m.hier) return fail(BA_E_INVALID, "not a hierarchical regression holiday model");
  rc = ba_sync(e);
  if (rc) return rc;
  const size_t W = RHH_MAX_WIDTH, d = (size_t)m.width, at = (size_t)chain * RH_MAX_MODELS + (size_t)model;
  if (mean) HIP_TRY(hipMemcpy(mean, e->drhh_mu.ptr + at * W, d * 8, hipMemcpyDeviceToHost));
  if (precision) {
    std::vector<double> om(W * W);
    HIP_TRY(hipMemcpy(om.data(), e->drhh_omega.ptr + at * W * W, W * W * 8, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < d; ++r)
      for (size_t c = 0; c < d; ++c) precision[r * d + c] = om[r * W + c];
  }
  return BA_OK;
}

// chain == -1: every chain
int ba_ss_set_hierarchical_regression_holiday(ba_engine *e, int64_t chain, int32_t model, const double *mean,
                                              const double *precision) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = rh_ready(e, model);
  if (rc) return rc;
  const RhModel &m = e->rh_models[(size_t)model];
  if (const char *refused = rhh_set_refusal(m, mean, precision)) return fail(BA_E_INVALID, refused);
  const size_t W = RHH_MAX_WIDTH, d = (size_t)m.width, C = (size_t)e->cfg.chains;
  std::vector<double> om(W * W, 0.0);
  for (size_t r = 0; r < d; ++r)
    for (size_t c = 0; c < d; ++c) om[r * W + c] = precision[r * d + c];
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t c = chain < 0 ? 0 : (size_t)chain; c < (chain < 0 ? C : (size_t)chain + 1); ++c) {
    const size_t at = c * RH_MAX_MODELS + (size_t)model;
    HIP_TRY(hipMemcpy(e->drhh_mu.ptr + at * W, mean, d * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->drhh_omega.ptr + at * W * W, om.data(), W * W * 8, hipMemcpyHostToDevice));
  }
  return BA_OK;
}

// MonthlyAnnualCycle's calendar from the date of the first observation (proleptic Gregorian): out[t] = 1
// where the day `t` days after (year, month, day) is the first of a month
int ba_monthly_cycle_calendar(int32_t year, int32_t month, int32_t day, int64_t count, uint8_t *out) {
  if (!out || count < 0) return fail(BA_E_INVALID, "bad argument");
  auto leap = [](int64_t y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; };
  auto days_in = [&](int64_t y, int mo) {
    static const int len[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    return len[mo - 1] + ((mo == 2 && leap(y)) ? 1 : 0);
  };
  if (month < 1 || month > 12 || day < 1 || day > days_in(year, month)) return fail(BA_E_INVALID, "not a date of the Gregorian calendar");
  int64_t y = year;
  int mo = month, d = day;
  for (int64_t t = 0; t < count; ++t) {
    out[t] = d == 1 ? 1 : 0;
    if (++d > days_in(y, mo)) {
      d = 1;
      if (++mo > 12) { mo = 1; ++y; }
    }
  }
  return BA_OK;
}

int ba_ss_set_structural(ba_engine *e, int32_t trend, int32_t nseasons, const double *var_df,
                         const double *var_sigma_guess, const double *var_sigma_upper_limit,
                         const double *var_initial_sigma, const double *initial_state_mean,
                         const double *initial_state_variance) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (!var_df || !var_sigma_guess || !var_sigma_upper_limit || !var_initial_sigma ||
      !initial_state_mean || !initial_state_variance)
    return fail(BA_E_INVALID, "null argument");
  if (trend != 1 && trend != 2) return fail(BA_E_INVALID, "trend must be 1 (local level) or 2 (local linear trend)");
  if (nseasons != 0 && nseasons < 2) return fail(BA_E_INVALID, "nseasons must be 0 or at least 2");
  const int m = trend + (nseasons > 0 ? nseasons - 1 : 0);
  if (m > SSG_MAX_STATE) return fail(BA_E_INVALID, "state dimension exceeds 64");
  for (int i = 0; i < 3; ++i) {
    const bool used = i == 0 || (i == 1 && trend == 2) || (i == 2 && nseasons > 0);
    if (used && var_sigma_upper_limit[i] < 0) return fail(BA_E_INVALID, "sigma_max must be non-negative.");
  }
  ssg_clear(e);
  int rc = ssg_add(e, trend == 2 ? SSG_LOCAL_LINEAR_TREND : SSG_LOCAL_LEVEL, nullptr, var_df, var_sigma_guess,
                   var_sigma_upper_limit, var_initial_sigma, nullptr, initial_state_mean, initial_state_variance);
  if (!rc && nseasons > 0) {
    const int32_t ip[3] = {nseasons, 1, 0};
    rc = ssg_add(e, SSG_SEASONAL, ip, var_df + 2, var_sigma_guess + 2, var_sigma_upper_limit + 2,
                 var_initial_sigma + 2, nullptr, initial_state_mean + trend, initial_state_variance + trend);
  }
  if (rc) {
    ssg_clear(e);
    return rc;
  }
  e->ssg_template_var[0] = 0;
  e->ssg_template_var[1] = trend == 2 ? 1 : -1;
  e->ssg_template_var[2] = nseasons > 0 ? trend : -1;
  return BA_OK;
}

int ba_ss_add_ar(ba_engine *e, int32_t lags, double prior_df, double sigma_guess,
                 double sigma_upper_limit, double initial_sigma, const double *initial_phi,
                 const double *initial_state_mean, const double *initial_state_variance) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  MUTATE(e);
  if (!e->ssm_set) return fail(BA_E_STATE, "call ba_ss_set_structural first");
  if (e->ssg_template_ar >= 0) return fail(BA_E_STATE, "the state already has an autoregression block");
  if (!initial_state_mean || !initial_state_variance) return fail(BA_E_INVALID, "null argument");
  if (lags < 1) return fail(BA_E_INVALID, "lags must be positive");
  const int32_t ip[3] = {lags, 0, 0};
  const int rc = ssg_add(e, SSG_AR, ip, &prior_df, &sigma_guess, &sigma_upper_limit, &initial_sigma, initial_phi,
                         initial_state_mean, initial_state_variance);
  if (rc) return rc;
  e->ssg_template_ar = e->ssg.nblocks - 1;
  return BA_OK;
}

// block `block` of one chain: its variance parameters, the state model's sufficient
// statistics of the last sweep, and for an autoregression block its coefficients and ArModel
// sufficient statistics
int ba_ss_get_state_model(ba_engine *e, int64_t chain, int32_t block, double *variances, double *suf_n,
                          double *suf_ss, double *phi, double *ar_xtx, double *ar_xty, double *ar_yty,
                          double *ar_n) {
  ENGINE_ACCESSOR_SERVED(e);
  if (!ss_kind(e->data_kind) || !e->ssm_set || e->dssm_work.count == 0)
    return fail(BA_E_STATE, "no structural state-space run yet");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  if (block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  const SsgBlock &k = e->ssg.blk[block];
  const bool is_sl = k.kind == SSG_SEMILOCAL;
  const bool is_ar = k.kind == SSG_AR || is_sl;   // (both keep coefficients and statistics in an autoregression slot)
  const bool is_student = block == e->ssg.student_block - 1;   // (phi: nu_level, nu_slope)
  if (!is_ar && ((phi && !is_student) || ar_xtx || ar_xty || ar_yty || ar_n))
    return fail(BA_E_INVALID, "not an autoregression state model");
  if (is_sl && (ar_xty || ar_yty))
    return fail(BA_E_INVALID, "a semilocal linear trend's Ar1Suf comes back through ar_xtx (six doubles) and ar_n");
  if (ss_la_serving(e)) {
    if (!suf_n && !suf_ss && !ar_xtx && !ar_xty && !ar_yty && !ar_n) {
      // the draw ba_ss_draw_next is serving, from the record
      const ba_engine::SsLa::Rows *r = nullptr;
      int rcr = ss_la_rows(e, chain, false, &r);
      if (rcr) return rcr;
      const size_t row = (size_t)e->ssla.served - 1;
      if (variances)
        for (int v = 0; v < k.nvar; ++v) variances[v] = r->var[row * e->ssla.nvar + k.var0 + v];
      if (phi)
        for (int i = 0; i < (is_sl ? 2 : k.lags); ++i) phi[i] = r->phi[row * e->ssla.nphi + (size_t)k.ar_index * AR_MAX + i];
      return BA_OK;
    }
    int rcs = ss_la_settle(e);   // (sufficient statistics are not in the record)
    if (rcs) return rcs;
  }
  int rc = ba_sync(e);
  if (rc) return rc;
  // (variances, n, sums of squares: up to SSG_MAX_VAR each -- a dynamic regression's d)
  HIP_TRY(pinned_reserve(e, (3 * SSG_MAX_VAR + AR_MAX + AR_SUF_STRIDE) * 8));
  double *hv = (double *)e->pinned, *hphi = hv + 3 * SSG_MAX_VAR, *hsuf = hphi + AR_MAX;
  const size_t at = (size_t)chain * SSG_MAX_VAR + k.var0;
  HIP_TRY(hipMemcpyAsync(hv, e->dssm_sigsq.ptr + at, (size_t)k.nvar * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(hv + SSG_MAX_VAR, e->dssm_n.ptr + at, (size_t)k.nvar * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(hv + 2 * SSG_MAX_VAR, e->dssm_ss.ptr + at, (size_t)k.nvar * 8, hipMemcpyDeviceToHost, e->stream));
  if (is_ar) {
    const size_t slot = (size_t)chain * SSG_MAX_AR + k.ar_index;
    HIP_TRY(hipMemcpyAsync(hphi, e->dar_phi.ptr + slot * AR_MAX, AR_MAX * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(hsuf, e->dar_suf.ptr + slot * AR_SUF_STRIDE, AR_SUF_STRIDE * 8, hipMemcpyDeviceToHost,
                           e->stream));
  }
  if (is_student && phi)
    HIP_TRY(hipMemcpyAsync(hphi, e->dslt_nu.ptr + (size_t)chain * 2, 2 * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (is_student && phi) { phi[0] = hphi[0]; phi[1] = hphi[1]; }
  for (int v = 0; v < k.nvar; ++v) {
    if (variances) variances[v] = hv[v];
    if (suf_n) suf_n[v] = hv[SSG_MAX_VAR + v];
    if (suf_ss) suf_ss[v] = hv[2 * SSG_MAX_VAR + v];
  }
  if (k.kind == SSG_SEMILOCAL) {
    // (phi, mu) of the slope's NonzeroMeanAr1Model; its Ar1Suf -- sumsq, sum, cross, n, first,
    // last value -- through ar_xtx (six doubles)
    if (phi) { phi[0] = hphi[0]; phi[1] = hphi[1]; }
    if (ar_xtx) std::memcpy(ar_xtx, hsuf, 6 * 8);
    if (ar_n) *ar_n = hsuf[3];
  } else if (is_ar) {
    const int L = k.lags;
    if (phi) std::memcpy(phi, hphi, (size_t)L * 8);
    if (ar_xtx)
      for (int i = 0; i < L; ++i)
        for (int j = 0; j < L; ++j) ar_xtx[(size_t)j * L + i] = hsuf[(size_t)i * AR_MAX + j];
    if (ar_xty) std::memcpy(ar_xty, hsuf + AR_SUF_XTY, (size_t)L * 8);
    if (ar_yty) *ar_yty = hsuf[AR_SUF_YTY];
    if (ar_n) *ar_n = hsuf[AR_SUF_N];
  }
  return BA_OK;
}

int ba_ss_get_ar(ba_engine *e, int64_t chain, double *phi, double *sigsq, double *suf_xtx,
                 double *suf_xty, double *suf_yty, double *suf_n) {
  if (!e) return fail(BA_E_INVALID, "null engine");
  if (!ss_kind(e->data_kind) || !e->ssm_set || e->ssg_template_ar < 0 || e->dar_phi.count == 0)
    return fail(BA_E_STATE, "no structural run with an autoregression block yet");
  return ba_ss_get_state_model(e, chain, e->ssg_template_ar, sigsq, nullptr, nullptr, phi, suf_xtx, suf_xty,
                               suf_yty, suf_n);
}

// ---- the Student local linear trend's own state (slt_kernel.hip)
static int slt_ready(ba_engine *e) {
  if (e->data_kind != DATA_STATE_SPACE) return fail(BA_E_STATE, set_data_first(DATA_STATE_SPACE));
  if (!e->ssm_set || !e->ssg.student_block)
    return fail(BA_E_STATE, "the list of state models holds no Student local linear trend");
  return ss_prepare(e);
}

int ba_ss_trend_get_weights(ba_engine *e, int64_t chain, double *level_w, double *slope_w) {
  ENGINE_PROLOGUE(e);
  if (!level_w || !slope_w) return fail(BA_E_INVALID, "null argument");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = slt_ready(e);
  if (rc) return rc;
  const size_t T = (size_t)e->T;
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(level_w, e->dslt_w.ptr + (size_t)chain * 2 * T, T * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(slope_w, e->dslt_w.ptr + (size_t)chain * 2 * T + T, T * 8, hipMemcpyDeviceToHost));
  return BA_OK;
}

int ba_ss_trend_set_weights(ba_engine *e, int64_t chain, const double *level_w, const double *slope_w) {
  ENGINE_PROLOGUE(e);
  MUTATE(e);
  if (!level_w || !slope_w) return fail(BA_E_INVALID, "null argument");
  if (chain < -1 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = slt_ready(e);
  if (rc) return rc;
  const size_t T = (size_t)e->T;
  for (size_t t = 0; t < T; ++t)
    if (!(level_w[t] > 0.0) || !std::isfinite(level_w[t]) || !(slope_w[t] > 0.0) || !std::isfinite(slope_w[t]))
      return fail(BA_E_INVALID, "Weights must be finite and positive.");
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::vector<double> w(level_w, level_w + T);   // (a chain's row: the level's weights, then the slope's)
  w.insert(w.end(), slope_w, slope_w + T);
  return write_chain_rows(e, e->dslt_w.ptr, chain, 2 * T, w.data());
}

// the GammaSuf of the weights the last observe_state drew: (n, sum, sum of logs) of the level, then of the slope
int ba_ss_trend_get_weight_suf(ba_engine *e, int64_t chain, double *out) {
  ENGINE_PROLOGUE(e);
  if (!out) return fail(BA_E_INVALID, "null argument");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  int rc = slt_ready(e);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, e->dslt_wsuf.ptr + (size_t)chain * 6, 6 * 8, hipMemcpyDeviceToHost));
  return BA_OK;
}

// the ArSpikeSlabSampler::draw() of every spike-and-slab autoregression alone
int ba_ss_autoar_draw_parameters(ba_engine *e) {
  ENGINE_PROLOGUE(e);
  e->table_ok = false;
  if (e->data_kind != DATA_STATE_SPACE) return fail(BA_E_STATE, set_data_first(DATA_STATE_SPACE));
  ArSpikeParams V;
  if (!fill_ar_spike_params(e, V)) return fail(BA_E_STATE, "the list of state models holds no spike-and-slab autoregression");
  int rc = ss_prepare(e);
  if (rc) return rc;
  SsParams S;
  fill_ss_params(e, S);
  fill_ar_spike_params(e, V);
  HIP_TRY(launch_ar_spike(e->stream, S, V));
  return BA_OK;
}

int ba_ss_get_ar_inclusion(ba_engine *e, int64_t chain, int32_t block, uint8_t *gamma) {
  ENGINE_PROLOGUE(e);   // (under a look-ahead: the chains back at the draw being served)
  if (!gamma) return fail(BA_E_INVALID, "null argument");
  if (!ss_kind(e->data_kind) || !e->ssm_set || e->dssm_work.count == 0)
    return fail(BA_E_STATE, "no structural state-space run yet");
  if (chain < 0 || chain >= e->cfg.chains) return fail(BA_E_INVALID, "chain index out of range");
  if (block < 0 || block >= e->ssg.nblocks) return fail(BA_E_INVALID, "state model index out of range");
  const SsgBlock &k = e->ssg.blk[block];
  if (!k.ar_spike || e->dar_gamma.count == 0) return fail(BA_E_INVALID, "not a spike-and-slab autoregression state model");
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(gamma, reinterpret_cast<const uint8_t *>(e->dar_gamma.ptr) + ((size_t)chain * SSG_MAX_AR + k.ar_index) * AR_MAX,
                    (size_t)k.lags, hipMemcpyDeviceToHost));
  return BA_OK;
}

// the block's sample_posterior() alone: sigma_level^2, nu_level, sigma_slope^2, nu_slope
int ba_ss_trend_draw_parameters(ba_engine *e) {
  ENGINE_PROLOGUE(e);
  e->table_ok = false;
  int rc = slt_ready(e);
  if (rc) return rc;
  SsParams S;
  fill_ss_params(e, S);
  SltParams U;
  fill_slt_params(e, U);
  HIP_TRY(launch_slt_params(e->stream, S, U));
  return BA_OK;
}

}  // extern "C"
