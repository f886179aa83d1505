// The regression holiday models of a list (RegressionHolidayStateModel, bsts AddRegressionHoliday) as
// host arithmetic: what a model is, the checks of its arguments and its calendar, and the three things
// the device reads that follow from the calendars and the observed flags -- the shared table, the list of
// active steps and the counts per coefficient.  No HIP call and nothing of the engine:
// tests/cpp/ssg_regholiday_check.cpp runs it on the CPU.
//
// The model's state is the constant 1 with variance 0 (T = 1, RQR = 0, a0 = 1, P0 = 0) and its Z_t is the
// coefficient of the holiday and day active at t: its whole effect is an offset on the observation
// series, so it takes no component of the structural kernel's state.  A model holds H holidays of widths
// w_0 .. w_{H-1}; its coefficients are flattened holiday by holiday, and its calendar is one int32 per
// time: -1, or the flat index offset_h + day.  One entry per time: "one holiday active at a time" within
// a model holds by construction.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/boom_amd.h"
#include "kalman_params.h"

namespace boom_amd {

struct RhModel {
  std::vector<int32_t> widths;         // w_h >= 1
  double prior_mean = 0.0, prior_sd = 1.0;   // the one prior N(mu, tau^2) of all its coefficients
  std::vector<double> initial;         // sum w_h coefficients
  std::vector<int32_t> calendar;       // as the caller gave it (empty: not set yet)
  int32_t ncoef() const { int32_t n = 0; for (int32_t w : widths) n += w; return n; }
};

inline int32_t rh_total_coef(const std::vector<RhModel> &models) {
  int32_t n = 0;
  for (const RhModel &m : models) n += m.ncoef();
  return n;
}

// ba_ss_add_regression_holiday's arguments against the list so far: nullptr, or the refusal (BA_E_INVALID).
// has_state_model: a state model has been added to the list.
inline const char *rh_add_refusal(const std::vector<RhModel> &models, bool has_state_model, int32_t nholidays,
                                  const int32_t *widths, double prior_mean, double prior_sd,
                                  const double *initial_coefficients) {
  if (!widths) return "null argument";
  if (nholidays < 1) return "a regression holiday model needs at least one holiday";
  if (!has_state_model) return "a regression holiday model goes on a list of state models: add a state model first";
  if ((int)models.size() >= RH_MAX_MODELS) return "more than 4 regression holiday models";
  int64_t n = 0;
  for (int32_t h = 0; h < nholidays; ++h) {
    if (widths[h] < 1) return "a holiday's width must be at least 1";
    n += widths[h];
    if (n > RH_MAX_COEF) break;
  }
  if (n + rh_total_coef(models) > RH_MAX_COEF) return "more than 256 regression holiday coefficients";
  if (!std::isfinite(prior_mean)) return "the prior mean must be finite";
  if (!(prior_sd > 0.0) || !std::isfinite(prior_sd)) return "the prior standard deviation must be positive and finite";
  for (int64_t i = 0; initial_coefficients && i < n; ++i)
    if (!std::isfinite(initial_coefficients[i])) return "the initial coefficients must be finite";
  return nullptr;
}

// a calendar's first entry outside {-1} u [0, n), or -1
inline int64_t rh_calendar_check(const int32_t *index, int64_t count, int32_t n) {
  for (int64_t t = 0; t < count; ++t)
    if (index[t] < -1 || index[t] >= n) return t;
  return -1;
}

// The calendars against a launch on a series of T steps (extra = 0) or a forecast of horizon `extra`:
// "" when every model's calendar covers T + extra entries, else the refusal; *code: BA_E_STATE for a
// calendar that is missing or shorter than the series, BA_E_INVALID for one shorter than T + horizon.
inline std::string rh_launch_refusal(const std::vector<RhModel> &models, int64_t T, int64_t extra, int *code) {
  char buf[240];
  for (size_t k = 0; k < models.size(); ++k) {
    const int64_t n = (int64_t)models[k].calendar.size();
    if (n == 0) {
      std::snprintf(buf, sizeof buf, "regression holiday model %d has no calendar: call ba_ss_set_regression_holiday_calendar first", (int)k);
      *code = BA_E_STATE;
      return buf;
    }
    if (n < T) {
      std::snprintf(buf, sizeof buf, "the calendar of regression holiday model %d has %lld entries, the series has %lld time points",
                    (int)k, (long long)n, (long long)T);
      *code = BA_E_STATE;
      return buf;
    }
    if (n < T + extra) {
      std::snprintf(buf, sizeof buf, "the calendar of regression holiday model %d has %lld entries: a forecast of horizon %lld needs %lld (the series' %lld and the horizon)",
                    (int)k, (long long)n, (long long)extra, (long long)(T + extra), (long long)T);
      *code = BA_E_INVALID;
      return buf;
    }
  }
  return std::string();
}

// what the device reads (RhParams): rebuilt when a calendar or the data changes
struct RhPacked {
  int64_t count = 0;             // the table's entries: the shortest calendar's
  std::vector<int32_t> table;    // count x RH_MAX_MODELS: the flat coefficient of model k active at t, or -1
  std::vector<int32_t> steps;    // the steps of [0, T) at which a model is active, ascending
  std::vector<double> counts;    // per flat coefficient: its observed active steps in [0, T)
  int32_t first[RH_MAX_MODELS + 1] = {};
};
// (the calendars have passed rh_calendar_check and rh_launch_refusal for T; observed: T flags, nullptr: all)
inline RhPacked rh_pack(const std::vector<RhModel> &models, int64_t T, const uint8_t *observed) {
  RhPacked R;
  for (size_t k = 0; k < models.size(); ++k) {
    R.first[k + 1] = R.first[k] + models[k].ncoef();
    const int64_t n = (int64_t)models[k].calendar.size();
    R.count = k == 0 ? n : (n < R.count ? n : R.count);
  }
  for (size_t k = models.size(); k < RH_MAX_MODELS; ++k) R.first[k + 1] = R.first[k];
  R.table.assign((size_t)R.count * RH_MAX_MODELS, -1);
  R.counts.assign((size_t)R.first[models.size()], 0.0);
  for (int64_t t = 0; t < R.count; ++t) {
    bool active = false;
    for (size_t k = 0; k < models.size(); ++k) {
      const int32_t j = models[k].calendar[(size_t)t];
      if (j < 0) continue;
      active = true;
      R.table[(size_t)t * RH_MAX_MODELS + k] = R.first[k] + j;
      if (t < T && (!observed || observed[t])) R.counts[(size_t)(R.first[k] + j)] += 1.0;
    }
    if (active && t < T) R.steps.push_back((int32_t)t);
  }
  return R;
}

}  // namespace boom_amd
