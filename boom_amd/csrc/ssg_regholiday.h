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
//
// A hierarchical model (HierarchicalRegressionHolidayStateModel, bsts AddHierarchicalRegressionHoliday) is
// such a model with a flag: one width d <= RHH_MAX_WIDTH for all its holidays, the flat index h d + day, and the
// hyperparameters of its coefficient vectors' prior N(mu, Omega^-1) -- Sigma0^-1, Sigma0^-1 mu0 and S0 formed
// once here, by the Cholesky factor and inverse below (rhh_add_refusal, rhh_model).
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
  // a hierarchical model (HierarchicalRegressionHolidayStateModel; rhh_add_refusal): every width is `width`,
  // the prior above is not used; d x d matrices row-major at leading dimension d
  bool hier = false;
  int32_t width = 0;
  double nu0 = 0.0;                    // variance_guess_weight
  std::vector<double> sinv0, s0, sinv0mu0;      // Sigma0^-1, S0 = nu0 x variance_guess, Sigma0^-1 mu0: formed once
  std::vector<double> initial_mu, initial_omega;   // the reference's MvnModel(d): 0 and the identity
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

// The lower Cholesky factor of the d x d matrix A (row-major, leading dimension d; its lower triangle is
// read) into L, zero above the diagonal: false where a pivot is not positive and finite.
inline bool rh_cholesky(const double *A, int32_t d, double *L) {
  for (int32_t i = 0; i < d * d; ++i) L[i] = 0.0;
  for (int32_t j = 0; j < d; ++j)
    for (int32_t r = j; r < d; ++r) {
      double s = A[r * d + j];
      for (int32_t k = 0; k < j; ++k) s -= L[r * d + k] * L[j * d + k];
      if (r == j) {
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        L[j * d + j] = std::sqrt(s);
      } else {
        L[r * d + j] = s / L[j * d + j];
      }
    }
  return true;
}

// symmetric (to the bit) and positive definite, every entry finite
inline bool rh_is_spd(const double *A, int32_t d) {
  for (int32_t r = 0; r < d; ++r)
    for (int32_t c = 0; c < d; ++c)
      if (!std::isfinite(A[r * d + c]) || A[r * d + c] != A[c * d + r]) return false;
  std::vector<double> L((size_t)d * d);
  return rh_cholesky(A, d, L.data());
}

// the inverse of a symmetric positive definite matrix by its factor: W = L^-1, then W'W; false as rh_cholesky
inline bool rh_spd_inverse(const double *A, int32_t d, double *out) {
  std::vector<double> L((size_t)d * d), W((size_t)d * d, 0.0);
  if (!rh_cholesky(A, d, L.data())) return false;
  for (int32_t c = 0; c < d; ++c)
    for (int32_t i = c; i < d; ++i) {
      double s = i == c ? 1.0 : 0.0;
      for (int32_t k = c; k < i; ++k) s -= L[i * d + k] * W[k * d + c];
      W[i * d + c] = s / L[i * d + i];
    }
  for (int32_t r = 0; r < d; ++r)
    for (int32_t c = 0; c < d; ++c) {
      double s = 0.0;
      for (int32_t k = r > c ? r : c; k < d; ++k) s += W[k * d + r] * W[k * d + c];
      out[r * d + c] = s;
    }
  return true;
}

// ba_ss_add_hierarchical_regression_holiday's arguments against the list so far, as rh_add_refusal
inline const char *rhh_add_refusal(const std::vector<RhModel> &models, bool has_state_model, int32_t nholidays, int32_t width,
                                   const double *mean_prior_mean, const double *mean_prior_variance,
                                   const double *variance_guess, double variance_guess_weight,
                                   const double *initial_coefficients) {
  if (!mean_prior_mean || !mean_prior_variance || !variance_guess) return "null argument";
  if (nholidays < 1) return "a regression holiday model needs at least one holiday";
  if (!has_state_model) return "a regression holiday model goes on a list of state models: add a state model first";
  if ((int)models.size() >= RH_MAX_MODELS) return "more than 4 regression holiday models";
  if (width < 1) return "a holiday's width must be at least 1";
  if (width > RHH_MAX_WIDTH) return "the holidays of a hierarchical regression holiday model are at most 16 days wide";
  const int64_t n = (int64_t)nholidays * width;
  if (n + rh_total_coef(models) > RH_MAX_COEF) return "more than 256 regression holiday coefficients";
  for (int32_t i = 0; i < width; ++i)
    if (!std::isfinite(mean_prior_mean[i])) return "the prior mean of the holidays' mean must be finite";
  for (int32_t i = 0; i < width * width; ++i)
    if (!std::isfinite(mean_prior_variance[i]) || !std::isfinite(variance_guess[i]))
      return "the prior variance of the holidays' mean and the variance guess must be finite";
  if (!std::isfinite(variance_guess_weight)) return "the variance guess weight must be finite";
  if (!(variance_guess_weight > (double)(width - 1)))
    return "the variance guess weight must exceed the holidays' width less 1 (the Wishart prior's degrees of freedom)";
  if (!rh_is_spd(mean_prior_variance, width)) return "the prior variance of the holidays' mean must be symmetric and positive definite";
  if (!rh_is_spd(variance_guess, width)) return "the variance guess must be symmetric and positive definite";
  for (int64_t i = 0; initial_coefficients && i < n; ++i)
    if (!std::isfinite(initial_coefficients[i])) return "the initial coefficients must be finite";
  return nullptr;
}

// the model those arguments describe (they have passed rhh_add_refusal)
inline RhModel rhh_model(int32_t nholidays, int32_t width, const double *mean_prior_mean, const double *mean_prior_variance,
                         const double *variance_guess, double variance_guess_weight, const double *initial_coefficients) {
  RhModel m;
  const int32_t d = width;
  m.hier = true;
  m.width = d;
  m.widths.assign((size_t)nholidays, d);
  m.nu0 = variance_guess_weight;
  m.initial.assign((size_t)nholidays * d, 0.0);
  if (initial_coefficients) m.initial.assign(initial_coefficients, initial_coefficients + (size_t)nholidays * d);
  m.sinv0.assign((size_t)d * d, 0.0);
  rh_spd_inverse(mean_prior_variance, d, m.sinv0.data());
  m.s0.assign((size_t)d * d, 0.0);
  for (int32_t i = 0; i < d * d; ++i) m.s0[(size_t)i] = variance_guess[i] * variance_guess_weight;
  m.sinv0mu0.assign((size_t)d, 0.0);
  for (int32_t r = 0; r < d; ++r)
    for (int32_t c = 0; c < d; ++c) m.sinv0mu0[(size_t)r] += m.sinv0[(size_t)(r * d + c)] * mean_prior_mean[c];
  m.initial_mu.assign((size_t)d, 0.0);
  m.initial_omega.assign((size_t)d * d, 0.0);
  for (int32_t r = 0; r < d; ++r) m.initial_omega[(size_t)(r * d + r)] = 1.0;
  return m;
}

// ba_ss_set_hierarchical_regression_holiday's arguments: nullptr, or the refusal
inline const char *rhh_set_refusal(const RhModel &m, const double *mean, const double *precision) {
  if (!m.hier) return "not a hierarchical regression holiday model";
  if (!mean || !precision) return "null argument";
  for (int32_t i = 0; i < m.width; ++i)
    if (!std::isfinite(mean[i])) return "the mean must be finite";
  for (int32_t i = 0; i < m.width * m.width; ++i)
    if (!std::isfinite(precision[i])) return "the precision must be finite";
  if (!rh_is_spd(precision, m.width)) return "the precision must be symmetric and positive definite";
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
