// The list of state models as arithmetic on SsgSpec, host side only: the table of the C-ABI's
// kinds, the append (model->add_state), the scalars that follow from the list (ssg_finish), the
// template shape, the rule book of what goes with what, and the packing of the calendars.  No
// HIP call and nothing of the engine: tests/cpp/ssg_spec_check.cpp runs it on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/boom_amd.h"
#include "kalman_params.h"
#include "student_params.h"

namespace boom_amd {

// ---- one row per C-ABI kind (include/boom_amd.h, ba_ss_add_state_model) ------------------
// the mark a kind leaves on its stored block: nvar = 0 | SsgSpec::student_block | SsgBlock::ar_spike |
// SsgBlock::holiday | phase SSG_PHASE_CALENDAR | SsgBlock::dynreg
enum SsgMark { SSG_MARK_NONE, SSG_MARK_STATIC, SSG_MARK_STUDENT, SSG_MARK_AR_SPIKE, SSG_MARK_HOLIDAY, SSG_MARK_CALENDAR, SSG_MARK_DYNREG };
// the sampler families: variance parameter v reads id base + 16 per earlier block that is a
// member of the parameter's family (a semilocal trend counts for the level family and for its
// slope's own; a static intercept, a holiday and a Student trend are in no level family)
enum { SSG_FAM_LEVEL = 1, SSG_FAM_SEASONAL = 2, SSG_FAM_AR = 4, SSG_FAM_TRIG = 8, SSG_FAM_SEMILOCAL = 16, SSG_FAM_HOLIDAY = 32 };
struct SsgSampler { int32_t family, base; };   // (family 0: the id is `base` itself)
struct SsgKind {
  int32_t stored;                  // SsgBlock::kind
  SsgMark mark;
  int32_t dim, dim_mul, dim_add;   // the dimension: dim, or where it is 0 dim_mul * iparams[0] + dim_add
  int32_t nvar, nslot, nerr;       // variance parameters, variance slots, state-error rows (0: one per component)
  bool ar_slot;                    // takes one of the SSG_MAX_AR autoregression slots
  bool iparams, phi;               // which of iparams / initial_phi it needs
  bool sigma_positive, zero_p0;    // its initial sigma must be positive; an initial state variance may be 0
  int32_t member;                  // the families its block counts for
  SsgSampler sampler[2];
};
inline const SsgKind *ssg_kind_row(int32_t kind) {
  static const SsgKind rows[11] = {
      /* 1 local level      */ {SSG_LOCAL_LEVEL, SSG_MARK_NONE, 1, 0, 0, 1, 1, 1, false, false, false, false, true, SSG_FAM_LEVEL, {{SSG_FAM_LEVEL, 1}, {0, 0}}},
      /* 2 linear trend     */ {SSG_LOCAL_LINEAR_TREND, SSG_MARK_NONE, 2, 0, 0, 2, 2, 2, false, false, false, false, false, SSG_FAM_LEVEL, {{SSG_FAM_LEVEL, 1}, {SSG_FAM_LEVEL, 6}}},
      /* 3 seasonal         */ {SSG_SEASONAL, SSG_MARK_NONE, 0, 1, -1, 1, 1, 1, false, true, false, false, false, SSG_FAM_SEASONAL, {{SSG_FAM_SEASONAL, 7}, {0, 0}}},
      /* 4 autoregression   */ {SSG_AR, SSG_MARK_NONE, 0, 1, 0, 1, 1, 1, true, true, false, true, false, SSG_FAM_AR, {{SSG_FAM_AR, 12}, {0, 0}}},
      /* 5 static intercept */ {SSG_LOCAL_LEVEL, SSG_MARK_STATIC, 1, 0, 0, 0, 1, 1, false, false, false, false, true, 0, {{0, 0}, {0, 0}}},
      /* 6 trig             */ {SSG_TRIG, SSG_MARK_NONE, 0, 2, 0, 1, 1, 0, false, true, true, false, false, SSG_FAM_TRIG, {{SSG_FAM_TRIG, 13}, {0, 0}}},
      /* 7 semilocal trend  */ {SSG_SEMILOCAL, SSG_MARK_NONE, 3, 0, 0, 2, 2, 2, true, true, true, true, false, SSG_FAM_LEVEL | SSG_FAM_SEMILOCAL, {{SSG_FAM_LEVEL, 1}, {SSG_FAM_SEMILOCAL, 14}}},
      /* 8 Student trend    */ {SSG_LOCAL_LINEAR_TREND, SSG_MARK_STUDENT, 2, 0, 0, 2, 2, 2, false, false, true, true, false, 0, {{0, (int32_t)SLT_PARAM_STREAM}, {0, (int32_t)SLT_PARAM_STREAM}}},
      /* 9 spike-slab AR    */ {SSG_AR, SSG_MARK_AR_SPIKE, 0, 1, 0, 1, 1, 1, true, true, true, true, false, SSG_FAM_AR, {{SSG_FAM_AR, 12}, {0, 0}}},
      /* 10 holiday         */ {SSG_LOCAL_LEVEL, SSG_MARK_HOLIDAY, 0, 1, 0, 1, 1, 1, false, true, false, false, false, SSG_FAM_HOLIDAY, {{SSG_FAM_HOLIDAY, 8}, {0, 0}}},
      /* 11 calendar seas.  */ {SSG_SEASONAL, SSG_MARK_CALENDAR, 0, 1, -1, 1, 1, 1, false, true, false, false, false, SSG_FAM_SEASONAL, {{SSG_FAM_SEASONAL, 7}, {0, 0}}},
  };
  return kind >= 1 && kind <= 11 ? &rows[kind - 1] : nullptr;
}
// The row of a dynamic regression of d coefficients (ba_ss_add_dynamic_regression: no kind of
// ba_ss_add_state_model, so no row of the table above): a local level per coefficient -- d variance
// parameters, d slots, a state-error row per component, sigma may start at 0 --, an initial state drawn
// by rmvn (positive variances).  Sampler ids: a convention of ours -- BOOM draws the d variances from
// one generator -- residue 10, which no family uses: variance slot i of the block reads 10 + 16 x (the
// dynamic coefficients earlier in the list, this block's first i among them); with at most 16 slots the
// largest id is 250.  SsgBlock::sid[0] holds the block's first, the others follow from it.
enum { SSG_DYNREG_SAMPLER = 10 };
inline const SsgKind *ssg_dynreg_row(int32_t d) {
  static SsgKind rows[SSG_MAX_STATE + 1];
  if (d < 1 || d > SSG_MAX_STATE) return nullptr;
  rows[d] = SsgKind{SSG_LOCAL_LEVEL, SSG_MARK_DYNREG, d, 0, 0, d, d, 0, false, false, false, false, false, 0, {{0, SSG_DYNREG_SAMPLER}, {0, 0}}};
  return &rows[d];
}
// the dynamic coefficients of the first `upto` blocks of a list (all: the columns of its predictor table)
// (a block of an AR dynamic regression -- stored kind SSG_AR -- holds one coefficient and its lags: one column)
inline int32_t ssg_dyn_width(const SsgBlock &k) { return !k.dynreg ? 0 : (k.kind == SSG_AR ? 1 : k.dim); }
inline int32_t ssg_dyn_columns(const SsgSpec &q, int upto = SSG_MAX_BLOCKS) {
  int32_t n = 0;
  for (int i = 0; i < q.nblocks && i < upto; ++i) n += ssg_dyn_width(q.blk[i]);
  return n;
}
// the C-ABI kind block i of a list was appended as (the one place that reads the marks back)
inline int32_t ssg_abi_kind(const SsgSpec &q, int i) {
  const SsgBlock &k = q.blk[i];
  if (i == q.student_block - 1) return SSG_STUDENT_TREND;
  if (k.holiday) return SSG_HOLIDAY;
  if (k.dynreg) return k.kind == SSG_AR ? (int32_t)SSG_DYNAMIC_REGRESSION_AR : (int32_t)SSG_DYNAMIC_REGRESSION;
  if (k.ar_spike) return SSG_AUTO_AR;
  if (ssg_is_calendar(k)) return SSG_CALENDAR_SEASONAL;
  if (k.kind == SSG_LOCAL_LEVEL && k.nvar == 0) return SSG_STATIC_INTERCEPT;
  return k.kind;
}
// (a block of an AR dynamic regression: an autoregression's row -- slot, family and sampler id are kind 4's)
inline const SsgKind &ssg_row_of(const SsgSpec &q, int i) {
  if (q.blk[i].dynreg) return q.blk[i].kind == SSG_AR ? *ssg_kind_row(SSG_AR) : *ssg_dynreg_row(q.blk[i].dim);
  return *ssg_kind_row(ssg_abi_kind(q, i));
}

// ---- what a list holds ---------------------------------------------------------------------
// a Student local linear trend (the general kernel's QT instances) | an autoregression with a
// spike-and-slab prior (ar_spike_kernel.hip) | a random-walk holiday | a calendar seasonal (the HD
// instances, a calendar per block) | a block of either kind: the list has a calendar | a dynamic
// regression (the DR instances, a table of predictors)
enum SsgFeature { SSG_HAS_STUDENT_TREND = 1, SSG_HAS_AR_SPIKE = 2, SSG_HAS_HOLIDAY = 4, SSG_HAS_CALENDAR_SEASONAL = 8,
                  SSG_HAS_CALENDAR = SSG_HAS_HOLIDAY | SSG_HAS_CALENDAR_SEASONAL, SSG_HAS_DYNREG = 16 };
inline bool ssg_has(const SsgSpec &q, int features) {
  int has = q.student_block ? SSG_HAS_STUDENT_TREND : 0;
  for (int i = 0; i < q.nblocks; ++i)
    has |= (q.blk[i].ar_spike ? SSG_HAS_AR_SPIKE : 0) | (q.blk[i].holiday ? SSG_HAS_HOLIDAY : 0) |
           (ssg_is_calendar(q.blk[i]) ? SSG_HAS_CALENDAR_SEASONAL : 0) | (q.blk[i].dynreg ? SSG_HAS_DYNREG : 0);
  return (has & features) != 0;
}

// does the block list have the shape the template kernel is compiled for?
// [local level | local linear trend] [seasonal, duration 1] [autoregression], m <= 16
inline void ssg_template_shape(const SsgSpec &q, int32_t *trend, int32_t *nseasons, int32_t *ar_lags) {
  *trend = *nseasons = *ar_lags = 0;
  if (q.nblocks < 1 || q.nblocks > 3 || q.m > 16) return;
  // (a Student trend, a spike-and-slab autoregression, a holiday, a calendar seasonal, a dynamic regression: the general kernel's instances)
  if (ssg_has(q, SSG_HAS_STUDENT_TREND | SSG_HAS_AR_SPIKE | SSG_HAS_CALENDAR | SSG_HAS_DYNREG)) return;
  for (int i = 0; i < q.nblocks; ++i)
    if (q.blk[i].nvar == 0) return;   // (a static intercept: the general kernel)
  int b = 0, tr = 0, ns = 0, lags = 0;
  if (q.blk[0].kind == SSG_LOCAL_LEVEL) tr = 1;
  else if (q.blk[0].kind == SSG_LOCAL_LINEAR_TREND) tr = 2;
  else return;
  b = 1;
  if (b < q.nblocks && q.blk[b].kind == SSG_SEASONAL) {
    if (q.blk[b].duration != 1) return;
    ns = q.blk[b].nseasons;
    ++b;
  }
  if (b < q.nblocks && q.blk[b].kind == SSG_AR) {
    lags = q.blk[b].lags;
    ++b;
  }
  if (b != q.nblocks) return;
  *trend = tr;
  *nseasons = ns;
  *ar_lags = lags;
}

// ---- the rule book: which state model goes with which observation family, with a Student trend
// in the same list, and with the look-ahead, the forecast and the prediction errors ---------------
enum SsFamily { SS_FAMILY_GAUSSIAN, SS_FAMILY_STUDENT, SS_FAMILY_POISSON, SS_FAMILY_LOGIT };
enum SsgUse { SSG_USE_APPEND, SSG_USE_LAUNCH, SSG_USE_LOOKAHEAD, SSG_USE_FORECAST, SSG_USE_PREDICTION_ERRORS, SSG_USE_HOLDOUT_ERRORS };
// The refusal (BA_E_STATE) of `use` under observation family `family`, or nullptr.  q: the list
// (nullptr: none is set).  SSG_USE_APPEND: `kind` is about to be appended to q; SSG_USE_LOOKAHEAD:
// a look-ahead above 1; SSG_USE_FORECAST: ba_ss_forecast, the Gaussian family's.  Where two
// refusals apply, the first below is given.  regholidays: the regression holiday models the list carries
// (ssg_regholiday.h: no blocks of q; SSG_USE_APPEND with kind SSG_REGRESSION_HOLIDAY: one is about to be added).
inline const char *ssg_refusal(const SsgSpec *q, SsFamily family, SsgUse use, int32_t kind = 0, int regholidays = 0) {
  static const char *const only_gaussian[6] = {
      "the Student local linear trend is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)",
      "the spike-and-slab autoregression is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)",
      "the random-walk holiday is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)",
      "the calendar seasonal is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)",
      "the dynamic regression is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)",
      "the regression holiday is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)"};
  static const char *const dynreg_student = "a list that holds both a dynamic regression and a Student local linear trend is not built";
  static const char *const dynreg_holiday = "a list that holds both a dynamic regression and a random-walk holiday is not built";
  static const char *const dynreg_calseas = "a list that holds both a dynamic regression and a calendar seasonal is not built";
  static const char *const holiday_student = "a list that holds both a random-walk holiday and a Student local linear trend is not built";
  static const char *const calseas_student = "a list that holds both a calendar seasonal and a Student local linear trend is not built";
  static const int special[5] = {SSG_HAS_STUDENT_TREND, SSG_HAS_AR_SPIKE, SSG_HAS_HOLIDAY, SSG_HAS_CALENDAR_SEASONAL, SSG_HAS_DYNREG};
  const bool other = family != SS_FAMILY_GAUSSIAN;
  auto has = [&](int f) { return q && ssg_has(*q, f); };
  switch (use) {
    case SSG_USE_APPEND:
      if (kind == SSG_STUDENT_TREND) {
        if (has(SSG_HAS_HOLIDAY)) return holiday_student;
        if (has(SSG_HAS_CALENDAR_SEASONAL)) return calseas_student;
        if (has(SSG_HAS_DYNREG)) return dynreg_student;
        return other ? only_gaussian[0] : nullptr;
      }
      if (kind == SSG_AUTO_AR) return other ? only_gaussian[1] : nullptr;
      if (kind == SSG_HOLIDAY)
        return other ? only_gaussian[2] : (has(SSG_HAS_STUDENT_TREND) ? holiday_student : (has(SSG_HAS_DYNREG) ? dynreg_holiday : nullptr));
      if (kind == SSG_CALENDAR_SEASONAL)
        return other ? only_gaussian[3] : (has(SSG_HAS_STUDENT_TREND) ? calseas_student : (has(SSG_HAS_DYNREG) ? dynreg_calseas : nullptr));
      if (kind == SSG_DYNAMIC_REGRESSION || kind == SSG_DYNAMIC_REGRESSION_AR) {   // (ssg_append_dynreg's, ssg_append_dynreg_ar's)
        if (other) return only_gaussian[4];
        if (has(SSG_HAS_STUDENT_TREND)) return dynreg_student;
        if (has(SSG_HAS_HOLIDAY)) return dynreg_holiday;
        return has(SSG_HAS_CALENDAR_SEASONAL) ? dynreg_calseas : nullptr;
      }
      if (kind == SSG_REGRESSION_HOLIDAY) return other ? only_gaussian[5] : nullptr;   // (beside every Gaussian block)
      return nullptr;
    case SSG_USE_LAUNCH:
      for (int i = 0; other && i < 5; ++i)
        if (has(special[i])) return only_gaussian[i];
      return other && regholidays > 0 ? only_gaussian[5] : nullptr;
    case SSG_USE_LOOKAHEAD:
      if (has(SSG_HAS_STUDENT_TREND)) return "the look-ahead does not carry a Student local linear trend's weights: use a look-ahead of 1";
      return regholidays > 0 ? "the look-ahead does not carry a regression holiday's coefficients: use a look-ahead of 1" : nullptr;
    case SSG_USE_FORECAST:
      if (family == SS_FAMILY_STUDENT) return "forecasts with Student-t observation noise are not implemented";
      if (family == SS_FAMILY_POISSON) return "forecasts with Poisson observation noise are not implemented";
      if (family == SS_FAMILY_LOGIT) return "forecasts with binomial observation noise are not implemented";
      return has(SSG_HAS_STUDENT_TREND) ? "forecasts with a Student local linear trend are not implemented" : nullptr;
    case SSG_USE_PREDICTION_ERRORS:
      return other ? "one-step prediction errors are built for the Gaussian observation model only" : nullptr;
    case SSG_USE_HOLDOUT_ERRORS:   // (ba_ss_holdout_prediction_errors)
      if (other) return "holdout prediction errors are built for the Gaussian observation model only";
      // (the reference's const method filters the block in its MIXTURE behaviour and reads its weight vectors at
      // T + i, past their end -- StudentLocalLinearTrend.cpp:178-185)
      if (has(SSG_HAS_STUDENT_TREND))
        return "holdout prediction errors with a Student local linear trend are not defined: the reference reads the trend's weights past the end of the series";
      return regholidays > 0 ? "holdout prediction errors with a regression holiday model are not built" : nullptr;
  }
  return nullptr;
}

// ---- the scalars of the specification that follow from the block list ----------------------
inline void ssg_finish(SsgSpec &q) {
  // P's leading dimension: odd (a lane per column and a lane per row both conflict-free), and
  // one of the four values ssg_simsmooth_kernel is compiled for
  q.ld = q.m <= 16 ? 17 : (q.m <= 32 ? 33 : (q.m <= 60 ? 61 : 65));
  // state-error rows: one per variance slot, except that a trig block's every component has one
  q.nerr = 0;
  for (int i = 0; i < q.nblocks; ++i) {
    q.blk[i].err0 = q.nerr;
    const int32_t nerr = ssg_row_of(q, i).nerr;
    q.nerr += nerr ? nerr : q.blk[i].dim;
  }
  // steps per block of the passes: the most that leaves FOUR workgroups to a CU's 160 KB of
  // LDS (all 1024 chains of a launch resident; at m = 59 sixteen steps left room for three,
  // and the launch ran as two rounds), never below 8; see ssg_pass_lds_doubles
  // (a list with dynamic regressions: a time block's predictor rows as well, staged once per wave)
  const int ndyn = ssg_dyn_columns(q);
  q.bl = 64;
  while (q.bl > 8 && (2 * q.bl * q.m + q.m * q.ld + q.bl * (q.nerr + 1) + SSG_MAX_STATE + 8 +
                      q.nar * AR_MAX * (AR_MAX + 1) + 2 * q.bl * ndyn) * 8 > 39 * 1024)
    q.bl /= 2;
}
// ArModel's constructor: "Attempt to initialize ArModel with an illegal value of the
// autoregression coefficients." (the quick bound, then the step-down recursion)
inline bool ar_stationary_host(const double *phi, int lags) {
  double a[AR_MAX], b[AR_MAX], sum = 0;
  for (int i = 0; i < lags; ++i) { a[i] = phi[i]; sum += std::fabs(a[i]); }
  if (sum < 1) return true;
  for (int k = lags; k >= 1; --k) {
    const double r = a[k - 1];
    if (!(std::fabs(r) < 1)) return false;
    for (int j = 0; j + 1 < k; ++j) b[j] = (a[j] + r * a[k - 2 - j]) / (1 - r * r);
    for (int j = 0; j + 1 < k; ++j) a[j] = b[j];
  }
  return true;
}
// the Philox sampler id of variance parameter v of a block of kind `row` about to be appended:
// level 1, slope 6, seasonal 7, holiday 8, autoregression 12, trig 13, a semilocal slope 14 for
// the first block of its family, + 16 for every earlier block of the family (a Student trend's
// sampler reads SLT_PARAM_STREAM: in no family)
inline int ssg_stream_id(const SsgSpec &q, const SsgKind &row, int v) {
  int occ = 0;
  for (int i = 0; i < q.nblocks; ++i) occ += (ssg_row_of(q, i).member & row.sampler[v].family) != 0;
  return row.sampler[v].base + 16 * occ;
}

// ---- the append: model->add_state(...) on a specification -----------------------------------
struct SsgRefusal { int code; const char *text; };   // (BA_OK, nullptr): appended
// the arrays of ba_ss_add_state_model
struct SsgModelArgs {
  const int32_t *iparams;
  const double *var_df, *var_sigma_guess, *var_sigma_upper_limit, *var_initial_sigma, *initial_phi, *initial_state_mean,
      *initial_state_variance;
};
// what the chains' parameters start from, host side (the engine's fields): the variances by slot, the
// coefficients by autoregression slot, the spike-and-slab priors by autoregression slot, the Student
// trend's nu priors (kind, a, b) and initial values of level and slope
struct SsgInitial {
  double *sigsq;                   // [SSG_MAX_VAR]
  double (*phi)[AR_MAX];           // [SSG_MAX_AR]
  ArSpikePrior *ar_spike_prior;    // [SSG_MAX_AR]
  int *nu_kind;                    // [2], as nu_a, nu_b and nu
  double *nu_a, *nu_b, *nu;
};

// ArStateModel + ArSpikeSlabSampler: iparams = {lags, truncate, max_flips, allow_model_selection};
// initial_phi = {coefficients, slab mean, inclusion probabilities (lags each), slab precision (lags x lags)}
inline const char *ar_spike_prior_parse(const int32_t *iparams, const double *initial_phi, ArSpikePrior &R) {
  const int L = iparams[0];
  const double *mu = initial_phi + L, *pi = initial_phi + 2 * L, *om = initial_phi + 3 * L;
  R = ArSpikePrior{};
  for (int i = 0; i < L; ++i) {
    if (!std::isfinite(mu[i])) return "the slab's mean must be finite";
    if (!(pi[i] >= 0.0 && pi[i] <= 1.0)) return "prior inclusion probabilities must lie in [0, 1]";
    R.mu[i] = mu[i];
    R.pi[i] = pi[i];
    R.log_pi[i] = std::log(pi[i]);
    R.log_1mpi[i] = std::log(1 - pi[i]);
  }
  double ch[AR_MAX][AR_MAX] = {};
  for (int i = 0; i < L; ++i)
    for (int j = 0; j < L; ++j) {
      const double a = om[(size_t)j * L + i], b = om[(size_t)i * L + j];
      if (!std::isfinite(a) || !(std::fabs(a - b) <= 1e-12 * (std::fabs(a) + std::fabs(b))))
        return "the slab's precision must be symmetric positive definite";
      R.siginv[i * AR_MAX + j] = a;
    }
  for (int j = 0; j < L; ++j) {
    for (int i = j; i < L; ++i) {
      double sacc = R.siginv[i * AR_MAX + j];
      for (int t = 0; t < j; ++t) sacc -= ch[i][t] * ch[j][t];
      if (i == j) {
        if (!(sacc > 0.0)) return "the slab's precision must be symmetric positive definite";
        ch[j][j] = std::sqrt(sacc);
      } else {
        ch[i][j] = sacc / ch[j][j];
      }
    }
  }
  R.truncate = iparams[1] != 0;
  R.max_flips = iparams[2];
  R.select = iparams[3] != 0;
  if (R.truncate && !ar_stationary_host(initial_phi, L)) return "the initial autoregression coefficients are not stationary";
  return nullptr;
}

inline SsgRefusal ssg_append_tail(SsgSpec &q, SsgInitial I, int32_t kind, const SsgKind *row, SsgBlock k,
                                   const ArSpikePrior &spike, const SsgModelArgs &A);
inline SsgRefusal ssg_append(SsgSpec &q, SsgInitial I, SsFamily family, int32_t kind, const SsgModelArgs &A) {
  auto invalid = [](const char *text) { return SsgRefusal{BA_E_INVALID, text}; };
  const SsgKind *row = ssg_kind_row(kind);
  // (a static intercept has no parameter: the var_* arrays are not read)
  if (((!row || row->nvar > 0) && (!A.var_df || !A.var_sigma_guess || !A.var_sigma_upper_limit || !A.var_initial_sigma)) ||
      !A.initial_state_mean || !A.initial_state_variance)
    return invalid("null argument");
  if (q.nblocks >= SSG_MAX_BLOCKS) return invalid("more than 8 state models");
  if (!row)
    return invalid("state model kind must be 1 (local level), 2 (local linear trend), 3 (seasonal), 4 (autoregression), 5 (static intercept), 6 (trig), 7 (semilocal linear trend), 8 (Student local linear trend), 9 (spike-and-slab autoregression), 10 (random-walk holiday) or 11 (calendar seasonal)");
  if ((row->iparams && !A.iparams) || (row->phi && !A.initial_phi)) return invalid("null argument");
  const int32_t *ip = A.iparams;
  const double *phi = A.initial_phi;
  const char *refused = nullptr;
  SsgBlock k{};
  k.kind = row->stored;
  k.nvar = row->nvar;
  k.duration = 1;
  k.ar_index = row->ar_slot ? q.nar : -1;
  k.ar_spike = row->mark == SSG_MARK_AR_SPIKE;
  k.holiday = row->mark == SSG_MARK_HOLIDAY;
  ArSpikePrior spike{};
  switch (kind) {
    case SSG_SEASONAL:
    case SSG_CALENDAR_SEASONAL:
      // SeasonalStateModelBase: "'nseasons' must be positive"; one season has no state
      if (ip[0] < 2) return invalid("nseasons must be at least 2");
      k.nseasons = ip[0];
      if (kind == SSG_CALENDAR_SEASONAL) {
        // iparams = {nseasons}; its season starts come through ba_ss_set_season_calendar
        // (duration and phase stay 1 and SSG_PHASE_CALENDAR: one family, one sampler id with kind 3)
        if ((refused = ssg_refusal(&q, family, SSG_USE_APPEND, kind))) return {BA_E_STATE, refused};
        k.phase = SSG_PHASE_CALENDAR;
        break;
      }
      if (ip[1] < 1) return invalid("season_duration must be positive");
      // (the kernels keep a block's duration and its running phase in 16-bit fields)
      if (ip[1] > 65535) return invalid("season_duration exceeds 65535");
      k.duration = ip[1];
      // new_season(t): (t - time_of_first_observation) is a multiple of the duration
      k.phase = ((ip[2] % k.duration) + k.duration) % k.duration;
      break;
    case SSG_HOLIDAY:
      // RandomWalkHolidayStateModel: iparams = {width}, the holiday's maximum window width; its
      // calendar comes through ba_ss_set_holiday_calendar
      if (ip[0] < 1 || ip[0] > SSG_MAX_STATE - 1) return invalid("a random-walk holiday's width must lie in [1, 63]");
      if ((refused = ssg_refusal(&q, family, SSG_USE_APPEND, kind))) return {BA_E_STATE, refused};
      break;
    case SSG_TRIG:
      // TrigStateModel: "At least one frequency needed ..."; the rotations as the transition
      // matrix holds them: (cos, sin) per frequency in initial_phi
      if (ip[0] < 1) return invalid("At least one frequency needed to initialize TrigStateModel.");
      if (2 * ip[0] > SSG_MAX_STATE) return invalid("state dimension exceeds 64");
      k.nfreq = ip[0];
      break;
    case SSG_SEMILOCAL:
      // SemilocalLinearTrendStateModel(level, slope): iparams = {force_stationary,
      // force_ar1_positive}; initial_phi = {slope mean prior mu, sigma, AR(1) coefficient prior mu,
      // sigma, initial mu, initial phi}
      if (ip[1] && !ip[0])
        return invalid("force_ar1_positive without force_stationary (a one-sided truncation of the slope's "
                       "AR(1) coefficient) is not built");
      if (!(phi[1] > 0) || !(phi[3] > 0)) return invalid("the slope's prior standard deviations must be positive");
      if (q.nar >= SSG_MAX_AR) return invalid("more than 4 autoregression / semilocal state models");
      k.sl_truncate = ip[0] != 0;
      k.sl_positive = ip[1] != 0;
      break;
    case SSG_STUDENT_TREND:
      // StudentLocalLinearTrendStateModel(sigma_level, nu_level, sigma_slope, nu_slope): initial_phi =
      // {nu_level prior kind, a, b, nu_slope prior kind, a, b, initial nu_level, initial nu_slope}; on
      // the device a local linear trend block (SsgSpec::student_block names it) with weights
      if (q.student_block) return invalid("at most one Student local linear trend per list of state models");
      if ((refused = ssg_refusal(&q, family, SSG_USE_APPEND, kind))) return {BA_E_STATE, refused};
      for (int c = 0; c < 2; ++c) {
        const double pk = phi[3 * c], a = phi[3 * c + 1], b = phi[3 * c + 2], nu = phi[6 + c];
        if (pk != STUDENT_NU_UNIFORM && pk != STUDENT_NU_GAMMA) return invalid("nu prior kind must be 0 (uniform) or 1 (gamma)");
        if (pk == STUDENT_NU_UNIFORM ? !(a < b) || !std::isfinite(a) || !std::isfinite(b) : !(a > 0) || !(b > 0))
          return invalid("nu prior: uniform needs a < b, gamma needs positive shape and rate");
        const bool ok = std::isfinite(nu) && nu > 0 && (pk != STUDENT_NU_UNIFORM || (nu >= a && nu <= b));
        if (!ok) return invalid("the initial nu must be positive and have positive prior density");
      }
      break;
    case SSG_AR:
    case SSG_AUTO_AR:
      if (ip[0] < 1) return invalid("lags must be positive");
      if (ip[0] > AR_MAX) return invalid("more than 16 lags");
      if (q.nar >= SSG_MAX_AR) return invalid("more than 4 autoregression state models");
      k.lags = ip[0];
      if (kind == SSG_AUTO_AR) {
        if ((refused = ssg_refusal(&q, family, SSG_USE_APPEND, kind))) return {BA_E_STATE, refused};
        if ((refused = ar_spike_prior_parse(ip, phi, spike))) return invalid(refused);
      }
      break;
    default:
      break;
  }
  k.dim = row->dim ? row->dim : row->dim_mul * ip[0] + row->dim_add;
  return ssg_append_tail(q, I, kind, row, k, spike, A);
}
// the append's second half -- the limits, the arrays' checks, the block into the list --, shared with
// ssg_append_dynreg: `k` has its kind, marks and dimension, `row` is its row
inline SsgRefusal ssg_append_tail(SsgSpec &q, SsgInitial I, int32_t kind, const SsgKind *row, SsgBlock k,
                                  const ArSpikePrior &spike, const SsgModelArgs &A) {
  auto invalid = [](const char *text) { return SsgRefusal{BA_E_INVALID, text}; };
  const double *phi = A.initial_phi;
  if (q.m + k.dim > SSG_MAX_STATE) return invalid("state dimension exceeds 64");
  if (q.nvar + row->nslot > SSG_MAX_VAR) return invalid("more than 16 variance parameters");
  for (int v = 0; v < k.nvar; ++v) {
    if (A.var_sigma_upper_limit[v] < 0) return invalid("sigma_max must be non-negative.");
    if (row->sigma_positive && !(A.var_initial_sigma[v] > 0)) return invalid("initial sigma must be positive");
  }
  for (int i = 0; i < k.dim; ++i) {
    // (a multivariate initial state goes through a Cholesky factor in the reference: it
    // needs a positive variance; the local level model alone does not)
    const bool ok = A.initial_state_variance[i] > 0.0 || (row->zero_p0 && A.initial_state_variance[i] == 0.0) ||
                    (kind == SSG_SEMILOCAL && i == 2);   // (the slope's long-run mean: a parameter, variance 0 whatever is passed)
    if (!ok) return invalid("initial state variances must be positive");
  }
  if (kind == SSG_AR && phi && !ar_stationary_host(phi, k.lags)) return invalid("the initial autoregression coefficients are not stationary");
  k.first = q.m;
  k.var0 = q.nvar;
  for (int v = 0; v < k.nvar; ++v) {
    const int vi = k.var0 + v;
    // ChisqModel(df, sigma_guess): 2 alpha = df, 2 beta = df sigma^2
    q.prior_df[vi] = 2 * (A.var_df[v] / 2.0);
    q.prior_ss[vi] = 2 * (A.var_df[v] * A.var_sigma_guess[v] * A.var_sigma_guess[v] / 2.0);
    q.sigma_max[vi] = A.var_sigma_upper_limit[v];
    I.sigsq[vi] = A.var_initial_sigma[v] * A.var_initial_sigma[v];
    if (row->mark != SSG_MARK_DYNREG) k.sid[v] = ssg_stream_id(q, *row, v);
  }
  if (row->mark == SSG_MARK_DYNREG) k.sid[0] = SSG_DYNREG_SAMPLER + 16 * ssg_dyn_columns(q);
  if (row->mark == SSG_MARK_STATIC) {
    // StaticInterceptStateModel: T = 1, RQR = 0, nothing to learn and no sampler -- a local level
    // whose variance (a slot of its own: variance 0, a sampler that is never run) is 0
    q.prior_df[k.var0] = 0.0;
    q.prior_ss[k.var0] = 0.0;
    q.sigma_max[k.var0] = std::numeric_limits<double>::infinity();
    I.sigsq[k.var0] = 0.0;
  }
  for (int i = 0; i < k.dim; ++i) {
    q.a0[k.first + i] = A.initial_state_mean[i];
    q.P0[k.first + i] = A.initial_state_variance[i];
    q.trig_c[k.first + i] = kind == SSG_TRIG ? phi[2 * (i / 2)] : 0.0;
    q.trig_s[k.first + i] = kind == SSG_TRIG ? phi[2 * (i / 2) + 1] : 0.0;
  }
  if (row->ar_slot) {
    for (int i = 0; i < AR_MAX; ++i) I.phi[k.ar_index][i] = (row->stored == SSG_AR && phi && i < k.lags) ? phi[i] : 0.0;
    if (row->mark == SSG_MARK_AR_SPIKE) I.ar_spike_prior[k.ar_index] = spike;
    q.nar += 1;
  }
  if (kind == SSG_SEMILOCAL) {
    I.phi[k.ar_index][0] = phi[5];   // phi
    I.phi[k.ar_index][1] = phi[4];   // mu
    for (int i = 0; i < 4; ++i) q.sl_prior[k.ar_index][i] = phi[i];
    // initial_state_mean()[2] = slope->mu() (per chain, per draw: the kernel's), variance 0
    q.a0[k.first + 2] = phi[4];
    q.P0[k.first + 2] = 0.0;
  }
  if (row->mark == SSG_MARK_STUDENT) {
    q.student_block = q.nblocks + 1;
    for (int c = 0; c < 2; ++c) {
      I.nu_kind[c] = (int)phi[3 * c];
      I.nu_a[c] = phi[3 * c + 1];
      I.nu_b[c] = phi[3 * c + 2];
      I.nu[c] = phi[6 + c];
    }
  }
  q.blk[q.nblocks] = k;
  q.nblocks += 1;
  q.m += k.dim;
  q.nvar += row->nslot;
  ssg_finish(q);
  return {BA_OK, nullptr};
}

// DynamicRegressionStateModel(X) + DynamicRegressionIndependentPosteriorSampler on a specification
// (ba_ss_add_dynamic_regression): d coefficients, one ChisqModel(df, sigma_guess) and sigma upper limit
// each.  The predictors themselves are the engine's (ssg_dyn_check: finite).
inline SsgRefusal ssg_append_dynreg(SsgSpec &q, SsgInitial I, SsFamily family, int32_t d, const SsgModelArgs &A) {
  auto invalid = [](const char *text) { return SsgRefusal{BA_E_INVALID, text}; };
  if (!A.var_df || !A.var_sigma_guess || !A.var_sigma_upper_limit || !A.var_initial_sigma || !A.initial_state_mean ||
      !A.initial_state_variance)
    return invalid("null argument");
  if (q.nblocks >= SSG_MAX_BLOCKS) return invalid("more than 8 state models");
  if (d < 1) return invalid("a dynamic regression needs at least one predictor");
  if (q.m + (int64_t)d > SSG_MAX_STATE) return invalid("state dimension exceeds 64");
  if (const char *refused = ssg_refusal(&q, family, SSG_USE_APPEND, SSG_DYNAMIC_REGRESSION)) return {BA_E_STATE, refused};
  SsgBlock k{};
  k.kind = SSG_LOCAL_LEVEL;
  k.nvar = d;
  k.duration = 1;
  k.ar_index = -1;
  k.dim = d;
  k.dynreg = 1 + ssg_dyn_columns(q);
  return ssg_append_tail(q, I, SSG_DYNAMIC_REGRESSION, ssg_dynreg_row(d), k, ArSpikePrior{}, A);
}
// DynamicRegressionArStateModel(X, lags) + DynamicRegressionArPosteriorSampler on a specification
// (ba_ss_add_dynamic_regression_ar): xdim consecutive blocks of stored kind SSG_AR and dimension lags, one per
// coefficient -- block i's first component is the coefficient, observed through column i of the model's
// predictors (SsgBlock::dynreg), the others are its lags -- each with what an autoregression (kind 4) has: an
// autoregression slot, a variance slot, a state-error row, the AR family's sampler id.  The var_* arrays
// hold xdim entries (an initial sigma is positive, as kind 4's), initial_phi (nullptr: zeros; every row stationary), initial_state_mean and
// initial_state_variance xdim x lags.  Limits: 1 <= lags <= AR_MAX, 1 <= xdim, and the list's: SSG_MAX_AR
// autoregression slots (so xdim <= 4), SSG_MAX_BLOCKS blocks, state dimension 64, 16 variance slots.
// All xdim blocks are appended, or none.
inline SsgRefusal ssg_append_dynreg_ar(SsgSpec &q, SsgInitial I, SsFamily family, int32_t xdim, int32_t lags, const SsgModelArgs &A) {
  auto invalid = [](const char *text) { return SsgRefusal{BA_E_INVALID, text}; };
  if (!A.var_df || !A.var_sigma_guess || !A.var_sigma_upper_limit || !A.var_initial_sigma || !A.initial_state_mean ||
      !A.initial_state_variance)
    return invalid("null argument");
  if (xdim < 1) return invalid("a dynamic regression needs at least one predictor");
  if (lags < 1) return invalid("lags must be positive");
  if (lags > AR_MAX) return invalid("more than 16 lags");
  if (q.nblocks + (int64_t)xdim > SSG_MAX_BLOCKS) return invalid("more than 8 state models");
  if (q.nar + (int64_t)xdim > SSG_MAX_AR) return invalid("more than 4 autoregression state models");
  if (q.m + (int64_t)xdim * lags > SSG_MAX_STATE) return invalid("state dimension exceeds 64");
  if (const char *refused = ssg_refusal(&q, family, SSG_USE_APPEND, SSG_DYNAMIC_REGRESSION_AR)) return {BA_E_STATE, refused};
  const SsgSpec before = q;
  const double zeros[AR_MAX] = {};
  for (int i = 0; i < xdim; ++i) {
    SsgBlock k{};
    k.kind = SSG_AR;
    k.nvar = 1;
    k.duration = 1;
    k.ar_index = q.nar;
    k.lags = lags;
    k.dim = lags;
    k.dynreg = 1 + ssg_dyn_columns(q);
    const SsgModelArgs Ai{nullptr, A.var_df + i, A.var_sigma_guess + i, A.var_sigma_upper_limit + i, A.var_initial_sigma + i,
                          A.initial_phi ? A.initial_phi + (size_t)i * lags : zeros, A.initial_state_mean + (size_t)i * lags,
                          A.initial_state_variance + (size_t)i * lags};
    const SsgRefusal r = ssg_append_tail(q, I, SSG_AR, ssg_kind_row(SSG_AR), k, ArSpikePrior{}, Ai);
    if (r.text) {
      q = before;
      return r;
    }
  }
  return {BA_OK, nullptr};
}
// the predictors of a dynamic regression, rows x xdim row-major: the first entry that is not finite, or -1
inline int64_t ssg_dyn_check(const double *predictors, int64_t rows, int32_t xdim) {
  for (int64_t i = 0; i < rows * (int64_t)xdim; ++i)
    if (!std::isfinite(predictors[i])) return i;
  return -1;
}
// the shortest predictor table of a list's dynamic blocks (-1: the list has none) ...
inline int64_t ssg_dyn_rows(const SsgSpec &q, const std::vector<double> *predictors) {
  int64_t rows = -1;
  for (int b = 0; b < q.nblocks; ++b) {
    if (!q.blk[b].dynreg) continue;
    const int64_t n = (int64_t)predictors[b].size() / ssg_dyn_width(q.blk[b]);
    rows = rows < 0 ? n : std::min(rows, n);
  }
  return rows;
}
// ... and the list's table (SsParams::dyn): row t = the blocks' x_t side by side, in state order
inline std::vector<double> ssg_pack_predictors(const SsgSpec &q, const std::vector<double> *predictors, int64_t rows) {
  const int cols = ssg_dyn_columns(q);
  std::vector<double> table((size_t)rows * (size_t)cols, 0.0);
  for (int b = 0; b < q.nblocks; ++b) {
    if (!q.blk[b].dynreg) continue;
    const int c0 = q.blk[b].dynreg - 1, d = ssg_dyn_width(q.blk[b]);
    for (int64_t t = 0; t < rows; ++t)
      for (int i = 0; i < d; ++i) table[(size_t)t * cols + c0 + i] = predictors[b][(size_t)t * d + i];
  }
  return table;
}

// ---- the calendars of the random-walk holidays and the calendar seasonals, packed -----------
// `holiday[b]` / `season[b]`: block b's calendar as the caller gave it (SSG_MAX_BLOCKS of each).
// The table's entries: the shortest calendar's (-1: the list has no calendar block) ...
inline int64_t ssg_calendar_count(const SsgSpec &q, const std::vector<int32_t> *holiday, const std::vector<uint8_t> *season) {
  int64_t count = -1;
  for (int b = 0; b < q.nblocks; ++b) {
    if (!q.blk[b].holiday && !ssg_is_calendar(q.blk[b])) continue;
    const int64_t n = ssg_is_calendar(q.blk[b]) ? (int64_t)season[b].size() : (int64_t)holiday[b].size();
    count = count < 0 ? n : std::min(count, n);
  }
  return count;
}
// ... its 64-bit words: the table, then -- a calendar seasonal in the list -- nblocks rows of int32 prefix counts
inline size_t ssg_calendar_words(const SsgSpec &q, int64_t count) {
  const size_t nstarted = ssg_has(q, SSG_HAS_CALENDAR_SEASONAL) ? (size_t)q.nblocks * (size_t)count : 0;
  return (size_t)count + (nstarted + 1) / 2;
}
// ... and the words themselves (SsParams::cal): byte b of entry t is a holiday's position at time t or
// SSG_CAL_OFF, a calendar seasonal's SSG_CAL_SEASON bit; row b behind the table counts the seasons
// block b has started in (0, t]
inline std::vector<uint64_t> ssg_pack_calendars(const SsgSpec &q, const std::vector<int32_t> *holiday,
                                                const std::vector<uint8_t> *season, int64_t count) {
  std::vector<uint64_t> packed(ssg_calendar_words(q, count), 0);
  std::fill(packed.begin(), packed.begin() + count, (uint64_t)SSG_CAL_NONE);
  int32_t *started = reinterpret_cast<int32_t *>(packed.data() + count);
  for (int b = 0; b < q.nblocks; ++b) {
    if (ssg_is_calendar(q.blk[b])) {
      // (entry 0 is never read: no step leads into time 0)
      int32_t *row = started + (size_t)b * (size_t)count;
      int32_t run = 0;
      for (int64_t t = 1; t < count; ++t) {
        if (season[b][(size_t)t]) {
          packed[(size_t)t] |= (uint64_t)SSG_CAL_SEASON << (8 * b);
          ++run;
        }
        row[t] = run;
      }
      continue;
    }
    if (!q.blk[b].holiday) continue;
    for (int64_t t = 0; t < count; ++t) {
      const int32_t k = holiday[b][(size_t)t];
      if (k >= 0) packed[(size_t)t] = (packed[(size_t)t] & ~(0xffull << (8 * b))) | ((uint64_t)k << (8 * b));
    }
  }
  return packed;
}

}  // namespace boom_amd
