// boom_amd.hpp -- header-only C++ host side over the C-ABI (boom_amd.h),
// mirroring the slice of BOOM's class surface that sits on the hot path so
// that callers (and our C++ parity test) read like code written against BOOM:
//
//   RegressionModel, GlmCoefs-style accessors   Models/Glm/RegressionModel.hpp:256-420
//   MvnGivenScalarSigma                         Models/MvnGivenScalarSigma.hpp:57-109
//   ChisqModel                                  Models/ChisqModel.hpp:28-39
//   VariableSelectionPrior                      Models/Glm/VariableSelectionPrior.hpp:99-135
//   BregVsSampler (5 ctors, setters, draw)      Models/Glm/PosteriorSamplers/BregVsSampler.hpp:64-161
//   StateSpaceRegressionModel                   Models/StateSpace/StateSpaceRegressionModel.hpp:82-113
//   LocalLevelStateModel                        Models/StateSpace/StateModels/LocalLevelStateModel.hpp
//   StateSpacePosteriorSampler                  Models/StateSpace/PosteriorSamplers/StateSpacePosteriorSampler.hpp:26-38
//   Model::sample_posterior / set_method        Models/ModelTypes.hpp:93-99, Policies/PriorPolicy.cpp:26-30
//   report_error -> std::runtime_error          cpputil/report_error.cpp:30-32
//
// Differences that are the point of the exercise: a sampler owns `chains`
// independent chains on one MI355X; draw() advances all of them; chain 0 backs
// the model's classic single-chain accessors; Ptr<T> is std::shared_ptr<T>.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "boom_amd.h"

namespace boom_amd_api {

template <class T>
using Ptr = std::shared_ptr<T>;
typedef std::vector<double> Vector;
typedef unsigned int uint;

inline void report_error(const std::string &msg) { throw std::runtime_error(msg); }
inline double infinity() { return std::numeric_limits<double>::infinity(); }

// column-major dense matrix, BOOM::Matrix layout (LinAlg/Matrix.hpp:429)
class Matrix {
 public:
  Matrix() : nr_(0), nc_(0) {}
  Matrix(int nr, int nc, double x = 0.0) : nr_(nr), nc_(nc), v_((size_t)nr * nc, x) {}
  int nrow() const { return nr_; }
  int ncol() const { return nc_; }
  double &operator()(int i, int j) { return v_[(size_t)j * nr_ + i]; }
  double operator()(int i, int j) const { return v_[(size_t)j * nr_ + i]; }
  double *data() { return v_.data(); }
  const double *data() const { return v_.data(); }
 private:
  int nr_, nc_;
  std::vector<double> v_;
};
typedef Matrix SpdMatrix;

// inclusion indicators (LinAlg/Selector.hpp)
class Selector {
 public:
  explicit Selector(int n = 0, bool all = false) : inc_(n, all ? 1 : 0) {}
  int nvars_possible() const { return (int)inc_.size(); }
  int nvars() const { int k = 0; for (auto b : inc_) k += b; return k; }
  bool operator[](int i) const { return inc_[i] != 0; }
  void add(int i) { inc_[i] = 1; }
  void drop(int i) { inc_[i] = 0; }
  void drop_all() { for (auto &b : inc_) b = 0; }
  std::vector<uint8_t> &bytes() { return inc_; }
  const std::vector<uint8_t> &bytes() const { return inc_; }
 private:
  std::vector<uint8_t> inc_;
};

// PosteriorSampler (Models/PosteriorSamplers/PosteriorSampler.hpp:49-66): the
// virtual surface of the path -- draw(), logpri(), the seed of the sampler's
// private stream(s)
class PosteriorSampler {
 public:
  virtual ~PosteriorSampler() {}
  virtual void draw() = 0;
  virtual double logpri() const = 0;
  virtual void set_seed(unsigned long seed) = 0;
};

class Model {
 public:
  virtual ~Model() {}
  void set_method(const Ptr<PosteriorSampler> &s) { samplers_.push_back(s); }
  void clear_methods() { samplers_.clear(); }
  int number_of_sampling_methods() const { return (int)samplers_.size(); }
  // PriorPolicy::sample_posterior
  void sample_posterior() { for (auto &s : samplers_) s->draw(); }
  Ptr<PosteriorSampler> sampler(int i) const { return samplers_[i]; }
 private:
  std::vector<Ptr<PosteriorSampler>> samplers_;
};

// ---- priors ---------------------------------------------------------------
struct MvnGivenScalarSigma {
  MvnGivenScalarSigma(const Vector &mean, const SpdMatrix &ominv) : mu_(mean), ominv_(ominv) {}
  const Vector &mu() const { return mu_; }
  const SpdMatrix &unscaled_precision() const { return ominv_; }
  int dim() const { return (int)mu_.size(); }
  Vector mu_;
  SpdMatrix ominv_;
};
struct ChisqModel {  // ChisqModel(df, sigma) == GammaModel(df/2, df sigma^2/2)
  explicit ChisqModel(double df = 1.0, double sigma_estimate = 1.0) : df_(df), sigma_(sigma_estimate) {}
  double df() const { return df_; }
  double sigma() const { return sigma_; }
  double alpha() const { return df_ / 2; }
  double beta() const { return df_ * sigma_ * sigma_ / 2; }
  double df_, sigma_;
};
struct VariableSelectionPrior {
  explicit VariableSelectionPrior(const Vector &pi) : pi_(pi), max_model_size_(-1) {}
  VariableSelectionPrior(uint n, double p) : pi_(n, p), max_model_size_(-1) {}
  void set_max_model_size(int64_t m) { max_model_size_ = m; }
  int64_t max_model_size() const { return max_model_size_; }
  const Vector &prior_inclusion_probabilities() const { return pi_; }
  uint potential_nvars() const { return (uint)pi_.size(); }
  Vector pi_;
  int64_t max_model_size_;
};

// BregVsSampler.hpp:33-40
struct ZellnerPriorParameters {
  Vector prior_inclusion_probabilities;
  Vector prior_beta_guess;
  double prior_beta_guess_weight;
  SpdMatrix prior_beta_information;  // Omega^{-1}
  double prior_sigma_guess;
  double prior_sigma_guess_weight;
};

// ---- engine handle shared by a model and its sampler ------------------------
class Engine {
 public:
  Engine(int chains, uint64_t seed, int device) {
    ba_config cfg{device, chains, 0, seed, 0, 0};
    if (ba_engine_create(&cfg, &e_) != BA_OK) report_error(ba_last_error());
    chains_ = chains;
  }
  // several devices of one node behind the handle (ba_group_*): engine i on devices[i]
  // owns the global chains [i * chains_per_device, (i + 1) * chains_per_device); get()
  // is the engine of chain 0.  Only RegressionModel / BregVsSampler take a device list.
  Engine(int chains_per_device, uint64_t seed, const std::vector<int> &devices) {
    std::vector<int32_t> dev(devices.begin(), devices.end());
    if (ba_group_create(dev.data(), (int32_t)dev.size(), chains_per_device, seed, &g_) != BA_OK)
      report_error(ba_group_last_error());
    e_ = ba_group_engine(g_, 0);
    chains_ = chains_per_device * (int)dev.size();
  }
  ~Engine() { if (g_) ba_group_destroy(g_); else ba_engine_destroy(e_); }
  Engine(const Engine &) = delete;
  ba_engine *get() const { return e_; }
  ba_group *group() const { return g_; }
  int size() const { return g_ ? ba_group_size(g_) : 1; }
  ba_engine *get(int i) const { return g_ ? ba_group_engine(g_, i) : e_; }
  int chains() const { return chains_; }
  void check(int rc) const { if (rc != BA_OK) report_error(ba_last_error()); }
  void check_group(int rc) const { if (rc != BA_OK) report_error(ba_group_last_error()); }
  // f(engine) on every engine of the handle
  template <class F> void each(F f) const { for (int i = 0; i < size(); ++i) check(f(get(i))); }
 private:
  ba_engine *e_ = nullptr;
  ba_group *g_ = nullptr;
  int chains_ = 0;
};

// ---- RegressionModel ----------------------------------------------------------
class RegressionModel : public Model {
 public:
  // RegressionModel(X, y, start_at_mle = false): sufficient statistics are
  // built on the device (NeRegSuf(X, y))
  RegressionModel(const Matrix &X, const Vector &y, int chains = 1,
                  uint64_t seed = 8675309, int device = 0)
      : eng_(new Engine(chains, seed, device)), p_(X.ncol()), inc_(X.ncol(), true),
        beta_(X.ncol(), 0.0), sigsq_(1.0) {
    if (X.nrow() != (int)y.size()) report_error("Number of rows of X must match the length of y.");
    eng_->check(ba_build_suf_from_xy(eng_->get(), X.nrow(), X.ncol(), X.data(), y.data()));
  }
  // the same over a device list: rows of X are sharded over the devices, one f64-MFMA
  // syrk per device and ONE all-reduce give every engine the identical NeRegSuf
  // (ba_group_build_suf_from_xy); `chains_per_device` chains on each entry of `devices`
  RegressionModel(const Matrix &X, const Vector &y, int chains_per_device,
                  const std::vector<int> &devices, uint64_t seed = 8675309)
      : eng_(new Engine(chains_per_device, seed, devices)), p_(X.ncol()), inc_(X.ncol(), true),
        beta_(X.ncol(), 0.0), sigsq_(1.0) {
    if (X.nrow() != (int)y.size()) report_error("Number of rows of X must match the length of y.");
    eng_->check_group(ba_group_build_suf_from_xy(eng_->group(), X.nrow(), X.ncol(), X.data(), y.data()));
  }
  int xdim() const { return p_; }
  int nvars_possible() const { return p_; }
  // (a change made through the mutators below goes to every chain before the
  // sampler's next draw, as BOOM's sampler reads the model's current state on
  // every draw)
  const Selector &inc() const { return inc_; }               // coef().inc()
  void set_inc(const Selector &g) { inc_ = g; dirty_ = true; }  // coef().set_inc(g)
  void drop_all() { inc_.drop_all(); dirty_ = true; }        // coef().drop_all()
  void add(int i) { inc_.add(i); dirty_ = true; }            // coef().add(i)
  void drop(int i) { inc_.drop(i); dirty_ = true; }          // coef().drop(i)
  const Vector &Beta() const { return beta_; }
  void set_Beta(const Vector &b) { beta_ = b; dirty_ = true; }
  double sigsq() const { return sigsq_; }
  void set_sigsq(double s) { sigsq_ = s; dirty_ = true; }
  bool dirty() const { return dirty_; }
  const Ptr<Engine> &engine() const { return eng_; }
  // all chains (chains x p row-major gamma / beta, chains sigsq)
  void chain_states(std::vector<uint8_t> &gamma, Vector &beta, Vector &sigsq) const {
    const size_t C = eng_->chains(), per = C / eng_->size();
    gamma.resize(C * p_); beta.resize(C * p_); sigsq.resize(C);
    for (int i = 0; i < eng_->size(); ++i)   // global chain order
      eng_->check(ba_get_states(eng_->get(i), gamma.data() + i * per * p_, beta.data() + i * per * p_,
                                sigsq.data() + i * per));
  }
  // used by the sampler
  void push_state() {
    eng_->each([&](ba_engine *e) { return ba_set_state(e, -1, inc_.bytes().data(), beta_.data(), sigsq_); });
    dirty_ = false;
  }
  // (while ba_draw_next serves a look-ahead batch, ba_get_state is the draw being served)
  void pull_chain0() {
    eng_->check(ba_get_state(eng_->get(), 0, inc_.bytes().data(), beta_.data(), &sigsq_));
    dirty_ = false;
  }
 private:
  Ptr<Engine> eng_;
  int p_;
  Selector inc_;
  Vector beta_;
  double sigsq_;
  bool dirty_ = true;
};

// ---- BregVsSampler ---------------------------------------------------------------
class BregVsSampler : public PosteriorSampler {
 public:
  // ctor #1 (BregVsSampler.cpp:48-85)
  BregVsSampler(RegressionModel *model, double prior_nobs, double expected_rsq,
                double expected_model_size, bool first_term_is_intercept = true)
      : model_(model) {
    all([&](ba_engine *e) { return ba_set_priors_ctor1(e, prior_nobs, expected_rsq, expected_model_size,
                                                        first_term_is_intercept); });
    all([&](ba_engine *e) { return ba_set_lookahead(e, kDefaultLookahead); });
  }
  // ctor #2 (BregVsSampler.cpp:87-142)
  BregVsSampler(RegressionModel *model, double prior_sigma_nobs, double prior_sigma_guess,
                double prior_beta_nobs, double diagonal_shrinkage,
                double prior_inclusion_probability, bool force_intercept = true)
      : model_(model) {
    all([&](ba_engine *e) { return ba_set_priors_ctor2(e, prior_sigma_nobs, prior_sigma_guess, prior_beta_nobs,
                                                        diagonal_shrinkage, prior_inclusion_probability,
                                                        force_intercept); });
    all([&](ba_engine *e) { return ba_set_lookahead(e, kDefaultLookahead); });
  }
  // ctor #3 (BregVsSampler.cpp:144-160)
  BregVsSampler(RegressionModel *model, const Vector &prior_mean,
                const SpdMatrix &unscaled_prior_precision, double sigma_guess, double df,
                const Vector &prior_inclusion_probs)
      : model_(model) {
    set_raw(prior_mean, unscaled_prior_precision, df, sigma_guess, prior_inclusion_probs, -1);
  }
  // ctor #4 (BregVsSampler.cpp:162-178)
  BregVsSampler(RegressionModel *model, const ZellnerPriorParameters &prior)
      : model_(model) {
    if ((int)prior.prior_beta_guess.size() != model->xdim()) report_error("Slab dimension did not match model dimension.");
    if ((int)prior.prior_inclusion_probabilities.size() != model->xdim()) report_error("Spike dimension did not match model dimension.");
    set_raw(prior.prior_beta_guess, prior.prior_beta_information, prior.prior_sigma_guess_weight,
            prior.prior_sigma_guess, prior.prior_inclusion_probabilities, -1);
  }
  // ctor #5 (BregVsSampler.cpp:180-194)
  BregVsSampler(RegressionModel *model, const Ptr<MvnGivenScalarSigma> &slab,
                const Ptr<ChisqModel> &residual_precision_prior,
                const Ptr<VariableSelectionPrior> &spike)
      : model_(model) {
    if (slab->dim() != model->xdim()) report_error("Slab dimension did not match model dimension.");
    if ((int)spike->potential_nvars() != model->xdim()) report_error("Spike dimension did not match model dimension.");
    set_raw(slab->mu(), slab->unscaled_precision(), residual_precision_prior->df(),
            residual_precision_prior->sigma(), spike->prior_inclusion_probabilities(),
            spike->max_model_size());
  }

  void draw() override {                     // BregVsSampler.cpp:252-261
    // the model's parameters as the caller left them (a host-side change since
    // the last draw goes to every chain first; the engine then rewinds any
    // look-ahead draws not handed out yet)
    if (model_->dirty()) model_->push_state();
    all([](ba_engine *e) { return ba_draw_next(e); });   // one launch per `lookahead` calls and device
    model_->pull_chain0();
  }
  // run `n` sweeps ahead per launch and hand them out one draw() at a time, for
  // EVERY chain (ba_set_lookahead: the draws are the ones one launch per call
  // would give, whatever is called in between)
  void set_lookahead(int n) { all([&](ba_engine *e) { return ba_set_lookahead(e, n < 1 ? 1 : n); }); }
  void draw(int nsweeps) {                   // many sweeps in one launch (per device, side by side)
    if (model_->dirty()) model_->push_state();
    all([&](ba_engine *e) { return ba_sweep(e, nsweeps); });
    model_->pull_chain0();
  }
  void limit_model_selection(uint n) { max_flips_ = (int)n; options(); }
  void suppress_model_selection() { max_flips_ = 0; options(); }
  void allow_model_selection(bool allow = true) { max_flips_ = allow ? -1 : 0; options(); }
  void suppress_beta_draw() { draw_beta_ = 0; options(); }
  void suppress_sigma_draw() { draw_sigma_ = 0; options(); }
  void set_correlation_swap_threshold(double t) { swap_ = t; options(); }
  void set_sigma_upper_limit(double s) {
    double df, ss;
    check(ba_get_priors(h(), nullptr, nullptr, nullptr, &df, &ss));
    all([&](ba_engine *e) { return ba_set_sigma_prior(e, df, std::sqrt(ss / df), s); });
  }
  void set_seed(unsigned long s) override { all([&](ba_engine *e) { return ba_seed(e, s); }); }
  double logpri() const override {           // BregVsSampler.cpp:380-393, chain 0 (the draw being served)
    double out;
    check(ba_logpri(h(), 0, &out));
    return out;
  }
  double prior_df() const { double df; check(ba_get_priors(h(), nullptr, nullptr, nullptr, &df, nullptr)); return df; }
  double prior_ss() const { double ss; check(ba_get_priors(h(), nullptr, nullptr, nullptr, nullptr, &ss)); return ss; }
  double log_model_prob(const Selector &g) const {
    double out;
    check(ba_log_model_prob(h(), 1, g.bytes().data(), &out));
    return out;
  }
 private:
  ba_engine *h() const { return model_->engine()->get(); }
  void check(int rc) const { model_->engine()->check(rc); }
  template <class F> void all(F f) const { model_->engine()->each(f); }
  void options() { all([&](ba_engine *e) { return ba_set_options(e, max_flips_, swap_, draw_beta_, draw_sigma_); }); }
  void set_raw(const Vector &b, const SpdMatrix &om, double df, double guess, const Vector &pi, int64_t mms) {
    all([&](ba_engine *e) { return ba_set_slab(e, b.data(), om.data()); });
    all([&](ba_engine *e) { return ba_set_spike(e, pi.data(), mms); });
    all([&](ba_engine *e) { return ba_set_sigma_prior(e, df, guess, infinity()); });
    // the caller's `for i: sample_posterior()` loop runs at the long-launch rate
    // by default; the draws do not depend on this number
    all([&](ba_engine *e) { return ba_set_lookahead(e, kDefaultLookahead); });
  }
  static constexpr int kDefaultLookahead = 256;
  RegressionModel *model_;
  int max_flips_ = -1, draw_beta_ = 1, draw_sigma_ = 1;
  double swap_ = 0.8;
};

// ---- bsts: local level + regression ----------------------------------------------
class LocalLevelStateModel {
 public:
  explicit LocalLevelStateModel(double sigma = 1.0) : sigma_(sigma) {}
  void set_initial_state_mean(double m) { a0_ = m; }
  void set_initial_state_variance(double v) { P0_ = v; }
  // ZeroMeanGaussianConjSampler(model, df, sigma_guess) + set_sigma_upper_limit
  void set_prior(double df, double sigma_guess, double sigma_upper_limit = infinity()) {
    df_ = df; guess_ = sigma_guess; upper_ = sigma_upper_limit;
  }
  double sigma_, a0_ = 0.0, P0_ = 1.0, df_ = 1.0, guess_ = 1.0, upper_ = infinity();
};

// LocalLinearTrendStateModel with one ZeroMeanMvnIndependenceSampler per variance
// (StateModels/LocalLinearTrend.cpp; the way bsts' AddLocalLinearTrend builds it)
class LocalLinearTrendStateModel {
 public:
  LocalLinearTrendStateModel() {}
  void set_initial_state_mean(const Vector &m) { a0_ = m; }
  void set_initial_state_variance(const Vector &diagonal) { P0_ = diagonal; }
  void set_initial_sigma(double level_sigma, double slope_sigma) { sigma_[0] = level_sigma; sigma_[1] = slope_sigma; }
  // ZeroMeanMvnIndependenceSampler(model, df, sigma_guess, which_variable) + set_sigma_upper_limit
  void set_prior(int which_variable, double df, double sigma_guess, double sigma_upper_limit = infinity()) {
    df_[which_variable] = df; guess_[which_variable] = sigma_guess; upper_[which_variable] = sigma_upper_limit;
  }
  Vector a0_ = Vector(2, 0.0), P0_ = Vector(2, 1.0);
  double sigma_[2] = {1.0, 1.0}, df_[2] = {1.0, 1.0}, guess_[2] = {1.0, 1.0}, upper_[2] = {infinity(), infinity()};
};
// StudentLocalLinearTrendStateModel with its StudentLocalLinearTrendPosteriorSampler
// (StateModels/StudentLocalLinearTrend.cpp; bsts' AddStudentLocalLinearTrend): a local linear trend
// whose level and slope errors are Student-t -- per-step weights, two degrees-of-freedom parameters.
// which = 0: level, 1: slope
class StudentLocalLinearTrendStateModel {
 public:
  explicit StudentLocalLinearTrendStateModel(double sigma_level = 1.0, double nu_level = 1000.0, double sigma_slope = 1.0,
                                             double nu_slope = 1000.0) {
    sigma_[0] = sigma_level; sigma_[1] = sigma_slope; nu_[0] = nu_level; nu_[1] = nu_slope;
  }
  void set_initial_state_mean(const Vector &m) { a0_ = m; }
  void set_initial_state_variance(const Vector &diagonal) { P0_ = diagonal; }
  void set_initial_sigma(double level_sigma, double slope_sigma) { sigma_[0] = level_sigma; sigma_[1] = slope_sigma; }
  void set_initial_nu(double level_nu, double slope_nu) { nu_[0] = level_nu; nu_[1] = slope_nu; }
  // ChisqModel(df, sigma_guess) on sigma^2 + set_sigma_{level, slope}_upper_limit
  void set_prior(int which, double df, double sigma_guess, double sigma_upper_limit = infinity()) {
    df_[which] = df; guess_[which] = sigma_guess; upper_[which] = sigma_upper_limit;
  }
  // the prior on nu: kind 0 = UniformModel(a, b) (bsts: (1, 500)), 1 = GammaModel(a, b)
  void set_nu_prior(int which, int kind, double a, double b) { nu_kind_[which] = kind; nu_a_[which] = a; nu_b_[which] = b; }
  Vector a0_ = Vector(2, 0.0), P0_ = Vector(2, 1.0);
  double sigma_[2], nu_[2], df_[2] = {1.0, 1.0}, guess_[2] = {1.0, 1.0}, upper_[2] = {infinity(), infinity()};
  int nu_kind_[2] = {0, 0};
  double nu_a_[2] = {1.0, 1.0}, nu_b_[2] = {500.0, 500.0};
};
// SeasonalStateModel(nseasons, season_duration) with a ZeroMeanGaussianConjSampler: the
// transition is the seasonal matrix on the steps INTO a new season and the identity
// inside one (StateModels/SeasonalStateModel.cpp:89-104, :248-258)
class SeasonalStateModel {
 public:
  explicit SeasonalStateModel(int nseasons, int season_duration = 1)
      : nseasons_(nseasons), duration_(season_duration) {
    if (nseasons <= 0) report_error("'nseasons' must be positive in constructor for SeasonalStateModelBase");
    if (season_duration < 1) report_error("season_duration must be positive");
    a0_ = Vector(nseasons - 1, 0.0);
    P0_ = Vector(nseasons - 1, 1.0);
  }
  int state_dimension() const { return nseasons_ - 1; }
  int nseasons() const { return nseasons_; }
  int season_duration() const { return duration_; }
  void set_time_of_first_observation(int t0) { t0_ = t0; }
  void set_sigsq(double s) { sigma_ = std::sqrt(s); }
  void set_initial_state_mean(const Vector &m) { a0_ = m; }
  void set_initial_state_variance(double v) { P0_ = Vector(nseasons_ - 1, v); }
  void set_prior(double df, double sigma_guess, double sigma_upper_limit = infinity()) {
    df_ = df; guess_ = sigma_guess; upper_ = sigma_upper_limit;
  }
  int nseasons_, duration_, t0_ = 0;
  Vector a0_, P0_;
  double sigma_ = 1.0, df_ = 1.0, guess_ = 1.0, upper_ = infinity();
};

// MonthlyAnnualCycle with a ZeroMeanGaussianConjSampler (StateModels/SeasonalStateModel.hpp; bsts
// AddMonthlyAnnualCycle): state model kind 11 with 12 seasons, a month-of-year effect for daily data.
// A new season starts where the day is the first of a month.  There is no Date class here: the
// constructor takes the date of the first observation as (year, month, day), and
// ba_monthly_cycle_calendar turns it into the block's calendar when the list goes to the device -- the
// series' length and forecast_horizon() entries beyond it (set_forecast_horizon: as many steps as a
// forecast will ask for; a year by default).
class MonthlyAnnualCycle {
 public:
  MonthlyAnnualCycle(int year, int month, int day) : year_(year), month_(month), day_(day) {
    uint8_t probe = 0;
    if (ba_monthly_cycle_calendar(year, month, day, 1, &probe) != BA_OK) report_error(ba_last_error());
    a0_ = Vector(11, 0.0);
    P0_ = Vector(11, 1.0);
  }
  int state_dimension() const { return 11; }
  int nseasons() const { return 12; }
  int forecast_horizon() const { return horizon_; }
  void set_forecast_horizon(int steps) {
    if (steps < 0) report_error("the forecast horizon must not be negative");
    horizon_ = steps;
  }
  // the calendar of a series of `length` time points (and the horizon beyond it)
  std::vector<uint8_t> calendar(int length) const {
    std::vector<uint8_t> flags((size_t)length + (size_t)horizon_, 0);
    if (!flags.empty() && ba_monthly_cycle_calendar(year_, month_, day_, (int64_t)flags.size(), flags.data()) != BA_OK)
      report_error(ba_last_error());
    return flags;
  }
  void set_sigsq(double s) { sigma_ = std::sqrt(s); }
  void set_initial_state_mean(const Vector &m) { a0_ = m; }
  void set_initial_state_variance(double v) { P0_ = Vector(11, v); }
  void set_prior(double df, double sigma_guess, double sigma_upper_limit = infinity()) {
    df_ = df; guess_ = sigma_guess; upper_ = sigma_upper_limit;
  }
  int year_, month_, day_, horizon_ = 366;
  Vector a0_, P0_;
  double sigma_ = 1.0, df_ = 1.0, guess_ = 1.0, upper_ = infinity();
};

// RandomWalkHolidayStateModel with a ZeroMeanGaussianConjSampler (StateModels/
// RandomWalkHolidayStateModel.cpp; bsts AddRandomWalkHoliday): state model kind 10.  There is no
// Date / Holiday layer here: where the reference's constructor takes (holiday, time_zero), this one
// takes the calendar those two would reveal -- positions[t] = -1 where time t is outside the holiday's
// window, else days_into_influence_window of time t -- and the maximum window width.  Entries past
// the series' length serve forecasts.
class RandomWalkHolidayStateModel {
 public:
  RandomWalkHolidayStateModel(const std::vector<int32_t> &positions, int width) : positions_(positions), width_(width) {
    if (width < 1) report_error("the holiday's maximum window width must be positive");
    for (int32_t k : positions)
      if (k < -1 || k >= width) report_error("a calendar entry must be -1 (inactive) or a position in [0, width)");
    a0_ = Vector(width, 0.0);
    P0_ = Vector(width, 1.0);
  }
  int state_dimension() const { return width_; }
  const std::vector<int32_t> &positions() const { return positions_; }
  void set_sigsq(double s) { sigma_ = std::sqrt(s); }
  void set_initial_state_mean(const Vector &m) { a0_ = m; }
  void set_initial_state_variance(const Vector &diagonal) { P0_ = diagonal; }
  void set_prior(double df, double sigma_guess, double sigma_upper_limit = infinity()) {
    df_ = df; guess_ = sigma_guess; upper_ = sigma_upper_limit;
  }
  std::vector<int32_t> positions_;
  int width_;
  Vector a0_, P0_;
  double sigma_ = 1.0, df_ = 1.0, guess_ = 1.0, upper_ = infinity();
};

// DynamicRegressionStateModel(X) with a DynamicRegressionIndependentPosteriorSampler (StateModels/
// DynamicRegressionStateModel.cpp; bsts AddDynamicRegression with DynamicRegressionRandomWalkOptions):
// ba_ss_add_dynamic_regression.  predictors: one row per time point, row t = x_t; rows past the series'
// length serve forecasts (the reference's add_forecast_data).  One variance, prior and sigma upper limit
// per coefficient.
class DynamicRegressionStateModel {
 public:
  explicit DynamicRegressionStateModel(const Matrix &predictors) : xdim_(predictors.ncol()), rows_(predictors.nrow()) {
    if (xdim_ < 1 || rows_ < 1) report_error("a dynamic regression needs at least one row and one column of predictors");
    x_.resize((size_t)rows_ * xdim_);   // (row-major, as the C-ABI takes them)
    for (int t = 0; t < rows_; ++t)
      for (int i = 0; i < xdim_; ++i) x_[(size_t)t * xdim_ + i] = predictors(t, i);
    a0_ = Vector(xdim_, 0.0);
    P0_ = Vector(xdim_, 1.0);
    sigma_ = Vector(xdim_, 1.0);
    df_ = Vector(xdim_, 1.0);
    guess_ = Vector(xdim_, 1.0);
    upper_ = Vector(xdim_, infinity());
  }
  int state_dimension() const { return xdim_; }
  int xdim() const { return xdim_; }
  int rows() const { return rows_; }
  const Vector &predictors() const { return x_; }   // rows x xdim, row-major
  void set_sigsq(const Vector &s) { check_size(s); for (int i = 0; i < xdim_; ++i) sigma_[i] = std::sqrt(s[i]); }
  void set_initial_state_mean(const Vector &m) { check_size(m); a0_ = m; }
  void set_initial_state_variance(const Vector &diagonal) { check_size(diagonal); P0_ = diagonal; }
  // coefficient i's ChisqModel(df, sigma_guess) and sigma upper limit
  void set_prior(int i, double df, double sigma_guess, double sigma_upper_limit = infinity()) {
    if (i < 0 || i >= xdim_) report_error("coefficient index out of range");
    df_[i] = df; guess_[i] = sigma_guess; upper_[i] = sigma_upper_limit;
  }
  void check_size(const Vector &v) const {
    if ((int)v.size() != xdim_) report_error("a dynamic regression takes one entry per predictor");
  }
  int xdim_, rows_;
  Vector x_, a0_, P0_, sigma_, df_, guess_, upper_;
};

// DynamicRegressionArStateModel(X, lags) with a DynamicRegressionArPosteriorSampler (StateModels/
// DynamicRegressionArStateModel.cpp; bsts AddDynamicRegression with DynamicRegressionArOptions(lags)):
// ba_ss_add_dynamic_regression_ar.  Every coefficient follows an autoregression of `lags` lags with its own
// ArModel (phi, sigma) and ArPosteriorSampler.  The state holds, coefficient by coefficient, the coefficient
// and its lags: state_dimension() = xdim x lags.  On the device the model is xdim state models of the list,
// one per coefficient (at most 4 less the list's other autoregressions and semilocal trends).  The arrays
// that run over the state -- initial mean and variance, the coefficients phi -- are xdim x lags, row-major.
class DynamicRegressionArStateModel {
 public:
  DynamicRegressionArStateModel(const Matrix &predictors, int lags) : xdim_(predictors.ncol()), rows_(predictors.nrow()), lags_(lags) {
    if (xdim_ < 1 || rows_ < 1) report_error("a dynamic regression needs at least one row and one column of predictors");
    if (lags_ < 1) report_error("lags must be positive");
    x_.resize((size_t)rows_ * xdim_);   // (row-major, as the C-ABI takes them)
    for (int t = 0; t < rows_; ++t)
      for (int i = 0; i < xdim_; ++i) x_[(size_t)t * xdim_ + i] = predictors(t, i);
    a0_ = Vector(xdim_ * lags_, 0.0);   // (bsts: mean 0, variance 1)
    P0_ = Vector(xdim_ * lags_, 1.0);
    phi_ = Vector(xdim_ * lags_, 0.0);
    sigma_ = Vector(xdim_, 1.0);
    df_ = Vector(xdim_, 1.0);
    guess_ = Vector(xdim_, 1.0);
    upper_ = Vector(xdim_, infinity());
  }
  int state_dimension() const { return xdim_ * lags_; }
  int xdim() const { return xdim_; }
  int lags() const { return lags_; }
  int rows() const { return rows_; }
  const Vector &predictors() const { return x_; }   // rows x xdim, row-major
  void set_sigsq(const Vector &s) { check_size(s, xdim_); for (int i = 0; i < xdim_; ++i) sigma_[i] = std::sqrt(s[i]); }
  void set_phi(const Vector &phi) { check_size(phi, xdim_ * lags_); phi_ = phi; }
  void set_initial_state_mean(const Vector &m) { check_size(m, xdim_ * lags_); a0_ = m; }
  void set_initial_state_variance(const Vector &diagonal) { check_size(diagonal, xdim_ * lags_); P0_ = diagonal; }
  // coefficient i's ChisqModel(df, sigma_guess) and sigma upper limit
  void set_prior(int i, double df, double sigma_guess, double sigma_upper_limit = infinity()) {
    if (i < 0 || i >= xdim_) report_error("coefficient index out of range");
    df_[i] = df; guess_[i] = sigma_guess; upper_[i] = sigma_upper_limit;
  }
  void check_size(const Vector &v, int n) const {
    if ((int)v.size() != n) report_error("an AR dynamic regression takes one entry per predictor, or per predictor and lag");
  }
  int xdim_, rows_, lags_;
  Vector x_, a0_, P0_, phi_, sigma_, df_, guess_, upper_;
};

// RegressionHolidayStateModel with its own sample_posterior (StateModels/RegressionHolidayStateModel.cpp;
// bsts AddRegressionHoliday): ba_ss_add_regression_holiday.  One coefficient per day of each holiday's
// window, shared across the years, all under the prior N(prior_mean, prior_sd^2).  There is no Date /
// Holiday layer here: where the reference's add_holiday takes a Holiday, this one takes the holidays'
// window widths, and set_calendar the calendar they would reveal -- index[t] = -1 where no holiday of the
// model is active at time t, else offset_h + days_into_influence_window (offset_h: the widths of the
// holidays before h).  Entries past the series' length serve forecasts.  On the device the model is an
// offset on the series, not a block of the state: state_dimension() of the model that holds it, its state
// draw and state_variances() do not count it.
class RegressionHolidayStateModel {
 public:
  RegressionHolidayStateModel(const std::vector<int32_t> &widths, double prior_mean, double prior_sd)
      : widths_(widths), prior_mean_(prior_mean), prior_sd_(prior_sd) {
    if (widths.empty()) report_error("a regression holiday model needs at least one holiday");
    for (int32_t w : widths) {
      if (w < 1) report_error("a holiday's width must be at least 1");
      ncoef_ += w;
    }
    if (!(prior_sd > 0.0)) report_error("the prior standard deviation must be positive");
    coef_ = Vector(ncoef_, 0.0);
  }
  int number_of_coefficients() const { return ncoef_; }
  const std::vector<int32_t> &widths() const { return widths_; }
  const std::vector<int32_t> &calendar() const { return calendar_; }
  void set_calendar(const std::vector<int32_t> &index) {
    for (int32_t k : index)
      if (k < -1 || k >= ncoef_) report_error("a calendar entry must be -1 (inactive) or a coefficient index in [0, sum of the widths)");
    calendar_ = index;
  }
  // the initial coefficients (default: zeros)
  void set_coefficients(const Vector &c) {
    if ((int)c.size() != ncoef_) report_error("a regression holiday model takes one coefficient per day of every holiday's window");
    coef_ = c;
  }
  std::vector<int32_t> widths_, calendar_;
  double prior_mean_, prior_sd_;
  int ncoef_ = 0;
  Vector coef_;
};

// HierarchicalRegressionHolidayStateModel with HierGaussianRegressionAsisSampler
// (StateModels/HierarchicalRegressionHolidayStateModel.cpp; bsts AddHierarchicalRegressionHoliday):
// ba_ss_add_hierarchical_regression_holiday.  nholidays holidays of one window width; holiday h's coefficient
// vector is N(mu, Omega^-1) with mu ~ N(mean_prior_mean, mean_prior_variance) and Omega ~ Wishart(
// variance_guess_weight, variance_guess_weight x variance_guess), both drawn with the coefficients.  As the
// plain model it takes window widths and a calendar in place of Holiday objects (index[t] = h x width + day),
// and is an offset on the series, not a block of the state.  holiday_mean / holiday_precision read one chain's
// mu and Omega once the model that holds it has been given its sampler.
class HierarchicalRegressionHolidayStateModel {
 public:
  HierarchicalRegressionHolidayStateModel(int nholidays, int width, const Vector &mean_prior_mean, const SpdMatrix &mean_prior_variance,
                                          const SpdMatrix &variance_guess, double variance_guess_weight)
      : nholidays_(nholidays), width_(width), mean_prior_mean_(mean_prior_mean), mean_prior_variance_(mean_prior_variance),
        variance_guess_(variance_guess), weight_(variance_guess_weight) {
    if (nholidays < 1) report_error("a regression holiday model needs at least one holiday");
    if (width < 1) report_error("a holiday's width must be at least 1");
    if ((int)mean_prior_mean.size() != width || mean_prior_variance.nrow() != width || mean_prior_variance.ncol() != width ||
        variance_guess.nrow() != width || variance_guess.ncol() != width)
      report_error("the prior mean takes width entries, the prior variance and the variance guess width x width");
    coef_ = Vector((size_t)nholidays * width, 0.0);
  }
  int number_of_coefficients() const { return nholidays_ * width_; }
  int number_of_holidays() const { return nholidays_; }
  int width() const { return width_; }
  const std::vector<int32_t> &calendar() const { return calendar_; }
  void set_calendar(const std::vector<int32_t> &index) {
    for (int32_t k : index)
      if (k < -1 || k >= number_of_coefficients()) report_error("a calendar entry must be -1 (inactive) or a coefficient index in [0, nholidays x width)");
    calendar_ = index;
  }
  // the initial coefficients (default: zeros)
  void set_coefficients(const Vector &c) {
    if ((int)c.size() != number_of_coefficients()) report_error("a regression holiday model takes one coefficient per day of every holiday's window");
    coef_ = c;
  }
  Vector holiday_mean(int chain = 0) const {
    Vector v((size_t)width_);
    bound()->check(ba_ss_get_hierarchical_regression_holiday(engine_->get(), chain, index_, v.data(), nullptr));
    return v;
  }
  SpdMatrix holiday_precision(int chain = 0) const {
    SpdMatrix m(width_, width_);   // (symmetric: the row-major entries are the column-major ones)
    bound()->check(ba_ss_get_hierarchical_regression_holiday(engine_->get(), chain, index_, nullptr, m.data()));
    return m;
  }
  int nholidays_, width_;
  Vector mean_prior_mean_;
  SpdMatrix mean_prior_variance_, variance_guess_;
  double weight_;
  std::vector<int32_t> calendar_;
  Vector coef_;
  // set when the model that holds it hands its list to the engine
  Ptr<Engine> engine_;
  int32_t index_ = -1;

 private:
  const Ptr<Engine> &bound() const {
    if (!engine_ || index_ < 0) report_error("the model is on no state space model with a sampler yet");
    return engine_;
  }
};

// ArStateModel(number_of_lags) with an ArPosteriorSampler (StateModels/ArStateModel.hpp:53,
// TimeSeries/PosteriorSamplers/ArPosteriorSampler.hpp)
class ArStateModel {
 public:
  explicit ArStateModel(int number_of_lags) : lags_(number_of_lags) {
    if (number_of_lags < 1) report_error("the number of lags must be positive in the constructor for ArStateModel");
    phi_ = Vector(number_of_lags, 0.0);
    a0_ = Vector(number_of_lags, 0.0);
    P0_ = Vector(number_of_lags, 1.0);
  }
  int state_dimension() const { return lags_; }
  int number_of_lags() const { return lags_; }
  void set_phi(const Vector &phi) { phi_ = phi; }
  void set_sigma(double s) { sigma_ = s; }
  void set_sigsq(double s) { sigma_ = std::sqrt(s); }
  void set_initial_state_mean(const Vector &m) { a0_ = m; }
  void set_initial_state_variance(double v) { P0_ = Vector(lags_, v); }
  // ArPosteriorSampler(model, ChisqModel(df, sigma_guess)) [+ set_sigma_upper_limit]
  void set_prior(double df, double sigma_guess, double sigma_upper_limit = infinity()) {
    df_ = df; guess_ = sigma_guess; upper_ = sigma_upper_limit;
  }
  // bsts AddAutoAr: an ArSpikeSlabSampler(model, MvnModel(mu, siginv) slab, VariableSelectionPrior(pi)
  // spike, ChisqModel(df, sigma_guess), truncate) [+ set_sigma_upper_limit, limit_model_selection(max_flips)]
  // in place of the ArPosteriorSampler: state model kind 9, every lag included at the start
  void set_spike_slab_prior(const Vector &mu, const SpdMatrix &siginv, const Vector &pi, double df, double sigma_guess,
                            double sigma_upper_limit = infinity(), bool truncate = true, int max_flips = -1) {
    if ((int)mu.size() != lags_ || siginv.nrow() != lags_ || (int)pi.size() != lags_)
      report_error("The spike and slab prior does not match the number of lags in ArStateModel.");
    df_ = df; guess_ = sigma_guess; upper_ = sigma_upper_limit;
    slab_mu_ = mu; slab_siginv_ = siginv; spike_pi_ = pi;
    truncate_ = truncate; max_flips_ = max_flips;
    spike_slab_ = true;
  }
  bool spike_slab() const { return spike_slab_; }
  int lags_;
  Vector phi_, a0_, P0_;
  double sigma_ = 1.0, df_ = 1.0, guess_ = 1.0, upper_ = infinity();
  bool spike_slab_ = false, truncate_ = true;
  int max_flips_ = -1;
  Vector slab_mu_, spike_pi_;
  SpdMatrix slab_siginv_;
};

// StaticInterceptStateModel (StateModels/StaticInterceptStateModel.hpp:35-131): one component,
// T = 1, no state error, nothing to learn; set_initial_state_mean / _variance are its prior
class StaticInterceptStateModel {
 public:
  StaticInterceptStateModel() {}
  int state_dimension() const { return 1; }
  void set_initial_state_mean(double m) { a0_ = m; }
  void set_initial_state_variance(double v) {
    if (v < 0) report_error("Initial state variance must be non-negative.");
    P0_ = v;
  }
  double a0_ = 0.0, P0_ = 1.0;
};

// TrigStateModel(period, frequencies) (StateModels/TrigStateModel.hpp:83, .cpp:130-223): a
// cosine / sine pair per frequency that rotates by 2 pi f / period a step, one error variance
// for all components with a ZeroMeanGaussianConjSampler (set_prior), as bsts builds it
class TrigStateModel {
 public:
  TrigStateModel(double period, const Vector &frequencies) : period_(period), frequencies_(frequencies) {
    if (frequencies.size() == 0) report_error("At least one frequency needed to initialize TrigStateModel.");
    const int n = 2 * (int)frequencies.size();
    a0_ = Vector(n, 0.0);
    P0_ = Vector(n, 1.0);
    rotations_ = Vector(n, 0.0);
    for (int i = 0; i < (int)frequencies.size(); ++i) {
      const double freq = 2 * 3.141592653589793 * frequencies[i] / period;   // (Constants::pi)
      rotations_[2 * i] = std::cos(freq);
      rotations_[2 * i + 1] = std::sin(freq);
    }
  }
  int state_dimension() const { return (int)a0_.size(); }
  void set_sigsq(double s) { sigma_ = std::sqrt(s); }
  void set_initial_state_mean(const Vector &m) {
    if ((int)m.size() != state_dimension()) report_error("Argument to TrigStateModel::set_initial_state_mean is of the wrong size.");
    a0_ = m;
  }
  void set_initial_state_variance(const Vector &diagonal) {
    if ((int)diagonal.size() != state_dimension()) report_error("Argument to TrigStateModel::set_initial_state_variance has the wrong number of rows.");
    P0_ = diagonal;
  }
  // ZeroMeanGaussianConjSampler(error_distribution(), ChisqModel(df, sigma_guess)) + set_sigma_upper_limit
  void set_prior(double df, double sigma_guess, double sigma_upper_limit = infinity()) {
    df_ = df; guess_ = sigma_guess; upper_ = sigma_upper_limit;
  }
  double period_;
  Vector frequencies_, rotations_, a0_, P0_;
  double sigma_ = 1.0, df_ = 1.0, guess_ = 1.0, upper_ = infinity();
};

// SemilocalLinearTrendStateModel(level, slope) (StateModels/SemilocalLinearTrend.hpp:75): a level
// that moves by a slope which is itself a stationary AR(1) around a long-run mean -- state (level,
// slope, mean).  The two model objects it is built from (Models/ZeroMeanGaussianModel.hpp,
// Models/TimeSeries/NonzeroMeanAr1Model.hpp:77-84) hold the initial parameter values only.
class ZeroMeanGaussianModel {
 public:
  explicit ZeroMeanGaussianModel(double sigma = 1.0) : sigma_(sigma) {}
  double sigma() const { return sigma_; }
  double sigma_;
};
class NonzeroMeanAr1Model {
 public:
  explicit NonzeroMeanAr1Model(double mu = 0.0, double phi = 0.0, double sigma = 1.0) : mu_(mu), phi_(phi), sigma_(sigma) {}
  double mu() const { return mu_; }
  double phi() const { return phi_; }
  double sigma() const { return sigma_; }
  double mu_, phi_, sigma_;
};
class SemilocalLinearTrendStateModel {
 public:
  SemilocalLinearTrendStateModel(const Ptr<ZeroMeanGaussianModel> &level, const Ptr<NonzeroMeanAr1Model> &slope)
      : level_(level), slope_(slope) {}
  int state_dimension() const { return 3; }
  void set_initial_level_mean(double m) { a0_[0] = m; }
  void set_initial_level_sd(double sd) { P0_[0] = sd * sd; }
  void set_initial_slope_mean(double m) { a0_[1] = m; }
  void set_initial_slope_sd(double sd) { P0_[1] = sd * sd; }
  // ZeroMeanGaussianConjSampler(level, df, sigma_guess) + set_sigma_upper_limit
  void set_level_prior(double df, double sigma_guess, double sigma_upper_limit = infinity()) {
    df_[0] = df; guess_[0] = sigma_guess; upper_[0] = sigma_upper_limit;
  }
  // NonzeroMeanAr1Sampler(slope, GaussianModel(mean_mu, mean_sigma), GaussianModel(ar1_mu, ar1_sigma),
  // ChisqModel(df, sigma_guess)) + set_sigma_upper_limit, force_stationary(), force_ar1_positive()
  void set_slope_prior(double mean_mu, double mean_sigma, double ar1_mu, double ar1_sigma, double df,
                       double sigma_guess, double sigma_upper_limit = infinity(), bool force_stationary = true,
                       bool force_ar1_positive = false) {
    prior_[0] = mean_mu; prior_[1] = mean_sigma; prior_[2] = ar1_mu; prior_[3] = ar1_sigma;
    df_[1] = df; guess_[1] = sigma_guess; upper_[1] = sigma_upper_limit;
    force_stationary_ = force_stationary; force_positive_ = force_ar1_positive;
  }
  Ptr<ZeroMeanGaussianModel> level_;
  Ptr<NonzeroMeanAr1Model> slope_;
  double a0_[3] = {0.0, 0.0, 0.0}, P0_[3] = {1.0, 1.0, 0.0};
  double df_[2] = {1.0, 1.0}, guess_[2] = {1.0, 1.0}, upper_[2] = {infinity(), infinity()};
  double prior_[4] = {0.0, 1.0, 0.0, 1.0};
  bool force_stationary_ = true, force_positive_ = false;
};

class StateSpaceRegressionModel : public Model {
 public:
  StateSpaceRegressionModel(const Vector &y, const Matrix &X, const std::vector<bool> &observed,
                            int chains = 1, uint64_t seed = 8675309, int device = 0)
      : eng_(new Engine(chains, seed, device)), T_((int)y.size()), p_(X.ncol()) {
    if (X.nrow() != T_) report_error("X and y are incompatible in constructor for StateSpaceRegressionModel.");
    std::vector<uint8_t> obs;
    if (!observed.empty()) { obs.resize(T_); for (int t = 0; t < T_; ++t) obs[t] = observed[t]; }
    eng_->check(ba_ss_set_data(eng_->get(), T_, p_, y.data(), X.data(), obs.empty() ? nullptr : obs.data()));
  }
  // add_state, in any order and number (StateSpaceModelBase.hpp:637-638): the list goes to
  // the device when the sampler is attached or at the first draw (finalize_state)
  void add_state(const Ptr<LocalLevelStateModel> &s) { Entry e; e.kind = 1; e.level = s; models_.push_back(e); finalized_ = false; }
  void add_state(const Ptr<LocalLinearTrendStateModel> &s) { Entry e; e.kind = 2; e.trend = s; models_.push_back(e); finalized_ = false; }
  void add_state(const Ptr<SeasonalStateModel> &s) { Entry e; e.kind = 3; e.seasonal = s; models_.push_back(e); finalized_ = false; }
  void add_state(const Ptr<ArStateModel> &s) { Entry e; e.kind = 4; e.ar = s; models_.push_back(e); finalized_ = false; }
  void add_state(const Ptr<StaticInterceptStateModel> &s) { Entry e; e.kind = 5; e.intercept = s; models_.push_back(e); finalized_ = false; }
  void add_state(const Ptr<TrigStateModel> &s) { Entry e; e.kind = 6; e.trig = s; models_.push_back(e); finalized_ = false; }
  void add_state(const Ptr<SemilocalLinearTrendStateModel> &s) { Entry e; e.kind = 7; e.semilocal = s; models_.push_back(e); finalized_ = false; }
  void add_state(const Ptr<StudentLocalLinearTrendStateModel> &s) { Entry e; e.kind = 8; e.student_trend = s; models_.push_back(e); finalized_ = false; }
  void add_state(const Ptr<RandomWalkHolidayStateModel> &s) { Entry e; e.kind = 10; e.holiday = s; models_.push_back(e); finalized_ = false; }
  void add_state(const Ptr<MonthlyAnnualCycle> &s) { Entry e; e.kind = 11; e.monthly = s; models_.push_back(e); finalized_ = false; }
  void add_state(const Ptr<DynamicRegressionStateModel> &s) { Entry e; e.kind = 12; e.dynreg = s; models_.push_back(e); finalized_ = false; }
  void add_state(const Ptr<DynamicRegressionArStateModel> &s) { Entry e; e.kind = 14; e.dynreg_ar = s; models_.push_back(e); finalized_ = false; }
  // (no block of the state: the engine numbers the regression holiday models on their own)
  void add_state(const Ptr<RegressionHolidayStateModel> &s) { reg_holidays_.push_back(s); hier_holidays_.push_back(nullptr); finalized_ = false; }
  // (a hierarchical one takes a place among them: reg_holidays_[k] is null where hier_holidays_[k] is not)
  void add_state(const Ptr<HierarchicalRegressionHolidayStateModel> &s) { reg_holidays_.push_back(nullptr); hier_holidays_.push_back(s); finalized_ = false; }
  int number_of_state_models() const { return (int)models_.size(); }
  bool has_student_trend() const {
    for (const Entry &e : models_) if (e.kind == 8) return true;
    return false;
  }
  bool has_regression_holiday() const { return !reg_holidays_.empty(); }
  // anything but a lone local level (which runs the local-level kernels; the Student-t family
  // always sends the list, and so does a model with a regression holiday)
  bool structural() const { return list_always_ || !reg_holidays_.empty() || !(models_.size() == 1 && models_[0].kind == 1); }
  int state_dimension() const {
    int m = 0;
    for (const Entry &e : models_)
      m += (e.kind == 1 || e.kind == 5) ? 1 : (e.kind == 2 || e.kind == 8) ? 2 : e.kind == 3 ? e.seasonal->state_dimension()
           : e.kind == 6 ? e.trig->state_dimension() : e.kind == 7 ? 3 : e.kind == 10 ? e.holiday->state_dimension() : e.kind == 11 ? e.monthly->state_dimension()
           : e.kind == 12 ? e.dynreg->state_dimension() : e.kind == 14 ? e.dynreg_ar->state_dimension() : e.ar->lags_;
    return m;
  }
  void finalize_state() {
    if (finalized_) return;
    if (models_.empty()) report_error("No state has been defined.");
    ba_engine *h = eng_->get();
    if (!structural()) {
      const LocalLevelStateModel &s = *models_[0].level;
      eng_->check(ba_ss_set_local_level(h, s.df_, s.guess_, s.upper_, s.a0_, s.P0_, s.sigma_));
    } else {
      eng_->check(ba_ss_clear_state_models(h));
      for (size_t b = 0; b < models_.size(); ++b) {
        const Entry &e = models_[b];
        if (e.kind == 10) {
          const RandomWalkHolidayStateModel &s = *e.holiday;
          const int32_t ip[3] = {s.width_, 0, 0};
          eng_->check(ba_ss_add_state_model(h, 10, ip, &s.df_, &s.guess_, &s.upper_, &s.sigma_, nullptr, s.a0_.data(), s.P0_.data()));
          eng_->check(ba_ss_set_holiday_calendar(h, engine_block(b), s.positions_.data(), (int64_t)s.positions_.size()));
        } else if (e.kind == 12) {
          const DynamicRegressionStateModel &s = *e.dynreg;
          eng_->check(ba_ss_add_dynamic_regression(h, s.xdim_, s.x_.data(), s.rows_, s.df_.data(), s.guess_.data(), s.upper_.data(),
                                                   s.sigma_.data(), s.a0_.data(), s.P0_.data()));
        } else if (e.kind == 14) {
          const DynamicRegressionArStateModel &s = *e.dynreg_ar;
          eng_->check(ba_ss_add_dynamic_regression_ar(h, s.xdim_, s.lags_, s.x_.data(), s.rows_, s.df_.data(), s.guess_.data(), s.upper_.data(),
                                                      s.sigma_.data(), s.phi_.data(), s.a0_.data(), s.P0_.data(), nullptr));
        } else if (e.kind == 11) {
          const MonthlyAnnualCycle &s = *e.monthly;
          const int32_t ip[3] = {s.nseasons(), 0, 0};
          const std::vector<uint8_t> flags = s.calendar(T_);
          eng_->check(ba_ss_add_state_model(h, 11, ip, &s.df_, &s.guess_, &s.upper_, &s.sigma_, nullptr, s.a0_.data(), s.P0_.data()));
          eng_->check(ba_ss_set_season_calendar(h, engine_block(b), flags.data(), (int64_t)flags.size()));
        } else if (e.kind == 1) {
          const LocalLevelStateModel &s = *e.level;
          eng_->check(ba_ss_add_state_model(h, 1, nullptr, &s.df_, &s.guess_, &s.upper_, &s.sigma_, nullptr, &s.a0_, &s.P0_));
        } else if (e.kind == 2) {
          const LocalLinearTrendStateModel &s = *e.trend;
          eng_->check(ba_ss_add_state_model(h, 2, nullptr, s.df_, s.guess_, s.upper_, s.sigma_, nullptr, s.a0_.data(), s.P0_.data()));
        } else if (e.kind == 3) {
          const SeasonalStateModel &s = *e.seasonal;
          const int32_t ip[3] = {s.nseasons_, s.duration_, s.t0_};
          eng_->check(ba_ss_add_state_model(h, 3, ip, &s.df_, &s.guess_, &s.upper_, &s.sigma_, nullptr, s.a0_.data(), s.P0_.data()));
        } else if (e.kind == 5) {
          const StaticInterceptStateModel &s = *e.intercept;
          eng_->check(ba_ss_add_state_model(h, 5, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &s.a0_, &s.P0_));
        } else if (e.kind == 7) {
          const SemilocalLinearTrendStateModel &s = *e.semilocal;
          const int32_t ip[3] = {s.force_stationary_ ? 1 : 0, s.force_positive_ ? 1 : 0, 0};
          const double sig[2] = {s.level_->sigma_, s.slope_->sigma_};
          const double pp[6] = {s.prior_[0], s.prior_[1], s.prior_[2], s.prior_[3], s.slope_->mu_, s.slope_->phi_};
          eng_->check(ba_ss_add_state_model(h, 7, ip, s.df_, s.guess_, s.upper_, sig, pp, s.a0_, s.P0_));
        } else if (e.kind == 8) {
          const StudentLocalLinearTrendStateModel &s = *e.student_trend;
          const double pp[8] = {(double)s.nu_kind_[0], s.nu_a_[0], s.nu_b_[0], (double)s.nu_kind_[1], s.nu_a_[1], s.nu_b_[1],
                                s.nu_[0], s.nu_[1]};
          eng_->check(ba_ss_set_lookahead(h, 1));   // (the engine refuses a look-ahead with this model)
          eng_->check(ba_ss_add_state_model(h, 8, nullptr, s.df_, s.guess_, s.upper_, s.sigma_, pp, s.a0_.data(), s.P0_.data()));
        } else if (e.kind == 6) {
          const TrigStateModel &s = *e.trig;
          const int32_t ip[3] = {(int32_t)s.frequencies_.size(), 0, 0};
          eng_->check(ba_ss_add_state_model(h, 6, ip, &s.df_, &s.guess_, &s.upper_, &s.sigma_, s.rotations_.data(), s.a0_.data(), s.P0_.data()));
        } else {
          const ArStateModel &s = *e.ar;
          if (s.spike_slab_) {
            // kind 9: initial_phi = coefficients | slab mean | inclusion probabilities | slab precision (column-major)
            const int32_t ip9[4] = {s.lags_, s.truncate_ ? 1 : 0, s.max_flips_, 1};
            std::vector<double> ph;
            for (int i = 0; i < s.lags_; ++i) ph.push_back(s.phi_[i]);
            for (int i = 0; i < s.lags_; ++i) ph.push_back(s.slab_mu_[i]);
            for (int i = 0; i < s.lags_; ++i) ph.push_back(s.spike_pi_[i]);
            for (int j = 0; j < s.lags_; ++j)
              for (int i = 0; i < s.lags_; ++i) ph.push_back(s.slab_siginv_(i, j));
            eng_->check(ba_ss_add_state_model(h, 9, ip9, &s.df_, &s.guess_, &s.upper_, &s.sigma_, ph.data(), s.a0_.data(), s.P0_.data()));
            continue;
          }
          const int32_t ip[3] = {s.lags_, 0, 0};
          eng_->check(ba_ss_add_state_model(h, 4, ip, &s.df_, &s.guess_, &s.upper_, &s.sigma_, s.phi_.data(), s.a0_.data(), s.P0_.data()));
        }
      }
      for (size_t k = 0; k < reg_holidays_.size(); ++k) {
        int32_t model = -1;
        eng_->check(ba_ss_set_lookahead(h, 1));   // (the engine refuses a look-ahead with this model)
        if (hier_holidays_[k]) {
          HierarchicalRegressionHolidayStateModel &s = *hier_holidays_[k];
          eng_->check(ba_ss_add_hierarchical_regression_holiday(h, s.nholidays_, s.width_, s.mean_prior_mean_.data(),
                                                                s.mean_prior_variance_.data(), s.variance_guess_.data(), s.weight_,
                                                                s.coef_.data(), &model));
          if (!s.calendar_.empty())
            eng_->check(ba_ss_set_regression_holiday_calendar(h, model, s.calendar_.data(), (int64_t)s.calendar_.size()));
          s.engine_ = eng_;
          s.index_ = model;
          continue;
        }
        const RegressionHolidayStateModel &s = *reg_holidays_[k];
        eng_->check(ba_ss_add_regression_holiday(h, (int32_t)s.widths_.size(), s.widths_.data(), s.prior_mean_, s.prior_sd_,
                                                 s.coef_.data(), &model));
        if (!s.calendar_.empty())
          eng_->check(ba_ss_set_regression_holiday_calendar(h, model, s.calendar_.data(), (int64_t)s.calendar_.size()));
      }
    }
    finalized_ = true;
  }
  // the coefficients of the `which`-th RegressionHolidayStateModel in one chain's current draw
  Vector regression_holiday_coefficients(int chain = 0, int which = 0) const {
    if (which < 0 || which >= (int)reg_holidays_.size()) report_error("The model has no such RegressionHolidayStateModel.");
    Vector v(hier_holidays_[which] ? hier_holidays_[which]->number_of_coefficients() : reg_holidays_[which]->number_of_coefficients());
    eng_->check(ba_ss_get_regression_holiday(eng_->get(), chain, which, v.data(), nullptr, nullptr));
    return v;
  }
  // the coefficients and error variance of the `which`-th ArStateModel in one chain's current draw
  Vector ar_phi(int chain = 0, int which = 0) const {
    const int b = ar_block(which);
    Vector v(models_[b].ar->lags_);
    eng_->check(ba_ss_get_state_model(eng_->get(), chain, engine_block(b), nullptr, nullptr, nullptr, v.data(), nullptr, nullptr, nullptr, nullptr));
    return v;
  }
  // the coefficients of the `which`-th DynamicRegressionArStateModel's autoregressions in one chain's current
  // draw: xdim x lags, row i = coefficient i's phi (their error variances: state_variances)
  Matrix dynamic_regression_ar_phi(int chain = 0, int which = 0) const {
    int seen = 0;
    for (size_t b = 0; b < models_.size(); ++b) {
      if (models_[b].kind != 14 || seen++ != which) continue;
      const DynamicRegressionArStateModel &s = *models_[b].dynreg_ar;
      Matrix phi(s.xdim_, s.lags_);
      Vector v(s.lags_);
      for (int i = 0; i < s.xdim_; ++i) {
        eng_->check(ba_ss_get_state_model(eng_->get(), chain, engine_block(b) + i, nullptr, nullptr, nullptr, v.data(), nullptr, nullptr, nullptr, nullptr));
        for (int j = 0; j < s.lags_; ++j) phi(i, j) = v[j];
      }
      return phi;
    }
    report_error("The model has no such DynamicRegressionArStateModel.");
    return Matrix();
  }
  // the inclusion indicators of the `which`-th ArStateModel (one with set_spike_slab_prior) in one chain
  std::vector<bool> ar_inclusion(int chain = 0, int which = 0) const {
    const int b = ar_block(which);
    std::vector<uint8_t> g(models_[b].ar->lags_);
    eng_->check(ba_ss_get_ar_inclusion(eng_->get(), chain, engine_block(b), g.data()));
    return std::vector<bool>(g.begin(), g.end());
  }
  double ar_sigsq(int chain = 0, int which = 0) const {
    double s2;
    eng_->check(ba_ss_get_state_model(eng_->get(), chain, engine_block(ar_block(which)), &s2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    return s2;
  }
  // the slope model of the `which`-th SemilocalLinearTrendStateModel in one chain's current draw:
  // (AR(1) coefficient, long-run mean)
  Vector semilocal_slope(int chain = 0, int which = 0) const {
    int seen = 0;
    for (size_t b = 0; b < models_.size(); ++b) {
      if (models_[b].kind != 7 || seen++ != which) continue;
      Vector v(2);
      eng_->check(ba_ss_get_state_model(eng_->get(), chain, engine_block(b), nullptr, nullptr, nullptr, v.data(), nullptr, nullptr, nullptr, nullptr));
      return v;
    }
    report_error("The model has no such SemilocalLinearTrendStateModel.");
    return Vector();
  }
  // the StudentLocalLinearTrendStateModel in one chain's current draw: (nu_level, nu_slope), and its
  // weights, 2 x time_dimension (row 0 the level's, row 1 the slope's)
  Vector student_trend_nu(int chain = 0) const {
    Vector v(2);
    eng_->check(ba_ss_get_state_model(eng_->get(), chain, engine_block(student_trend_block()), nullptr, nullptr, nullptr, v.data(), nullptr, nullptr, nullptr, nullptr));
    return v;
  }
  Matrix student_trend_weights(int chain = 0) const {
    student_trend_block();
    Vector lw(T_), sw(T_);
    eng_->check(ba_ss_trend_get_weights(eng_->get(), chain, lw.data(), sw.data()));
    Matrix w(2, T_);
    for (int t = 0; t < T_; ++t) { w(0, t) = lw[t]; w(1, t) = sw[t]; }
    return w;
  }
  // one chain's state draw: state_dimension x time_dimension, the models' components in
  // the order the models were added
  Matrix structural_state(int chain = 0) const {
    const int m = state_dimension();
    Vector buf((size_t)T_ * m);
    eng_->check(ba_ss_get_state_draw(eng_->get(), chain, buf.data()));
    Matrix st(m, T_);
    for (int t = 0; t < T_; ++t) for (int i = 0; i < m; ++i) st(i, t) = buf[(size_t)t * m + i];
    return st;
  }
  // every variance parameter in state-model order (a local linear trend has two: level,
  // slope; an autoregression's is its error variance; a static intercept has none)
  Vector state_variances(int chain = 0) const {
    std::vector<double> out;
    for (size_t b = 0; b < models_.size(); ++b) {
      if (models_[b].kind == 5) continue;
      double v[16] = {0, 0};   // (a dynamic regression: one per coefficient, at most the list's 16 slots)
      if (models_[b].kind == 14) {   // (an AR dynamic regression: a state model of the engine's list per coefficient)
        for (int i = 0; i < models_[b].dynreg_ar->xdim(); ++i) {
          eng_->check(ba_ss_get_state_model(eng_->get(), chain, engine_block(b) + i, v, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
          out.push_back(v[0]);
        }
        continue;
      }
      eng_->check(ba_ss_get_state_model(eng_->get(), chain, engine_block(b), v, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
      out.push_back(v[0]);
      if (models_[b].kind == 12)
        for (int i = 1; i < models_[b].dynreg->xdim(); ++i) out.push_back(v[i]);
      if (models_[b].kind == 2 || models_[b].kind == 7 || models_[b].kind == 8) out.push_back(v[1]);
    }
    Vector ans(out.size());
    for (size_t i = 0; i < out.size(); ++i) ans[i] = out[i];
    return ans;
  }
  int time_dimension() const { return T_; }
  int xdim() const { return p_; }
  const Ptr<Engine> &engine() const { return eng_; }
  const LocalLevelStateModel *level() const { return structural() ? nullptr : models_[0].level.get(); }
  Vector state(int chain = 0) const {
    Vector st(T_);
    eng_->check(ba_ss_get_state(eng_->get(), chain, st.data(), nullptr, nullptr, nullptr));
    return st;
  }
  double level_sigsq(int chain = 0) const {
    double v;
    eng_->check(ba_ss_get_state(eng_->get(), chain, nullptr, &v, nullptr, nullptr));
    return v;
  }
  // ScalarStateSpaceModelBase::one_step_prediction_errors (StateSpaceModelBase.cpp:682-691) for
  // EVERY chain's current draw: time_dimension x chains, column c = chain c (bsts's
  // one.step.prediction.errors); standardize: v_t / sqrt(F_t).  Gaussian observation model only:
  // the Student-t, Poisson and logit families throw the engine's refusal.
  Matrix one_step_prediction_errors(bool standardize = false) {
    finalize_state();
    Matrix ans(T_, eng_->chains());
    eng_->check(ba_ss_prediction_errors(eng_->get(), 0, eng_->chains(), standardize ? 1 : 0, ans.data(), nullptr, nullptr));
    return ans;
  }
  // StateSpaceRegressionModel::one_step_holdout_prediction_errors(newX, newY, final_state, standardize)
  // (StateSpaceRegressionModel.cpp:280-305) for EVERY chain's current draw and its own final state: chains x
  // newY.size(), row c = chain c (bsts.prediction.errors' holdout part).  Refused by the engine: the Student-t,
  // Poisson and logit families, a Student local linear trend, regression holiday models.
  Matrix one_step_holdout_prediction_errors(const Matrix &newX, const Vector &newY, bool standardize = false) {
    if (newX.nrow() != (int)newY.size()) report_error("X and y do not match in one_step_holdout_prediction_errors.");
    if (newX.ncol() != p_) report_error("The holdout predictors do not match the model dimension.");
    finalize_state();
    const int h = (int)newY.size(), chains = (int)eng_->chains();
    std::vector<double> rows((size_t)chains * (size_t)(h > 0 ? h : 0));
    eng_->check(ba_ss_holdout_prediction_errors(eng_->get(), 0, chains, standardize ? 1 : 0, h, p_ > 0 ? newX.data() : nullptr,
                                                newY.data(), rows.data(), nullptr));
    Matrix ans(chains, h);
    for (int c = 0; c < chains; ++c)
      for (int i = 0; i < h; ++i) ans(c, i) = rows[(size_t)c * h + i];
    return ans;
  }
  // the filter's log likelihood of every chain's current draw (bsts's log.likelihood), one entry per chain
  Vector log_likelihood() {
    finalize_state();
    Vector ans(eng_->chains());
    eng_->check(ba_ss_prediction_errors(eng_->get(), 0, eng_->chains(), 0, nullptr, nullptr, ans.data()));
    return ans;
  }
 protected:
  // StateSpaceStudentRegressionModel: the same state, the Student-t observation model
  struct StudentFamily {};
  StateSpaceRegressionModel(StudentFamily, const Vector &y, const Matrix &X, const std::vector<bool> &observed,
                            int chains, uint64_t seed, int device)
      : eng_(new Engine(chains, seed, device)), T_((int)y.size()), p_(X.ncol()), list_always_(true) {
    if (X.nrow() != T_) report_error("X and y are incompatible in constructor for StateSpaceStudentRegressionModel.");
    std::vector<uint8_t> obs;
    if (!observed.empty()) { obs.resize(T_); for (int t = 0; t < T_; ++t) obs[t] = observed[t]; }
    eng_->check(ba_ss_student_set_data(eng_->get(), T_, p_, y.data(), X.data(), obs.empty() ? nullptr : obs.data()));
  }
  // StateSpacePoissonModel: the same state, the Poisson observation model
  struct PoissonFamily {};
  StateSpaceRegressionModel(PoissonFamily, const Vector &counts, const Vector &exposure, const Matrix &X,
                            const std::vector<bool> &observed, int chains, uint64_t seed, int device)
      : eng_(new Engine(chains, seed, device)), T_((int)counts.size()), p_(X.ncol()), list_always_(true) {
    if (X.nrow() != T_ || (int)exposure.size() != T_)
      report_error("counts, exposure and X are incompatible in constructor for StateSpacePoissonModel.");
    std::vector<uint8_t> obs;
    if (!observed.empty()) { obs.resize(T_); for (int t = 0; t < T_; ++t) obs[t] = observed[t]; }
    eng_->check(ba_ss_poisson_set_data(eng_->get(), T_, p_, counts.data(), exposure.data(), X.data(),
                                       obs.empty() ? nullptr : obs.data()));
  }
  // StateSpaceLogitModel: the same state, the binomial logit observation model
  struct LogitFamily {};
  StateSpaceRegressionModel(LogitFamily, const Vector &successes, const Vector &trials, const Matrix &X,
                            const std::vector<bool> &observed, int clt_threshold, int chains, uint64_t seed, int device)
      : eng_(new Engine(chains, seed, device)), T_((int)successes.size()), p_(X.ncol()), list_always_(true) {
    if (X.nrow() != T_ || (int)trials.size() != T_)
      report_error("successes, trials and X are incompatible in constructor for StateSpaceLogitModel.");
    std::vector<uint8_t> obs;
    if (!observed.empty()) { obs.resize(T_); for (int t = 0; t < T_; ++t) obs[t] = observed[t]; }
    eng_->check(ba_ss_logit_set_data(eng_->get(), T_, p_, successes.data(), trials.data(), X.data(),
                                     obs.empty() ? nullptr : obs.data(), clt_threshold));
  }
 private:
  struct Entry {
    int kind = 0;   // 1 local level, 2 local linear trend, 3 seasonal, 4 autoregression, 5 static intercept, 6 trig, 7 semilocal linear trend, 8 Student local linear trend, 10 random-walk holiday, 11 monthly annual cycle (a calendar seasonal), 12 dynamic regression, 14 AR dynamic regression
    Ptr<LocalLevelStateModel> level;
    Ptr<LocalLinearTrendStateModel> trend;
    Ptr<SeasonalStateModel> seasonal;
    Ptr<ArStateModel> ar;
    Ptr<StaticInterceptStateModel> intercept;
    Ptr<TrigStateModel> trig;
    Ptr<SemilocalLinearTrendStateModel> semilocal;
    Ptr<StudentLocalLinearTrendStateModel> student_trend;
    Ptr<RandomWalkHolidayStateModel> holiday;
    Ptr<DynamicRegressionStateModel> dynreg;
    Ptr<DynamicRegressionArStateModel> dynreg_ar;
    Ptr<MonthlyAnnualCycle> monthly;
  };
  // the index of model b's (first) state model in the engine's list: an AR dynamic regression is one per coefficient
  int32_t engine_block(size_t b) const {
    int32_t at = 0;
    for (size_t i = 0; i < b && i < models_.size(); ++i) at += models_[i].kind == 14 ? models_[i].dynreg_ar->xdim() : 1;
    return at;
  }
  int student_trend_block() const {
    for (size_t b = 0; b < models_.size(); ++b)
      if (models_[b].kind == 8) return (int)b;
    report_error("The model has no StudentLocalLinearTrendStateModel.");
    return -1;
  }
  int ar_block(int which) const {
    int seen = 0;
    for (size_t b = 0; b < models_.size(); ++b)
      if (models_[b].kind == 4 && seen++ == which) return (int)b;
    report_error("The model has no such ArStateModel.");
    return -1;
  }
  Ptr<Engine> eng_;
  int T_, p_;
  std::vector<Entry> models_;
  std::vector<Ptr<RegressionHolidayStateModel>> reg_holidays_;
  std::vector<Ptr<HierarchicalRegressionHolidayStateModel>> hier_holidays_;
  bool finalized_ = false;
  bool list_always_ = false;
};

// regression priors are set through the same three pieces as BregVsSampler
class StateSpacePosteriorSampler : public PosteriorSampler {
 public:
  StateSpacePosteriorSampler(StateSpaceRegressionModel *model, const Ptr<MvnGivenScalarSigma> &slab,
                             const Ptr<ChisqModel> &residual_precision_prior,
                             const Ptr<VariableSelectionPrior> &spike,
                             double sigma_upper_limit = infinity())
      : model_(model) {
    ba_engine *h = model->engine()->get();
    model->engine()->check(ba_set_slab(h, slab->mu().data(), slab->unscaled_precision().data()));
    model->engine()->check(ba_set_spike(h, spike->prior_inclusion_probabilities().data(), spike->max_model_size()));
    model->engine()->check(ba_set_sigma_prior(h, residual_precision_prior->df(), residual_precision_prior->sigma(), sigma_upper_limit));
    std::vector<uint8_t> g0(model->xdim(), 0);
    model->engine()->check(ba_set_state(h, -1, g0.data(), nullptr, 1.0));
    // the callers' per-iteration loop at the device's rate (ba_ss_draw_next serves the
    // rounds from batches enqueued ahead; nothing a caller does can observe it)
    // (a StudentLocalLinearTrendStateModel's weights and a RegressionHolidayStateModel's coefficients -- a
    // hierarchical one's too -- are not in the look-ahead's snapshots: one round per draw)
    model->engine()->check(ba_ss_set_lookahead(h, (model->has_student_trend() || model->has_regression_holiday()) ? 1 : 64));
  }
  void set_lookahead(int rounds) { model_->engine()->check(ba_ss_set_lookahead(model_->engine()->get(), rounds)); }
  void draw() override {                     // StateSpacePosteriorSampler.cpp:42-64
    model_->finalize_state();
    model_->engine()->check(ba_ss_draw_next(model_->engine()->get()));
  }
  // StateSpacePosteriorSampler::logpri (StateSpacePosteriorSampler.cpp:66-74) sums
  // the observation model's and the state models' log priors; the regression
  // part is what the engine evaluates (chain 0)
  double logpri() const override {
    double out;
    model_->engine()->check(ba_logpri(model_->engine()->get(), 0, &out));
    // + LocalLevelStateModel's sampler: ZeroMeanGaussianConjSampler::logpri =
    // GenericGaussianVarianceSampler::log_prior(sigma^2_level)
    // (GenericGaussianVarianceSampler.cpp: Gamma(df/2, ss/2) density of the
    // precision and the Jacobian of the reciprocal)
    if (const LocalLevelStateModel *lv = model_->level()) {
      const double a = lv->df_ / 2, b = lv->df_ * lv->guess_ * lv->guess_ / 2;
      const double s2 = model_->level_sigsq(0), x = 1.0 / s2;
      out += a * std::log(b) - std::lgamma(a) + (a - 1.0) * std::log(x) - b * x - 2.0 * std::log(s2);
    }
    return out;
  }
  void set_seed(unsigned long s) override {
    model_->engine()->check(ba_seed(model_->engine()->get(), s));
  }
 private:
  StateSpaceRegressionModel *model_;
};

// ---- binomial probit / logit spike and slab -----------------------------------------
struct MvnModel {   // a slab whose precision does not scale with sigma^2 (MvnBase)
  MvnModel(const Vector &mean, const SpdMatrix &precision) : mu_(mean), siginv_(precision) {}
  const Vector &mu() const { return mu_; }
  const SpdMatrix &siginv() const { return siginv_; }
  int dim() const { return (int)mu_.size(); }
  Vector mu_;
  SpdMatrix siginv_;
};

// BinomialLogitModel / BinomialProbitModel(X, y, n): the coefficients live in
// coef() = (inc(), Beta()); many chains on the device, chain 0 backs the model
class BinomialRegressionModelBase : public Model {
 public:
  BinomialRegressionModelBase(const Matrix &X, const Vector &y, const Vector &n, bool logit,
                              int clt_threshold, int chains, uint64_t seed, int device)
      : eng_(new Engine(chains, seed, device)), p_(X.ncol()), logit_(logit), inc_(X.ncol(), true),
        beta_(X.ncol(), 0.0) {
    if (X.nrow() != (int)y.size() || y.size() != n.size())
      report_error("X, y and n are incompatible in the binomial regression model's constructor.");
    eng_->check(logit ? ba_logit_set_data(eng_->get(), X.nrow(), X.ncol(), X.data(), y.data(), n.data(), clt_threshold)
                      : ba_probit_set_data(eng_->get(), X.nrow(), X.ncol(), X.data(), y.data(), n.data(), clt_threshold));
  }
  int xdim() const { return p_; }
  bool logit() const { return logit_; }
  const Selector &inc() const { return inc_; }
  void drop_all() { inc_.drop_all(); dirty_ = true; }
  void add(int i) { inc_.add(i); dirty_ = true; }
  void drop(int i) { inc_.drop(i); dirty_ = true; }
  const Vector &Beta() const { return beta_; }
  void set_Beta(const Vector &b) { beta_ = b; dirty_ = true; }
  bool dirty() const { return dirty_; }
  const Ptr<Engine> &engine() const { return eng_; }
  void push_state() {
    eng_->check(ba_set_state(eng_->get(), -1, inc_.bytes().data(), beta_.data(), 1.0));
    dirty_ = false;
  }
  void pull_chain0() {
    eng_->check(ba_get_state(eng_->get(), 0, inc_.bytes().data(), beta_.data(), nullptr));
    dirty_ = false;
  }
  void chain_states(std::vector<uint8_t> &gamma, Vector &beta) const {
    const size_t C = eng_->chains();
    gamma.resize(C * p_); beta.resize(C * p_);
    eng_->check(ba_get_states(eng_->get(), gamma.data(), beta.data(), nullptr));
  }
 private:
  Ptr<Engine> eng_;
  int p_;
  bool logit_;
  Selector inc_;
  Vector beta_;
  bool dirty_ = true;
};
class BinomialLogitModel : public BinomialRegressionModelBase {
 public:
  BinomialLogitModel(const Matrix &X, const Vector &y, const Vector &n, int clt_threshold = 5,
                     int chains = 1, uint64_t seed = 8675309, int device = 0)
      : BinomialRegressionModelBase(X, y, n, true, clt_threshold, chains, seed, device) {}
};
class BinomialProbitModel : public BinomialRegressionModelBase {
 public:
  BinomialProbitModel(const Matrix &X, const Vector &y, const Vector &n, int clt_threshold = 5,
                      int chains = 1, uint64_t seed = 8675309, int device = 0)
      : BinomialRegressionModelBase(X, y, n, false, clt_threshold, chains, seed, device) {}
};

// BinomialLogitSpikeSlabSampler / BinomialProbitSpikeSlabSampler(model, slab, spike, clt_threshold)
class BinomialSpikeSlabSamplerBase : public PosteriorSampler {
 public:
  BinomialSpikeSlabSamplerBase(BinomialRegressionModelBase *model, const Ptr<MvnModel> &slab,
                               const Ptr<VariableSelectionPrior> &spike)
      : model_(model), slab_(slab) {
    if (slab->dim() != model->xdim()) report_error("Slab does not match model dimension.");
    if ((int)spike->potential_nvars() != model->xdim()) report_error("Spike does not match model dimension.");
    check(ba_sss_set_slab(h(), slab->mu().data(), slab->siginv().data(), 0, -1));
    check(ba_set_spike(h(), spike->prior_inclusion_probabilities().data(), spike->max_model_size()));
  }
  void draw() override {
    if (model_->dirty()) model_->push_state();
    check(model_->logit() ? ba_logit_sweep(h(), 1) : ba_probit_sweep(h(), 1));
    check(ba_sync(h()));
    model_->pull_chain0();
  }
  double logpri() const override { report_error("logpri() is not implemented for the binomial samplers"); return 0; }
  void set_seed(unsigned long s) override { check(ba_seed(h(), s)); }
  void limit_model_selection(int max_flips) {
    check(ba_sss_set_slab(h(), slab_->mu().data(), slab_->siginv().data(), 0, max_flips));
  }
 private:
  ba_engine *h() const { return model_->engine()->get(); }
  void check(int rc) const { model_->engine()->check(rc); }
  BinomialRegressionModelBase *model_;
  Ptr<MvnModel> slab_;
};
class BinomialLogitSpikeSlabSampler : public BinomialSpikeSlabSamplerBase {
 public:
  BinomialLogitSpikeSlabSampler(BinomialLogitModel *model, const Ptr<MvnModel> &slab,
                                const Ptr<VariableSelectionPrior> &spike)
      : BinomialSpikeSlabSamplerBase(model, slab, spike) {}
};
class BinomialProbitSpikeSlabSampler : public BinomialSpikeSlabSamplerBase {
 public:
  BinomialProbitSpikeSlabSampler(BinomialProbitModel *model, const Ptr<MvnModel> &slab,
                                 const Ptr<VariableSelectionPrior> &spike)
      : BinomialSpikeSlabSamplerBase(model, slab, spike) {}
};


// ---- Poisson regression spike and slab ---------------------------------------------------
// PoissonRegressionModel + PoissonRegressionSpikeSlabSampler (Models/Glm/
// PoissonRegressionModel.hpp, PosteriorSamplers/PoissonRegressionSpikeSlabSampler.cpp:55-108;
// the data augmentation of PoissonDataImputer.cpp:36-96).  The normal mixtures that
// approximate the negative log-gamma densities are DATA of the reference
// (create_poisson_mixture_approximation_table, NormalMixtureApproximationTable): the caller
// hands them over, as a BOOM-side binding reads them from BOOM's own table
// (bindings/boom/DevicePoissonRegressionSpikeSlabSampler.cpp).
struct NormalMixtureTable {
  std::vector<int64_t> counts;     // ascending; 1 and every positive count of the data below largest_index
  std::vector<int32_t> ncomp;      // components of each count's mixture (<= 32)
  Vector mu, sigma, weight;        // the mixtures one after the other
  int64_t largest_index = 0;       // from here on the Gaussian limit is used
};
class PoissonRegressionModel : public Model {
 public:
  PoissonRegressionModel(const Matrix &X, const Vector &y, const Vector &exposure, int chains = 1,
                         uint64_t seed = 8675309, int device = 0)
      : eng_(new Engine(chains, seed, device)), p_(X.ncol()), inc_(X.ncol(), true), beta_(X.ncol(), 0.0) {
    if (X.nrow() != (int)y.size() || y.size() != exposure.size())
      report_error("X, y and exposure are incompatible in the Poisson regression model's constructor.");
    eng_->check(ba_poisson_set_data(eng_->get(), X.nrow(), X.ncol(), X.data(), y.data(), exposure.data()));
  }
  void set_mixture_table(const NormalMixtureTable &t) {
    if (t.counts.size() != t.ncomp.size()) report_error("the mixture table's counts and ncomp differ in length");
    eng_->check(ba_poisson_set_mixtures(eng_->get(), (int32_t)t.counts.size(), t.counts.data(), t.ncomp.data(),
                                        t.mu.data(), t.sigma.data(), t.weight.data(), t.largest_index));
  }
  int xdim() const { return p_; }
  const Selector &inc() const { return inc_; }
  void drop_all() { inc_.drop_all(); dirty_ = true; }
  void add(int i) { inc_.add(i); dirty_ = true; }
  void drop(int i) { inc_.drop(i); dirty_ = true; }
  const Vector &Beta() const { return beta_; }
  void set_Beta(const Vector &b) { beta_ = b; dirty_ = true; }
  bool dirty() const { return dirty_; }
  const Ptr<Engine> &engine() const { return eng_; }
  void push_state() {
    eng_->check(ba_set_state(eng_->get(), -1, inc_.bytes().data(), beta_.data(), 1.0));
    dirty_ = false;
  }
  void pull_chain0() {
    eng_->check(ba_get_state(eng_->get(), 0, inc_.bytes().data(), beta_.data(), nullptr));
    dirty_ = false;
  }
  void chain_states(std::vector<uint8_t> &gamma, Vector &beta) const {
    const size_t C = eng_->chains();
    gamma.resize(C * p_); beta.resize(C * p_);
    eng_->check(ba_get_states(eng_->get(), gamma.data(), beta.data(), nullptr));
  }
 private:
  Ptr<Engine> eng_;
  int p_;
  Selector inc_;
  Vector beta_;
  bool dirty_ = true;
};
// PoissonRegressionSpikeSlabSampler(model, slab, spike, number_of_threads, seeding_rng)
class PoissonRegressionSpikeSlabSampler : public PosteriorSampler {
 public:
  PoissonRegressionSpikeSlabSampler(PoissonRegressionModel *model, const Ptr<MvnModel> &slab,
                                    const Ptr<VariableSelectionPrior> &spike)
      : model_(model), slab_(slab) {
    if (slab->dim() != model->xdim()) report_error("Slab does not match model dimension.");
    if ((int)spike->potential_nvars() != model->xdim()) report_error("Spike does not match model dimension.");
    check(ba_sss_set_slab(h(), slab->mu().data(), slab->siginv().data(), 0, -1));
    check(ba_set_spike(h(), spike->prior_inclusion_probabilities().data(), spike->max_model_size()));
  }
  void draw() override {
    if (model_->dirty()) model_->push_state();
    check(ba_poisson_sweep(h(), 1));
    check(ba_sync(h()));
    model_->pull_chain0();
  }
  double logpri() const override { report_error("logpri() is not implemented for the Poisson sampler"); return 0; }
  void set_seed(unsigned long s) override { check(ba_seed(h(), s)); }
  void limit_model_selection(int max_flips) {
    check(ba_sss_set_slab(h(), slab_->mu().data(), slab_->siginv().data(), 0, max_flips));
  }
 private:
  ba_engine *h() const { return model_->engine()->get(); }
  void check(int rc) const { model_->engine()->check(rc); }
  PoissonRegressionModel *model_;
  Ptr<MvnModel> slab_;
};

// ---- Student-t regression spike and slab ----------------------------------------------
// TRegressionModel + TRegressionSpikeSlabSampler (Models/Glm/TRegression.hpp,
// PosteriorSamplers/TRegressionSpikeSlabSampler.cpp:41-47): the weights, the inclusion /
// coefficient draws given sigma^2, sigma^2 and the slice-sampler draw of nu, on the device
// (ba_student_*).  The prior on nu is a UniformModel(lo, hi) or a GammaModel(a, b).
struct DoubleModel {
  DoubleModel(int kind, double a, double b) : kind_(kind), a_(a), b_(b) {}
  virtual ~DoubleModel() {}
  int kind_;
  double a_, b_;
};
struct UniformModel : DoubleModel {
  UniformModel(double lo = 0.0, double hi = 1.0) : DoubleModel(0, lo, hi) {}
  double lo() const { return a_; }
  double hi() const { return b_; }
};
struct GammaModel : DoubleModel {   // shape a, rate b
  GammaModel(double a = 1.0, double b = 1.0) : DoubleModel(1, a, b) {}
  double alpha() const { return a_; }
  double beta() const { return b_; }
};

// TRegressionModel(X, y): sigma^2 = 1 and nu = 30 (TRegression.cpp:35-45); chain 0 backs
// the model's accessors
class TRegressionModel : public Model {
 public:
  TRegressionModel(const Matrix &X, const Vector &y, int chains = 1, uint64_t seed = 8675309, int device = 0)
      : eng_(new Engine(chains, seed, device)), p_(X.ncol()), inc_(X.ncol(), true), beta_(X.ncol(), 0.0) {
    if (X.nrow() != (int)y.size()) report_error("X and y are incompatible in TRegressionModel constructor.");
    eng_->check(ba_student_set_data(eng_->get(), X.nrow(), X.ncol(), X.data(), y.data()));
  }
  int xdim() const { return p_; }
  const Selector &inc() const { return inc_; }
  void drop_all() { inc_.drop_all(); dirty_ = true; }
  void add(int i) { inc_.add(i); dirty_ = true; }
  void drop(int i) { inc_.drop(i); dirty_ = true; }
  const Vector &Beta() const { return beta_; }
  void set_Beta(const Vector &b) { beta_ = b; dirty_ = true; }
  double sigsq() const { return sigsq_; }
  void set_sigsq(double s2) { sigsq_ = s2; dirty_ = true; }
  double nu() const { return nu_; }
  void set_nu(double nu) {
    eng_->check(ba_student_set_nu(eng_->get(), -1, nu));
    nu_ = nu;
  }
  bool dirty() const { return dirty_; }
  const Ptr<Engine> &engine() const { return eng_; }
  void push_state() {
    eng_->check(ba_set_state(eng_->get(), -1, inc_.bytes().data(), beta_.data(), sigsq_));
    dirty_ = false;
  }
  void pull_chain0() {
    eng_->check(ba_get_state(eng_->get(), 0, inc_.bytes().data(), beta_.data(), &sigsq_));
    eng_->check(ba_student_get_nu(eng_->get(), 0, &nu_));
    dirty_ = false;
  }
 private:
  Ptr<Engine> eng_;
  int p_;
  Selector inc_;
  Vector beta_;
  double sigsq_ = 1.0, nu_ = 30.0;
  bool dirty_ = true;
};
// TRegressionSpikeSlabSampler(model, slab, spike, siginv_prior, nu_prior)
class TRegressionSpikeSlabSampler : public PosteriorSampler {
 public:
  TRegressionSpikeSlabSampler(TRegressionModel *model, const Ptr<MvnGivenScalarSigma> &slab,
                              const Ptr<VariableSelectionPrior> &spike, const Ptr<ChisqModel> &siginv_prior,
                              const Ptr<DoubleModel> &nu_prior)
      : model_(model), slab_(slab), siginv_(siginv_prior) {
    if (slab->dim() != model->xdim()) report_error("Slab does not match model dimension.");
    if ((int)spike->potential_nvars() != model->xdim()) report_error("Spike does not match model dimension.");
    check(ba_sss_set_slab(h(), slab->mu().data(), slab->unscaled_precision().data(), 1, -1));
    check(ba_set_spike(h(), spike->prior_inclusion_probabilities().data(), spike->max_model_size()));
    check(ba_set_sigma_prior(h(), siginv_prior->df(), siginv_prior->sigma(), sigma_max_));
    check(ba_student_set_nu_prior(h(), nu_prior->kind_, nu_prior->a_, nu_prior->b_));
  }
  void draw() override {
    if (model_->dirty()) model_->push_state();
    check(ba_student_sweep(h(), 1));
    check(ba_sync(h()));
    model_->pull_chain0();
  }
  double logpri() const override { report_error("logpri() is not implemented for the Student-t sampler"); return 0; }
  void set_seed(unsigned long s) override { check(ba_seed(h(), s)); }
  void set_sigma_upper_limit(double max_sigma) {
    sigma_max_ = max_sigma;
    check(ba_set_sigma_prior(h(), siginv_->df(), siginv_->sigma(), sigma_max_));
  }
  void limit_model_selection(int max_flips) {
    check(ba_sss_set_slab(h(), slab_->mu().data(), slab_->unscaled_precision().data(), 1, max_flips));
  }
  void allow_model_selection(bool allow) { check(ba_student_allow_model_selection(h(), allow ? 1 : 0)); }
 private:
  ba_engine *h() const { return model_->engine()->get(); }
  void check(int rc) const { model_->engine()->check(rc); }
  TRegressionModel *model_;
  Ptr<MvnGivenScalarSigma> slab_;
  Ptr<ChisqModel> siginv_;
  double sigma_max_ = std::numeric_limits<double>::infinity();
};

// ---- bsts family = "student" --------------------------------------------------------------
// StateSpaceStudentRegressionModel + StateSpaceStudentPosteriorSampler (Models/StateSpace/
// StateSpaceStudentRegressionModel.hpp, PosteriorSamplers/StateSpaceStudentPosteriorSampler.cpp:
// 56-126): the state of StateSpaceRegressionModel with TRegressionModel's observation noise, on
// the device (ba_ss_student_*).  One observation per time step.  Chain 0 backs the accessors'
// defaults.
class StateSpaceStudentRegressionModel : public StateSpaceRegressionModel {
 public:
  StateSpaceStudentRegressionModel(const Vector &y, const Matrix &X, const std::vector<bool> &observed,
                                   int chains = 1, uint64_t seed = 8675309, int device = 0)
      : StateSpaceRegressionModel(StudentFamily(), y, X, observed, chains, seed, device) {}
  double nu(int chain = 0) const {
    double v;
    engine()->check(ba_student_get_nu(engine()->get(), chain, &v));
    return v;
  }
  void set_nu(double nu) { engine()->check(ba_student_set_nu(engine()->get(), -1, nu)); }
  double sigsq(int chain = 0) const {
    double v;
    engine()->check(ba_get_state(engine()->get(), chain, nullptr, nullptr, &v));
    return v;
  }
  // the latent weights of one chain (AugmentedStudentRegressionData::weight); 0 at a missing step
  Vector weights(int chain = 0) const {
    Vector w(time_dimension());
    engine()->check(ba_ss_student_get_weights(engine()->get(), chain, w.data()));
    return w;
  }
  void set_weights(const Vector &w, int chain = -1) {   // set_weight, every step (chain -1: every chain)
    if ((int)w.size() != time_dimension()) report_error("One weight per time step is needed.");
    engine()->check(ba_ss_student_set_weights(engine()->get(), chain, w.data()));
  }
  void impute_state() {   // Base::impute_state with the current parameters and weights
    finalize_state();
    engine()->check(ba_ss_student_impute_state(engine()->get()));
  }
  // simulate_forecast(rng, predictors, final_state) for EVERY chain's current draw: column c is
  // chain c's draw of the next predictors.nrow() observations (the chains' forecast streams go on
  // from call to call)
  Matrix simulate_forecast(const Matrix &predictors) {
    if (predictors.ncol() != xdim()) report_error("The forecast predictors do not match the model dimension.");
    Matrix ans(predictors.nrow(), engine()->chains());
    engine()->check(ba_ss_student_forecast(engine()->get(), predictors.nrow(), predictors.data(), ans.data()));
    return ans;
  }
};
// StateSpaceStudentPosteriorSampler(model, observation model sampler's priors): slab, spike,
// siginv prior and nu prior as TRegressionSpikeSlabSampler takes them
class StateSpaceStudentPosteriorSampler : public PosteriorSampler {
 public:
  StateSpaceStudentPosteriorSampler(StateSpaceStudentRegressionModel *model, const Ptr<MvnGivenScalarSigma> &slab,
                                    const Ptr<VariableSelectionPrior> &spike, const Ptr<ChisqModel> &siginv_prior,
                                    const Ptr<DoubleModel> &nu_prior)
      : model_(model), siginv_(siginv_prior) {
    if (slab->dim() != model->xdim()) report_error("Slab does not match model dimension.");
    if ((int)spike->potential_nvars() != model->xdim()) report_error("Spike does not match model dimension.");
    check(ba_sss_set_slab(h(), slab->mu().data(), slab->unscaled_precision().data(), 1, -1));
    check(ba_set_spike(h(), spike->prior_inclusion_probabilities().data(), spike->max_model_size()));
    check(ba_set_sigma_prior(h(), siginv_prior->df(), siginv_prior->sigma(), infinity()));
    check(ba_student_set_nu_prior(h(), nu_prior->kind_, nu_prior->a_, nu_prior->b_));
    std::vector<uint8_t> g0(model->xdim(), 0);
    check(ba_set_state(h(), -1, g0.data(), nullptr, 1.0));
  }
  void draw() override {                     // StateSpacePosteriorSampler.cpp:41-63
    model_->finalize_state();
    check(ba_ss_student_sweep(h(), 1));
    check(ba_sync(h()));
  }
  double logpri() const override { report_error("logpri() is not implemented for the Student-t state space sampler"); return 0; }
  void set_seed(unsigned long s) override { check(ba_seed(h(), s)); }
  void set_sigma_upper_limit(double max_sigma) { check(ba_set_sigma_prior(h(), siginv_->df(), siginv_->sigma(), max_sigma)); }
 private:
  ba_engine *h() const { return model_->engine()->get(); }
  void check(int rc) const { model_->engine()->check(rc); }
  StateSpaceStudentRegressionModel *model_;
  Ptr<ChisqModel> siginv_;
};

// ---- bsts family = "poisson", "logit" ------------------------------------------------------
// What the two latent-data families share: an observed step carries a latent value and its
// precision, the observation model's sampler takes a fixed-precision slab, and sigma^2 stays 1.
// A family is its entry points and the words of its texts.
struct LatentDataFamily {
  int (*sweep)(ba_engine *, int32_t);
  int (*impute_state)(ba_engine *);
  int (*get_latent)(ba_engine *, int64_t, double *, double *);
  int (*set_latent)(ba_engine *, int64_t, const double *, const double *);
  int (*forecast)(ba_engine *, int32_t, const double *, const double *, double *);
  const char *forecast_scale_text;   // a forecast's exposures (trials) of the wrong length
  const char *name;                  // in the sampler's texts
};
inline const LatentDataFamily kPoissonFamily = {
    ba_ss_poisson_sweep, ba_ss_poisson_impute_state, ba_ss_poisson_get_latent, ba_ss_poisson_set_latent,
    ba_ss_poisson_forecast, "One exposure per forecast step is needed.", "Poisson"};
inline const LatentDataFamily kLogitFamily = {
    ba_ss_logit_sweep, ba_ss_logit_impute_state, ba_ss_logit_get_latent, ba_ss_logit_set_latent,
    ba_ss_logit_forecast, "One trial count per forecast step is needed.", "logit"};
// the state of StateSpaceRegressionModel under a latent-data observation model, on the device.
// One observation per time step, regression present.  Chain 0 backs the accessors' defaults.
class StateSpaceLatentDataModel : public StateSpaceRegressionModel {
 public:
  // one chain's latent data (Augmented{Poisson,Binomial}RegressionData::latent_data_value and
  // the precisions behind latent_data_variance); 0 at a missing step
  Vector latent_values(int chain = 0) const { return latent(chain).first; }
  Vector latent_precisions(int chain = 0) const { return latent(chain).second; }
  void set_latent_data(const Vector &value, const Vector &precision, int chain = -1) {   // set_latent_data, every step (chain -1: every chain)
    if ((int)value.size() != time_dimension() || (int)precision.size() != time_dimension())
      report_error("One latent value and one precision per time step are needed.");
    engine()->check(family_.set_latent(engine()->get(), chain, value.data(), precision.data()));
  }
  void impute_state() {   // Base::impute_state with the current parameters and latent data
    finalize_state();
    engine()->check(family_.impute_state(engine()->get()));
  }
  // simulate_forecast(rng, forecast_predictors, exposure or trials, final_state) for EVERY chain's
  // current draw: column c is chain c's draw of the next (success) counts (an empty scale: ones)
  Matrix simulate_forecast(const Matrix &predictors, const Vector &scale = Vector()) {
    if (predictors.ncol() != xdim()) report_error("The forecast predictors do not match the model dimension.");
    if (!scale.empty() && (int)scale.size() != predictors.nrow()) report_error(family_.forecast_scale_text);
    Matrix ans(predictors.nrow(), engine()->chains());
    engine()->check(family_.forecast(engine()->get(), predictors.nrow(), predictors.data(),
                                     scale.empty() ? nullptr : scale.data(), ans.data()));
    return ans;
  }
  const LatentDataFamily &family() const { return family_; }
 protected:
  template <class... Args>   // (args: the family's constructor of StateSpaceRegressionModel)
  StateSpaceLatentDataModel(const LatentDataFamily &family, Args &&...args)
      : StateSpaceRegressionModel(std::forward<Args>(args)...), family_(family) {}
 private:
  std::pair<Vector, Vector> latent(int chain) const {
    Vector v(time_dimension()), q(time_dimension());
    engine()->check(family_.get_latent(engine()->get(), chain, v.data(), q.data()));
    return {v, q};
  }
  const LatentDataFamily &family_;
};
// ... and its sampler: the priors of the observation model's sampler, a fixed-precision slab and a spike
class StateSpaceLatentDataPosteriorSampler : public PosteriorSampler {
 public:
  void draw() override {                     // StateSpacePosteriorSampler.cpp:42-64
    model_->finalize_state();
    check(model_->family().sweep(h(), 1));
    check(ba_sync(h()));
  }
  double logpri() const override {
    report_error(std::string("logpri() is not implemented for the ") + model_->family().name + " state space sampler");
    return 0;
  }
  void set_seed(unsigned long s) override { check(ba_seed(h(), s)); }
  void limit_model_selection(int max_flips) {
    check(ba_sss_set_slab(h(), slab_->mu().data(), slab_->siginv().data(), 0, max_flips));
  }
 protected:
  StateSpaceLatentDataPosteriorSampler(StateSpaceLatentDataModel *model, const Ptr<MvnModel> &slab,
                                       const Ptr<VariableSelectionPrior> &spike)
      : model_(model), slab_(slab) {
    if (slab->dim() != model->xdim()) report_error("Slab does not match model dimension.");
    if ((int)spike->potential_nvars() != model->xdim()) report_error("Spike does not match model dimension.");
    limit_model_selection(-1);
    check(ba_set_spike(h(), spike->prior_inclusion_probabilities().data(), spike->max_model_size()));
    std::vector<uint8_t> g0(model->xdim(), 0);
    check(ba_set_state(h(), -1, g0.data(), nullptr, 1.0));
  }
 private:
  ba_engine *h() const { return model_->engine()->get(); }
  void check(int rc) const { model_->engine()->check(rc); }
  StateSpaceLatentDataModel *model_;
  Ptr<MvnModel> slab_;
};

// StateSpacePoissonModel + StateSpacePoissonPosteriorSampler (Models/StateSpace/
// StateSpacePoissonModel.hpp, PosteriorSamplers/StateSpacePoissonPosteriorSampler.cpp:79-147):
// PoissonRegressionModel's observations (ba_ss_poisson_*).  The mixture table is handed over as
// PoissonRegressionModel's is; slab and spike as PoissonRegressionSpikeSlabSampler takes them.
class StateSpacePoissonModel : public StateSpaceLatentDataModel {
 public:
  StateSpacePoissonModel(const Vector &counts, const Vector &exposure, const Matrix &X,
                         const std::vector<bool> &observed, int chains = 1, uint64_t seed = 8675309, int device = 0)
      : StateSpaceLatentDataModel(kPoissonFamily, PoissonFamily(), counts, exposure, X, observed, chains, seed, device) {}
  void set_mixture_table(const NormalMixtureTable &t) {
    if (t.counts.size() != t.ncomp.size()) report_error("the mixture table's counts and ncomp differ in length");
    engine()->check(ba_poisson_set_mixtures(engine()->get(), (int32_t)t.counts.size(), t.counts.data(), t.ncomp.data(),
                                            t.mu.data(), t.sigma.data(), t.weight.data(), t.largest_index));
  }
};
class StateSpacePoissonPosteriorSampler : public StateSpaceLatentDataPosteriorSampler {
 public:
  StateSpacePoissonPosteriorSampler(StateSpacePoissonModel *model, const Ptr<MvnModel> &slab,
                                    const Ptr<VariableSelectionPrior> &spike)
      : StateSpaceLatentDataPosteriorSampler(model, slab, spike) {}
};

// StateSpaceLogitModel + StateSpaceLogitPosteriorSampler (Models/StateSpace/
// StateSpaceLogitModel.hpp, PosteriorSamplers/StateSpaceLogitPosteriorSampler.cpp:49-123):
// BinomialLogitModel's observations (ba_ss_logit_*); slab and spike as BinomialLogitSpikeSlabSampler
// takes them.
class StateSpaceLogitModel : public StateSpaceLatentDataModel {
 public:
  StateSpaceLogitModel(const Vector &successes, const Vector &trials, const Matrix &X,
                       const std::vector<bool> &observed, int chains = 1, uint64_t seed = 8675309, int device = 0,
                       int clt_threshold = 5)
      : StateSpaceLatentDataModel(kLogitFamily, LogitFamily(), successes, trials, X, observed, clt_threshold, chains, seed,
                                  device) {}
};
class StateSpaceLogitPosteriorSampler : public StateSpaceLatentDataPosteriorSampler {
 public:
  StateSpaceLogitPosteriorSampler(StateSpaceLogitModel *model, const Ptr<MvnModel> &slab,
                                  const Ptr<VariableSelectionPrior> &spike)
      : StateSpaceLatentDataPosteriorSampler(model, slab, spike) {}
};

// ---- Quantile regression spike and slab --------------------------------------------------
// QuantileRegressionModel + QuantileRegressionSpikeSlabSampler (Models/Glm/
// QuantileRegressionModel.hpp, PosteriorSamplers/QuantileRegressionPosteriorSampler.cpp:30-39,
// :77-91; qreg.spike's quantile_spike_wrapper.cc:31-47): the inverse-Gaussian weights and the
// inclusion / coefficient draws at sigma^2 = 1, on the device (ba_quantile_*).  The model is
// built from its dimension and quantile; set_data hands over the observations (the
// reference's add_data, all at once).  Chain 0 backs the model's accessors.
class QuantileRegressionModel : public Model {
 public:
  QuantileRegressionModel(int xdim, double quantile, int chains = 1, uint64_t seed = 8675309, int device = 0)
      : eng_(new Engine(chains, seed, device)), p_(xdim), quantile_(quantile), inc_(xdim, true), beta_(xdim, 0.0) {
    if (xdim <= 0) report_error("The dimension of a QuantileRegressionModel must be positive.");
    if (!(quantile > 0 && quantile < 1)) report_error("Quantile must be strictly between 0 and 1.");
  }
  double quantile() const { return quantile_; }
  void set_data(const Matrix &X, const Vector &y) {
    if (X.nrow() != (int)y.size() || X.ncol() != p_)
      report_error("X and y are incompatible with the QuantileRegressionModel.");
    eng_->check(ba_quantile_set_data(eng_->get(), X.nrow(), X.ncol(), X.data(), y.data(), quantile_));
    dirty_ = true;
  }
  int xdim() const { return p_; }
  const Selector &inc() const { return inc_; }
  void drop_all() { inc_.drop_all(); dirty_ = true; }
  void add(int i) { inc_.add(i); dirty_ = true; }
  void drop(int i) { inc_.drop(i); dirty_ = true; }
  const Vector &Beta() const { return beta_; }
  void set_Beta(const Vector &b) { beta_ = b; dirty_ = true; }
  bool dirty() const { return dirty_; }
  const Ptr<Engine> &engine() const { return eng_; }
  void push_state() {
    eng_->check(ba_set_state(eng_->get(), -1, inc_.bytes().data(), beta_.data(), 1.0));
    dirty_ = false;
  }
  void pull_chain0() {
    eng_->check(ba_get_state(eng_->get(), 0, inc_.bytes().data(), beta_.data(), nullptr));
    dirty_ = false;
  }
 private:
  Ptr<Engine> eng_;
  int p_;
  double quantile_;
  Selector inc_;
  Vector beta_;
  bool dirty_ = true;
};
// QuantileRegressionSpikeSlabSampler(model, slab, spike, seeding_rng); the slab and the
// spike are kept and handed to the engine with the first draw after the data
class QuantileRegressionSpikeSlabSampler : public PosteriorSampler {
 public:
  QuantileRegressionSpikeSlabSampler(QuantileRegressionModel *model, const Ptr<MvnModel> &slab,
                                     const Ptr<VariableSelectionPrior> &spike)
      : model_(model), slab_(slab), spike_(spike) {
    if (slab->dim() != model->xdim()) report_error("Slab does not match model dimension.");
    if ((int)spike->potential_nvars() != model->xdim()) report_error("Spike does not match model dimension.");
  }
  void draw() override {
    if (!priors_set_) {
      check(ba_sss_set_slab(h(), slab_->mu().data(), slab_->siginv().data(), 0, max_flips_));
      check(ba_set_spike(h(), spike_->prior_inclusion_probabilities().data(), spike_->max_model_size()));
      priors_set_ = true;
    }
    if (model_->dirty()) model_->push_state();
    check(ba_quantile_sweep(h(), 1));
    check(ba_sync(h()));
    model_->pull_chain0();
  }
  double logpri() const override { report_error("logpri() is not implemented for the quantile regression sampler"); return 0; }
  void set_seed(unsigned long s) override { check(ba_seed(h(), s)); }
  void limit_model_selection(int max_flips) {
    max_flips_ = max_flips;
    priors_set_ = false;
  }
 private:
  ba_engine *h() const { return model_->engine()->get(); }
  void check(int rc) const { model_->engine()->check(rc); }
  QuantileRegressionModel *model_;
  Ptr<MvnModel> slab_;
  Ptr<VariableSelectionPrior> spike_;
  int max_flips_ = -1;
  bool priors_set_ = false;
};

// ---- Multinomial logit spike and slab ----------------------------------------------------
// MultinomialLogitModel + MLVS (Models/Glm/MultinomialLogitModel.hpp, PosteriorSamplers/MLVS.cpp:
// 71-75, :101-190; mlm.spike's data-augmentation move, proposal.weights = c(DA = 1, 0, 0)): the
// utilities, mixture components and the inclusion / coefficient draws on the device
// (ba_mlogit_*).  The model is built from its dimensions; set_data hands over the responses, the
// subject predictors and the choice predictors (row i Nchoices + m), all at once.  Chain 0
// backs the model's accessors.  Not covered: log_sampling_probs, restricted choice sets, the
// composite sampler's RWM / TIM moves.
//
// The order MLVS::draw_inclusion_vector visits the coefficients in (MLVS.cpp:140-141): the
// shuffle of 0 .. n - 1 by a freshly constructed std::default_random_engine -- the same
// permutation every draw, and the one the caller's own standard library gives their BOOM build.
inline std::vector<int32_t> mlvs_flip_order(int n) {
  std::vector<int32_t> v((size_t)n);
  for (int i = 0; i < n; ++i) v[(size_t)i] = i;
  std::shuffle(v.begin(), v.end(), std::default_random_engine());
  return v;
}
class MultinomialLogitModel : public Model {
 public:
  // (coef() of the reference: the GlmCoefs' inclusion indicators)
  struct Coefs {
    const Selector &inc() const { return inc_; }
    Selector inc_;
  };
  MultinomialLogitModel(int nchoices, int subject_xdim, int choice_xdim, int chains = 1, uint64_t seed = 8675309,
                        int device = 0)
      : eng_(new Engine(chains, seed, device)), M_(nchoices), psub_(subject_xdim), pch_(choice_xdim),
        coef_{Selector((nchoices - 1) * subject_xdim + choice_xdim, true)},
        beta_((size_t)((nchoices - 1) * subject_xdim + choice_xdim), 0.0) {
    if (nchoices < 2) report_error("A MultinomialLogitModel needs at least two choices.");
    if (subject_xdim < 0 || choice_xdim < 0 || beta_size() <= 0)
      report_error("The dimensions of a MultinomialLogitModel must be non-negative and not both zero.");
  }
  int Nchoices() const { return M_; }
  int subject_nvars() const { return psub_; }
  int choice_nvars() const { return pch_; }
  int beta_size() const { return (M_ - 1) * psub_ + pch_; }
  void set_data(const std::vector<int32_t> &y, const Matrix &Xsubject, const Matrix &Xchoice) {
    const int n = (int)y.size();
    if ((psub_ > 0 && (Xsubject.nrow() != n || Xsubject.ncol() != psub_)) ||
        (pch_ > 0 && (Xchoice.nrow() != n * M_ || Xchoice.ncol() != pch_)))
      report_error("The data are incompatible with the MultinomialLogitModel.");
    eng_->check(ba_mlogit_set_data(eng_->get(), n, M_, psub_, pch_, y.data(), psub_ > 0 ? Xsubject.data() : nullptr,
                                   pch_ > 0 ? Xchoice.data() : nullptr));
    dirty_ = true;
    data_set_ = true;
  }
  bool data_set() const { return data_set_; }
  const Coefs &coef() const { return coef_; }
  const Selector &inc() const { return coef_.inc_; }
  void drop_all() { coef_.inc_.drop_all(); dirty_ = true; }
  void add(int i) { coef_.inc_.add(i); dirty_ = true; }
  void drop(int i) { coef_.inc_.drop(i); dirty_ = true; }
  const Vector &beta() const { return beta_; }
  void set_beta(const Vector &b) { beta_ = b; dirty_ = true; }
  bool dirty() const { return dirty_; }
  const Ptr<Engine> &engine() const { return eng_; }
  void push_state() {
    eng_->check(ba_set_state(eng_->get(), -1, coef_.inc_.bytes().data(), beta_.data(), 1.0));
    dirty_ = false;
  }
  void pull_chain0() {
    eng_->check(ba_get_state(eng_->get(), 0, coef_.inc_.bytes().data(), beta_.data(), nullptr));
    dirty_ = false;
  }
 private:
  Ptr<Engine> eng_;
  int M_, psub_, pch_;
  Coefs coef_;
  Vector beta_;
  bool dirty_ = true, data_set_ = false;
};
// MLVS(model, slab, spike); the slab, the spike and the visiting order are handed to the
// engine with the first draw after the data
class MLVS : public PosteriorSampler {
 public:
  MLVS(MultinomialLogitModel *model, const Ptr<MvnModel> &slab, const Ptr<VariableSelectionPrior> &spike)
      : model_(model), slab_(slab), spike_(spike), max_nflips_(model->beta_size()) {
    if (slab->dim() != model->beta_size()) report_error("Slab does not match model dimension.");
    if ((int)spike->potential_nvars() != model->beta_size()) report_error("Spike does not match model dimension.");
  }
  void draw() override {
    if (!priors_set_) {
      // (ba_sss_set_slab limits only if max_flips > 0; limit_model_selection(0) is suppress)
      check(ba_sss_set_slab(h(), slab_->mu().data(), slab_->siginv().data(), 0, max_nflips_ > 0 ? max_nflips_ : -1));
      check(ba_set_spike(h(), spike_->prior_inclusion_probabilities().data(), spike_->max_model_size()));
      const std::vector<int32_t> order = mlvs_flip_order(model_->beta_size());
      check(ba_mlogit_set_flip_order(h(), order.data()));
      check(ba_mlogit_allow_model_selection(h(), (select_ && max_nflips_ > 0) ? 1 : 0));
      priors_set_ = true;
    }
    if (model_->dirty()) model_->push_state();
    check(ba_mlogit_sweep(h(), 1));
    check(ba_sync(h()));
    model_->pull_chain0();
  }
  double logpri() const override { report_error("logpri() is not implemented for the multinomial logit sampler"); return 0; }
  void set_seed(unsigned long s) override { check(ba_seed(h(), s)); }
  void suppress_model_selection() { select_ = false; priors_set_ = false; }
  void allow_model_selection() { select_ = true; priors_set_ = false; }
  void limit_model_selection(unsigned n) { max_nflips_ = (int)n; priors_set_ = false; }
  unsigned max_nflips() const { return (unsigned)max_nflips_; }
 private:
  ba_engine *h() const { return model_->engine()->get(); }
  void check(int rc) const { model_->engine()->check(rc); }
  MultinomialLogitModel *model_;
  Ptr<MvnModel> slab_;
  Ptr<VariableSelectionPrior> spike_;
  int max_nflips_;
  bool select_ = true, priors_set_ = false;
};

}  // namespace boom_amd_api
