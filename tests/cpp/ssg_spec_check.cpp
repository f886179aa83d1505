// Host-only check of boom_amd/csrc/ssg_spec.h, the arithmetic of a list of state models: the table
// of the C-ABI's kinds, the append and its limits, the sampler ids, the scalars ssg_finish derives,
// the template shape, the rule book of refusals and the packed calendars.  The expectations are the
// documented rules (include/boom_amd.h at ba_ss_add_state_model) written out as literals
// or restated here; none is computed with the header's own functions.  Built with
// -fsanitize=address,undefined and run by tests/test_ssg_spec_cpu.py.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../boom_amd/csrc/ssg_spec.h"

using namespace boom_amd;

static int failures = 0, checks = 0;
static void expect(bool ok, const char *what, int a = 0, int b = 0) {
  ++checks;
  if (ok) return;
  std::printf("FAIL %s (%d, %d)\n", what, a, b);
  ++failures;
}

// the refusal texts, as the GPU tests and the header document them
static const char *const SLT_FAMILY = "the Student local linear trend is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)";
static const char *const AUTOAR_FAMILY = "the spike-and-slab autoregression is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)";
static const char *const HOLIDAY_FAMILY = "the random-walk holiday is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)";
static const char *const CALSEAS_FAMILY = "the calendar seasonal is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)";
static const char *const HOLIDAY_STUDENT = "a list that holds both a random-walk holiday and a Student local linear trend is not built";
static const char *const CALSEAS_STUDENT = "a list that holds both a calendar seasonal and a Student local linear trend is not built";
static const char *const LOOKAHEAD = "the look-ahead does not carry a Student local linear trend's weights: use a look-ahead of 1";
static const char *const FORECAST_FAMILY[4] = {nullptr, "forecasts with Student-t observation noise are not implemented",
                                               "forecasts with Poisson observation noise are not implemented",
                                               "forecasts with binomial observation noise are not implemented"};
static const char *const FORECAST_STUDENT_TREND = "forecasts with a Student local linear trend are not implemented";
static const char *const PREDICTION_ERRORS = "one-step prediction errors are built for the Gaussian observation model only";

static bool same(const char *a, const char *b) { return (!a && !b) || (a && b && std::strcmp(a, b) == 0); }

// a list with the host-side initial values it starts from, and valid arguments for every kind
struct List {
  SsgSpec q{};
  double sigsq[SSG_MAX_VAR] = {};
  double phi[SSG_MAX_AR][AR_MAX] = {};
  ArSpikePrior prior[SSG_MAX_AR] = {};
  int nu_kind[2] = {};
  double nu_a[2] = {}, nu_b[2] = {}, nu[2] = {};
  SsFamily family = SS_FAMILY_GAUSSIAN;

  static std::vector<int32_t> default_iparams(int kind) {
    switch (kind) {
      case 3: return {4, 1, 0};
      case 4: return {2};
      case 6: return {2};
      case 7: return {1, 0};
      case 9: return {2, 0, 0, 1};
      case 10: return {3};
      case 11: return {12};
    }
    return {};
  }
  static std::vector<double> default_phi(int kind) {
    switch (kind) {
      case 4: return {0.3, 0.2};
      case 6: return {0.8, 0.6, 0.6, 0.8};
      case 7: return {0.0, 1.0, 0.0, 1.0, 0.1, 0.5};
      case 8: return {0, 1, 500, 0, 1, 500, 10, 10};
      case 9: return {0.3, 0.2, 0, 0, 0.5, 0.5, 1, 0, 0, 1};
    }
    return {};
  }
  SsgRefusal add(int kind, std::vector<int32_t> ip, std::vector<double> ph, double p0 = 1.0, double sigma = 0.5) {
    const double inf = std::numeric_limits<double>::infinity();
    const double df[2] = {1.0, 2.0}, guess[2] = {1.0, 3.0}, upper[2] = {inf, 10.0}, init[2] = {sigma, sigma};
    std::vector<double> mean(SSG_MAX_STATE + 1, 0.25), var(SSG_MAX_STATE + 1, p0);
    const SsgModelArgs args{ip.empty() ? nullptr : ip.data(), df, guess, upper, init, ph.empty() ? nullptr : ph.data(),
                            mean.data(), var.data()};
    return ssg_append(q, SsgInitial{sigsq, phi, prior, nu_kind, nu_a, nu_b, nu}, family, kind, args);
  }
  SsgRefusal add(int kind) { return add(kind, default_iparams(kind), default_phi(kind)); }
  void must(int kind) {
    const SsgRefusal r = add(kind);
    expect(r.code == BA_OK && !r.text, "a valid state model is appended", kind, r.code);
  }
  // a seasonal of dimension `dim`
  void must_dim(int dim) {
    const SsgRefusal r = add(3, {dim + 1, 1, 0}, {});
    expect(r.code == BA_OK, "a seasonal of the dimension is appended", dim, r.code);
  }
};

static void refused(List &l, SsgRefusal r, int code, const char *text, const char *what) {
  const int nblocks = l.q.nblocks, m = l.q.m;
  expect(r.code == code && same(r.text, text), what, r.code, code);
  if (!same(r.text, text)) std::printf("     got: %s\n", r.text ? r.text : "(nothing)");
  expect(l.q.nblocks == nblocks && l.q.m == m, "a refused append leaves the list as it was");
}

// ---- every kind alone ------------------------------------------------------------------------
static void every_kind_alone() {
  struct Row { int kind, dim, nvar, slots, nerr, ar_index, sid0, sid1, stored, holiday, ar_spike, student, phase; };
  const Row rows[11] = {
      {1, 1, 1, 1, 1, -1, 1, 0, 1, 0, 0, 0, 0},   {2, 2, 2, 2, 2, -1, 1, 6, 2, 0, 0, 0, 0},
      {3, 3, 1, 1, 1, -1, 7, 0, 3, 0, 0, 0, 0},   {4, 2, 1, 1, 1, 0, 12, 0, 4, 0, 0, 0, 0},
      {5, 1, 0, 1, 1, -1, 0, 0, 1, 0, 0, 0, 0},   {6, 4, 1, 1, 4, -1, 13, 0, 6, 0, 0, 0, 0},
      {7, 3, 2, 2, 2, 0, 1, 14, 7, 0, 0, 0, 0},   {8, 2, 2, 2, 2, -1, 160, 160, 2, 0, 0, 1, 0},
      {9, 2, 1, 1, 1, 0, 12, 0, 4, 0, 1, 0, 0},   {10, 3, 1, 1, 1, -1, 8, 0, 1, 1, 0, 0, 0},
      {11, 11, 1, 1, 1, -1, 7, 0, 3, 0, 0, 0, -1}};
  for (const Row &r : rows) {
    List l;
    l.must(r.kind);
    const SsgBlock &k = l.q.blk[0];
    expect(l.q.nblocks == 1 && l.q.m == r.dim && k.dim == r.dim && k.first == 0, "dim", r.kind, k.dim);
    expect(k.nvar == r.nvar && l.q.nvar == r.slots && k.var0 == 0, "nvar and slots", r.kind, k.nvar);
    expect(l.q.nerr == r.nerr && k.err0 == 0, "nerr, err0", r.kind, l.q.nerr);
    expect(k.ar_index == r.ar_index && l.q.nar == (r.ar_index >= 0 ? 1 : 0), "ar_index", r.kind, k.ar_index);
    expect(k.nvar < 1 || k.sid[0] == r.sid0, "sid[0]", r.kind, k.sid[0]);
    expect(k.nvar < 2 || k.sid[1] == r.sid1, "sid[1]", r.kind, k.sid[1]);
    expect(k.kind == r.stored, "stored kind", r.kind, k.kind);
    expect(k.holiday == r.holiday && k.ar_spike == r.ar_spike && l.q.student_block == r.student && k.phase == r.phase &&
               k.duration == 1,
           "marks", r.kind);
    expect(l.q.a0[0] == 0.25 && l.q.P0[0] == 1.0, "initial state", r.kind);
    if (r.nvar > 0) {
      // ChisqModel(df = 1, sigma_guess = 1); the second parameter's: (2, 3), upper limit 10
      expect(l.q.prior_df[0] == 1.0 && l.q.prior_ss[0] == 1.0 && std::isinf(l.q.sigma_max[0]) && l.sigsq[0] == 0.25, "prior", r.kind);
      if (r.nvar > 1) expect(l.q.prior_df[1] == 2.0 && l.q.prior_ss[1] == 18.0 && l.q.sigma_max[1] == 10.0 && l.sigsq[1] == 0.25, "second prior", r.kind);
    }
  }
  {  // a static intercept: a slot of its own that is never drawn
    List l;
    l.sigsq[0] = 7.0;
    l.must(5);
    expect(l.q.prior_df[0] == 0.0 && l.q.prior_ss[0] == 0.0 && std::isinf(l.q.sigma_max[0]) && l.q.sigma_max[0] > 0 && l.sigsq[0] == 0.0,
           "a static intercept's slot: variance 0, sigma_max infinite");
    // ... and the two kinds whose initial state variance may be 0
    List z;
    refused(z, z.add(2, {}, {}, 0.0), BA_E_INVALID, "initial state variances must be positive", "a trend's zero initial variance");
    refused(z, z.add(10, {3}, {}, 0.0), BA_E_INVALID, "initial state variances must be positive", "a holiday's zero initial variance");
    expect(z.add(1, {}, {}, 0.0).code == BA_OK && z.add(5, {}, {}, 0.0).code == BA_OK, "a level's and a static intercept's may be 0");
    refused(z, z.add(4, {2}, {0.3, 0.2}, 1.0, 0.0), BA_E_INVALID, "initial sigma must be positive", "an autoregression's initial sigma 0");
    expect(z.add(1, {}, {}, 1.0, 0.0).code == BA_OK, "a level's initial sigma may be 0");
  }
  {  // details of the kinds with parameters of their own
    List l;
    l.must(6);
    expect(l.q.blk[0].nfreq == 2 && l.q.trig_c[0] == 0.8 && l.q.trig_s[1] == 0.6 && l.q.trig_c[2] == 0.6 && l.q.trig_s[3] == 0.8, "trig rotations");
    l.must(7);   // {mu prior 0, 1, phi prior 0, 1, initial mu .1, initial phi .5}
    expect(l.phi[0][0] == 0.5 && l.phi[0][1] == 0.1 && l.q.sl_prior[0][1] == 1.0 && l.q.a0[6] == 0.1 && l.q.P0[6] == 0.0 &&
               l.q.blk[1].sl_truncate == 1 && l.q.blk[1].sl_positive == 0,
           "semilocal: coefficients, priors, the mean component");
    l.must(9);
    expect(l.phi[1][0] == 0.3 && l.phi[1][1] == 0.2 && l.phi[1][2] == 0.0 && l.prior[1].pi[1] == 0.5 && l.prior[1].siginv[AR_MAX + 1] == 1.0 &&
               l.prior[1].select == 1 && l.prior[1].truncate == 0,
           "spike-and-slab autoregression: coefficients and prior by slot");
    List s;
    s.must(8);
    expect(s.nu_kind[0] == 0 && s.nu_a[1] == 1.0 && s.nu_b[0] == 500.0 && s.nu[1] == 10.0, "Student trend: nu priors and initial values");
    // err0 along a list: a trend's two rows, a trig block's every component, one for the level
    List e;
    e.must(2); e.must(6); e.must(1);
    expect(e.q.blk[0].err0 == 0 && e.q.blk[1].err0 == 2 && e.q.blk[2].err0 == 6 && e.q.nerr == 7, "err0 along a list");
    expect(e.q.blk[1].first == 2 && e.q.blk[2].first == 6 && e.q.blk[1].var0 == 2 && e.q.blk[2].var0 == 3, "first and var0 along a list");
  }
}

// ---- the sampler ids in sequence -------------------------------------------------------------
static void sampler_ids() {
  auto ids = [](std::vector<int> kinds, std::vector<std::vector<int>> want, const char *what) {
    List l;
    for (size_t i = 0; i < kinds.size(); ++i) {
      l.must(kinds[i]);
      for (size_t v = 0; v < want[i].size(); ++v) expect(l.q.blk[i].sid[v] == want[i][v], what, (int)i, l.q.blk[i].sid[v]);
      expect(l.q.blk[i].nvar == (int)want[i].size(), "variance parameters", (int)i);
    }
  };
  // the level family counts 1, 17, 33 ...; a slope 6 + 16 per earlier member; a static intercept and a
  // Student trend are no members; a semilocal trend's level is one, its slope counts 14, 30
  ids({1, 1, 2, 7, 5, 8, 1, 7}, {{1}, {17}, {33, 38}, {49, 14}, {}, {160, 160}, {65}, {81, 30}}, "level family");
  // holidays count 8, 24 and are no members of the level family; a calendar seasonal counts with the seasonals
  ids({10, 1, 10, 3, 11, 1, 3, 2}, {{8}, {1}, {24}, {7}, {23}, {17}, {39}, {33, 38}}, "holidays and seasonals");
  // a spike-and-slab autoregression counts with the autoregressions; trig 13, 29
  ids({4, 9, 6, 4, 6, 9, 11, 3}, {{12}, {28}, {13}, {44}, {29}, {60}, {7}, {23}}, "autoregressions and trig");
}

// ---- ld and bl: steps_per_block of tests/test_student_trend_gpu.py, restated ------------------
static void ld_bl_rule(int m, int nerr, int nar, int *ld, int *bl) {
  *ld = m <= 16 ? 17 : (m <= 32 ? 33 : (m <= 60 ? 61 : 65));
  *bl = 64;
  while (*bl > 8 && (2 * *bl * m + m * *ld + *bl * (nerr + 1) + 64 + 8 + nar * 16 * 17) * 8 > 39 * 1024) *bl /= 2;
}
static void ld_and_bl() {
  // one seasonal of dimension m: nerr 1, no autoregression; the literals by hand from the rule
  struct Row { int m, ld, bl; };
  const Row rows[] = {{16, 17, 64}, {17, 33, 64}, {29, 33, 64}, {30, 33, 32}, {32, 33, 32}, {33, 61, 32}, {38, 61, 32}, {39, 61, 16},
                      {52, 61, 16}, {53, 61, 8},  {60, 61, 8},  {61, 65, 8},  {64, 65, 8}};
  for (const Row &r : rows) {
    List l;
    l.must_dim(r.m);
    int ld = 0, bl = 0;
    ld_bl_rule(r.m, 1, 0, &ld, &bl);
    expect(ld == r.ld && bl == r.bl, "the restated rule gives the literals", r.m, bl);
    expect(l.q.ld == r.ld && l.q.bl == r.bl, "ld, bl", l.q.ld, l.q.bl);
  }
  // the state-error rows and the autoregression slots count: a trig block of 14 frequencies, four autoregressions of 13 lags
  List t;
  expect(t.add(6, {14}, std::vector<double>(28, 0.5)).code == BA_OK, "trig of 14 frequencies");
  int ld = 0, bl = 0;
  ld_bl_rule(28, 28, 0, &ld, &bl);
  expect(t.q.nerr == 28 && t.q.ld == ld && t.q.bl == bl && bl == 32, "ld, bl with a state-error row per component", t.q.ld, t.q.bl);
  List a;
  for (int i = 0; i < 4; ++i) expect(a.add(4, {13}, {}).code == BA_OK, "autoregression of 13 lags");
  ld_bl_rule(52, 4, 4, &ld, &bl);
  expect(a.q.m == 52 && a.q.nar == 4 && a.q.ld == ld && a.q.bl == bl && bl == 8, "ld, bl with four autoregression slots", a.q.ld, a.q.bl);
  ld_bl_rule(52, 4, 0, &ld, &bl);
  expect(bl == 16, "(without the slots the same dimension keeps sixteen steps)", bl);
}

// ---- the limits --------------------------------------------------------------------------------
static void limits() {
  {
    List l;
    for (int i = 0; i < 8; ++i) l.must(1);
    refused(l, l.add(1), BA_E_INVALID, "more than 8 state models", "the 9th block");
  }
  {
    List l;
    l.must_dim(64);
    refused(l, l.add(1), BA_E_INVALID, "state dimension exceeds 64", "m = 65");
    List t;
    refused(t, t.add(6, {33}, std::vector<double>(66, 0.5)), BA_E_INVALID, "state dimension exceeds 64", "33 frequencies");
    refused(t, t.add(6, {0}, {0.5}), BA_E_INVALID, "At least one frequency needed to initialize TrigStateModel.", "no frequency");
  }
  {
    // (eight blocks of two parameters are sixteen: the 17th is out of the C-ABI's reach and is
    // reached here by a list that says it holds fifteen)
    List l;
    for (int i = 0; i < 7; ++i) l.must(2);
    l.q.nvar = 15;
    refused(l, l.add(2), BA_E_INVALID, "more than 16 variance parameters", "the 17th variance");
    expect(l.add(1).code == BA_OK && l.q.nvar == 16, "the 16th is taken");
  }
  {
    List l;
    for (int i = 0; i < 3; ++i) l.must(4);
    l.must(7);
    refused(l, l.add(4), BA_E_INVALID, "more than 4 autoregression state models", "the 5th autoregression slot");
    refused(l, l.add(9), BA_E_INVALID, "more than 4 autoregression state models", "the 5th autoregression slot, spike and slab");
    refused(l, l.add(7), BA_E_INVALID, "more than 4 autoregression / semilocal state models", "the 5th slot, semilocal");
  }
  List l;
  refused(l, l.add(4, {17}, {}), BA_E_INVALID, "more than 16 lags", "17 lags");
  refused(l, l.add(4, {0}, {}), BA_E_INVALID, "lags must be positive", "no lag");
  refused(l, l.add(3, {1, 1, 0}, {}), BA_E_INVALID, "nseasons must be at least 2", "nseasons 1");
  refused(l, l.add(11, {1}, {}), BA_E_INVALID, "nseasons must be at least 2", "nseasons 1, calendar");
  refused(l, l.add(3, {4, 0, 0}, {}), BA_E_INVALID, "season_duration must be positive", "duration 0");
  refused(l, l.add(3, {4, 65536, 0}, {}), BA_E_INVALID, "season_duration exceeds 65535", "duration 65 536");
  expect(l.add(3, {4, 65535, 0}, {}).code == BA_OK && l.q.blk[0].duration == 65535, "duration 65 535 is taken");
  refused(l, l.add(10, {0}, {}), BA_E_INVALID, "a random-walk holiday's width must lie in [1, 63]", "width 0");
  refused(l, l.add(10, {64}, {}), BA_E_INVALID, "a random-walk holiday's width must lie in [1, 63]", "width 64");
  refused(l, l.add(4, {1}, {1.1}), BA_E_INVALID, "the initial autoregression coefficients are not stationary", "phi = 1.1");
  refused(l, l.add(4, {2}, {0.6, 0.5}), BA_E_INVALID, "the initial autoregression coefficients are not stationary", "phi = (.6, .5)");
  expect(l.add(4, {2}, {1.2, -0.5}).code == BA_OK, "phi = (1.2, -.5) is stationary");
  refused(l, l.add(9, {2, 1, 0, 1}, {0.6, 0.5, 0, 0, 0.5, 0.5, 1, 0, 0, 1}), BA_E_INVALID,
          "the initial autoregression coefficients are not stationary", "spike and slab, truncated, phi = (.6, .5)");
  expect(l.add(9, {2, 0, 0, 1}, {0.6, 0.5, 0, 0, 0.5, 0.5, 1, 0, 0, 1}).code == BA_OK, "... taken when the sampler does not truncate");
  refused(l, l.add(9, {2, 0, 0, 1}, {0.1, 0.1, 0, 0, 0.5, 0.5, 1, 2, 2, 1}), BA_E_INVALID,
          "the slab's precision must be symmetric positive definite", "an indefinite slab precision");
  refused(l, l.add(9, {2, 0, 0, 1}, {0.1, 0.1, 0, 0, 0.5, 1.5, 1, 0, 0, 1}), BA_E_INVALID,
          "prior inclusion probabilities must lie in [0, 1]", "an inclusion probability of 1.5");
  refused(l, l.add(12), BA_E_INVALID,
          "state model kind must be 1 (local level), 2 (local linear trend), 3 (seasonal), 4 (autoregression), 5 (static intercept), 6 (trig), 7 (semilocal linear trend), 8 (Student local linear trend), 9 (spike-and-slab autoregression), 10 (random-walk holiday) or 11 (calendar seasonal)",
          "kind 12");
  refused(l, l.add(3, {}, {}), BA_E_INVALID, "null argument", "a seasonal without iparams");
  refused(l, l.add(8, {}, {}), BA_E_INVALID, "null argument", "a Student trend without initial_phi");
  l.must(8);
  refused(l, l.add(8), BA_E_INVALID, "at most one Student local linear trend per list of state models", "a second Student trend");
  refused(l, l.add(7, {0, 1}, List::default_phi(7)), BA_E_INVALID,
          "force_ar1_positive without force_stationary (a one-sided truncation of the slope's AR(1) coefficient) is not built",
          "force_ar1_positive alone");
  {
    List s;
    refused(s, s.add(8, {}, {0, 1, 500, 0, 1, 500, 10, 600}), BA_E_INVALID, "the initial nu must be positive and have positive prior density", "nu outside its uniform prior");
    refused(s, s.add(8, {}, {2, 1, 500, 0, 1, 500, 10, 10}), BA_E_INVALID, "nu prior kind must be 0 (uniform) or 1 (gamma)", "prior kind 2");
  }
  // new_season(t): the phase normalised into [0, duration)
  const int phases[][2] = {{-1, 2}, {-3, 0}, {7, 1}, {2, 2}, {-4, 2}};
  for (const auto &ph : phases) {
    List s;
    expect(s.add(3, {4, 3, ph[0]}, {}).code == BA_OK && s.q.blk[0].phase == ph[1] && s.q.blk[0].duration == 3, "phase", ph[0], s.q.blk[0].phase);
  }
}

// ---- the template shape ----------------------------------------------------------------------
static void template_shape() {
  auto shape = [](List &l, int tr, int ns, int lags, const char *what) {
    int32_t a = -1, b = -1, c = -1;
    ssg_template_shape(l.q, &a, &b, &c);
    expect(a == tr && b == ns && c == lags, what, a, b);
  };
  { List l; l.must(1); shape(l, 1, 0, 0, "[level]"); }
  { List l; l.must(2); l.must(3); l.must(4); shape(l, 2, 4, 2, "[trend, seasonal, autoregression]"); }
  { List l; l.must(1); l.must_dim(15); shape(l, 1, 16, 0, "m = 16"); }
  { List l; l.must(1); l.must_dim(16); shape(l, 0, 0, 0, "m = 17"); }
  { List l; l.must(1); expect(l.add(3, {4, 2, 0}, {}).code == BA_OK, "duration 2"); shape(l, 0, 0, 0, "duration 2"); }
  { List l; l.must(5); shape(l, 0, 0, 0, "[static intercept]"); }
  { List l; l.must(1); l.must(5); shape(l, 0, 0, 0, "[level, static intercept]"); }
  { List l; l.must(1); l.must(9); shape(l, 0, 0, 0, "a spike-and-slab autoregression"); }
  { List l; l.must(1); l.must(10); shape(l, 0, 0, 0, "a holiday"); }
  { List l; l.must(10); shape(l, 0, 0, 0, "[holiday]"); }
  { List l; l.must(1); l.must(11); shape(l, 0, 0, 0, "a calendar seasonal"); }
  { List l; l.must(8); shape(l, 0, 0, 0, "[Student trend]"); }
  { List l; l.must(1); l.must(3); l.must(4); l.must(1); shape(l, 0, 0, 0, "four blocks"); }
  { List l; l.must(1); l.must(4); l.must(3); shape(l, 0, 0, 0, "autoregression before seasonal"); }
  { List l; l.must(3); shape(l, 0, 0, 0, "[seasonal]"); }
  { List l; shape(l, 0, 0, 0, "no block"); }
}

// ---- the rule book ---------------------------------------------------------------------------
static void rule_book() {
  const int specials[4] = {8, 9, 10, 11};
  const char *const family_text[4] = {SLT_FAMILY, AUTOAR_FAMILY, HOLIDAY_FAMILY, CALSEAS_FAMILY};
  const SsFamily families[4] = {SS_FAMILY_GAUSSIAN, SS_FAMILY_STUDENT, SS_FAMILY_POISSON, SS_FAMILY_LOGIT};
  auto cell = [](const SsgSpec *q, SsFamily f, SsgUse use, const char *want, const char *what, int kind = 0) {
    const char *got = ssg_refusal(q, f, use, kind);
    expect(same(got, want), what, (int)f, (int)use);
    if (!same(got, want)) std::printf("     got: %s\n", got ? got : "(nothing)");
  };
  for (int fi = 0; fi < 4; ++fi) {
    const SsFamily f = families[fi];
    const bool other = fi != 0;
    // no list, and a list of plain blocks: only the family's own refusals
    List plain;
    plain.must(1); plain.must(3); plain.must(4);
    for (const SsgSpec *q : {(const SsgSpec *)nullptr, (const SsgSpec *)&plain.q}) {
      for (int kind = 1; kind <= 7; ++kind) cell(q, f, SSG_USE_APPEND, nullptr, "a plain kind is appended under every family", kind);
      cell(q, f, SSG_USE_LAUNCH, nullptr, "plain list: launch");
      cell(q, f, SSG_USE_LOOKAHEAD, nullptr, "plain list: look-ahead");
      cell(q, f, SSG_USE_FORECAST, FORECAST_FAMILY[fi], "plain list: forecast");
      cell(q, f, SSG_USE_PREDICTION_ERRORS, other ? PREDICTION_ERRORS : nullptr, "plain list: prediction errors");
    }
    for (int si = 0; si < 4; ++si) {
      // the append, through ssg_append: to an empty list and behind a level
      for (int behind = 0; behind < 2; ++behind) {
        List l;
        l.family = f;
        if (behind) l.must(1);
        const SsgRefusal r = l.add(specials[si]);
        if (other) refused(l, r, BA_E_STATE, family_text[si], "a special block under a family");
        else expect(r.code == BA_OK && !r.text, "a special block under the Gaussian model", specials[si]);
      }
      // a list that holds it (built under the Gaussian model), under each family
      List l;
      l.must(1);
      l.must(specials[si]);
      cell(&l.q, f, SSG_USE_LAUNCH, other ? family_text[si] : nullptr, "launch");
      cell(&l.q, f, SSG_USE_LOOKAHEAD, si == 0 ? LOOKAHEAD : nullptr, "look-ahead above 1");
      cell(&l.q, f, SSG_USE_FORECAST, other ? FORECAST_FAMILY[fi] : (si == 0 ? FORECAST_STUDENT_TREND : nullptr), "forecast");
      cell(&l.q, f, SSG_USE_PREDICTION_ERRORS, other ? PREDICTION_ERRORS : nullptr, "prediction errors");
    }
    if (!other) continue;
    // the order at a launch: Student trend, spike-and-slab autoregression, holiday, calendar seasonal --
    // whatever the order of the blocks
    const int pairs[][3] = {{9, 10, 1}, {10, 9, 1}, {10, 11, 2}, {11, 10, 2}, {8, 9, 0}, {9, 8, 0}, {11, 9, 1}};
    for (const auto &pr : pairs) {
      List l;
      l.must(pr[0]);
      l.must(pr[1]);
      cell(&l.q, f, SSG_USE_LAUNCH, family_text[pr[2]], "launch: the first refusal of two");
    }
  }
  // a Student trend with a holiday or a calendar seasonal, in both orders of appending
  for (int fi = 0; fi < 4; ++fi) {
    const SsFamily f = families[fi];
    const int cal[2] = {10, 11};
    const char *const both[2] = {HOLIDAY_STUDENT, CALSEAS_STUDENT};
    const char *const fam[2] = {HOLIDAY_FAMILY, CALSEAS_FAMILY};
    for (int ci = 0; ci < 2; ++ci) {
      List a;   // the calendar block first (a list built under the Gaussian model)
      a.must(cal[ci]);
      a.family = f;
      refused(a, a.add(8), BA_E_STATE, both[ci], "a Student trend behind a calendar block: the list's refusal before the family's");
      List b;   // the Student trend first
      b.must(8);
      b.family = f;
      refused(b, b.add(cal[ci]), BA_E_STATE, fi ? fam[ci] : both[ci], "a calendar block behind a Student trend: the family's refusal first");
    }
    List c;   // both calendar kinds in the list: the holiday's text
    c.must(11);
    c.must(10);
    c.family = f;
    refused(c, c.add(8), BA_E_STATE, HOLIDAY_STUDENT, "a Student trend behind both calendar kinds");
  }
  {  // argument checks come before the rule book, the rule book before the prior's and nu's validation
    List l;
    l.family = SS_FAMILY_LOGIT;
    refused(l, l.add(10, {0}, {}), BA_E_INVALID, "a random-walk holiday's width must lie in [1, 63]", "width before family");
    refused(l, l.add(11, {1}, {}), BA_E_INVALID, "nseasons must be at least 2", "nseasons before family");
    refused(l, l.add(9, {17, 0, 0, 1}, List::default_phi(9)), BA_E_INVALID, "more than 16 lags", "lags before family");
    refused(l, l.add(9, {2, 0, 0, 1}, {0.1, 0.1, 0, 0, 0.5, 1.5, 1, 0, 0, 1}), BA_E_STATE, AUTOAR_FAMILY, "family before the slab's validation");
    refused(l, l.add(8, {}, {2, 1, 500, 0, 1, 500, 10, 10}), BA_E_STATE, SLT_FAMILY, "family before the nu priors' validation");
  }
}

// ---- the packed calendars --------------------------------------------------------------------
static void calendars() {
  // holidays of widths 1 and 3 in blocks 0 and 2, a calendar seasonal in block 1; T = 5
  List l;
  expect(l.add(10, {1}, {}).code == BA_OK && l.add(11, {3}, {}).code == BA_OK && l.add(10, {3}, {}).code == BA_OK, "the list");
  std::vector<int32_t> hol[SSG_MAX_BLOCKS];
  std::vector<uint8_t> seas[SSG_MAX_BLOCKS];
  hol[0] = {-1, 0, -1, -1, 0, 0};
  seas[1] = {1, 0, 1, 1, 0};   // (entry 0 is not read)
  hol[2] = {0, 1, 2, -1, -1, 0, 1};
  const int64_t count = ssg_calendar_count(l.q, hol, seas);
  expect(count == 5, "count: the shortest calendar", (int)count);
  expect(ssg_calendar_words(l.q, 5) == 5 + (3 * 5 + 1) / 2, "words: count + (nblocks count + 1) / 2", (int)ssg_calendar_words(l.q, 5));
  const std::vector<uint64_t> packed = ssg_pack_calendars(l.q, hol, seas, 5);
  expect(packed.size() == 13, "packed size", (int)packed.size());
  // byte 0: the first holiday's position or 0x80; byte 1: 0x80 with the season bit at entries >= 1;
  // byte 2: the second holiday's; bytes 3 .. 7: 0x80
  const uint64_t want[5] = {0x8080808080008080ull, 0x8080808080018000ull, 0x8080808080028180ull, 0x8080808080808180ull,
                            0x8080808080808000ull};
  for (int t = 0; t < 5 && t < (int)packed.size(); ++t) expect(packed[t] == want[t], "table entry", t, (int)(packed[t] & 0xffffff));
  if (packed.size() == 13) {
    int32_t rows[16];
    std::memcpy(rows, packed.data() + 5, sizeof rows);
    const int32_t want_rows[16] = {0, 0, 0, 0, 0, /* block 1 */ 0, 0, 1, 2, 2, 0, 0, 0, 0, 0, /* padding */ 0};
    for (int i = 0; i < 16; ++i) expect(rows[i] == want_rows[i], "prefix counts", i, rows[i]);
  }
  // holidays only: the table and no prefix rows; a block that is no calendar block keeps 0x80
  List h;
  h.must(1);
  expect(h.add(10, {2}, {}).code == BA_OK, "[level, holiday]");
  std::vector<int32_t> hol2[SSG_MAX_BLOCKS];
  hol2[1] = {1, -1, 0};
  hol2[0] = {0, 0};   // (a calendar the list has no block for is not read)
  expect(ssg_calendar_count(h.q, hol2, seas) == 3 && ssg_calendar_words(h.q, 3) == 3, "holidays only: no prefix rows");
  const std::vector<uint64_t> p2 = ssg_pack_calendars(h.q, hol2, seas, 3);
  expect(p2.size() == 3 && p2[0] == 0x8080808080800180ull && p2[1] == 0x8080808080808080ull && p2[2] == 0x8080808080800080ull,
         "holidays only: the table");
  List none;
  none.must(1);
  expect(ssg_calendar_count(none.q, hol2, seas) == -1, "no calendar block");
}

int main() {
  every_kind_alone();
  sampler_ids();
  ld_and_bl();
  limits();
  template_shape();
  rule_book();
  calendars();
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
