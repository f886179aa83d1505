// Host-only check of the AR dynamic regression's part of boom_amd/csrc/ssg_spec.h and ssg_instances.h
// (ssg_append_dynreg_ar; include/boom_amd.h at ba_ss_add_dynamic_regression_ar): the blocks'
// dimensions, columns, slots and sampler ids, what the launch of the DR instance is sized by at xdim = 4,
// lags = 16, the predictor table, and every refusal with its text.  The expectations are the documented
// rules written out as literals.  Built with -fsanitize=address,undefined (dynreg_ar.mk) and run by
// tests/test_ss_dynreg_ar_cpu.py.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../boom_amd/csrc/ssg_instances.h"
#include "../../boom_amd/csrc/ssg_spec.h"

using namespace boom_amd;

static int failures = 0, checks = 0;
static void expect(bool ok, const char *what, int a = 0, int b = 0) {
  ++checks;
  if (ok) return;
  std::printf("FAIL %s (%d, %d)\n", what, a, b);
  ++failures;
}
static bool same(const char *a, const char *b) { return (!a && !b) || (a && b && std::strcmp(a, b) == 0); }

static const char *const DYNREG_FAMILY = "the dynamic regression is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)";
static const char *const DYNREG_STUDENT = "a list that holds both a dynamic regression and a Student local linear trend is not built";
static const char *const DYNREG_HOLIDAY = "a list that holds both a dynamic regression and a random-walk holiday is not built";
static const char *const DYNREG_CALSEAS = "a list that holds both a dynamic regression and a calendar seasonal is not built";
static const char *const FIFTH_SLOT = "more than 4 autoregression state models";

struct List {
  SsgSpec q{};
  double sigsq[SSG_MAX_VAR] = {};
  double phi[SSG_MAX_AR][AR_MAX] = {};
  ArSpikePrior prior[SSG_MAX_AR] = {};
  int nu_kind[2] = {};
  double nu_a[2] = {}, nu_b[2] = {}, nu[2] = {};
  SsFamily family = SS_FAMILY_GAUSSIAN;
  SsgInitial initial() { return SsgInitial{sigsq, phi, prior, nu_kind, nu_a, nu_b, nu}; }

  SsgRefusal add(int kind, std::vector<int32_t> ip = {}, std::vector<double> ph = {}) {
    const double inf = std::numeric_limits<double>::infinity();
    const double df[2] = {1.0, 2.0}, guess[2] = {1.0, 3.0}, upper[2] = {inf, 10.0}, init[2] = {0.5, 0.5};
    std::vector<double> mean(SSG_MAX_STATE + 1, 0.25), var(SSG_MAX_STATE + 1, 1.0);
    const SsgModelArgs args{ip.empty() ? nullptr : ip.data(), df, guess, upper, init, ph.empty() ? nullptr : ph.data(),
                            mean.data(), var.data()};
    return ssg_append(q, initial(), family, kind, args);
  }
  // a plain dynamic regression of d coefficients
  SsgRefusal dyn(int d) {
    std::vector<double> df(d, 1.0), guess(d, 2.0), upper(d, 10.0), init(d, 0.1), mean(d, 0.25), var(d, 1.0);
    const SsgModelArgs args{nullptr, df.data(), guess.data(), upper.data(), init.data(), nullptr, mean.data(), var.data()};
    return ssg_append_dynreg(q, initial(), family, d, args);
  }
  // an AR dynamic regression: coefficient i has df i + 1, guess 2, upper 10 + i, sigma 0.1 (i + 1) unless given,
  // phi_i = (0.1 (i + 1), 0, ..) unless `ph` is given (xdim x lags), state mean 0.25 + i, variance p0
  SsgRefusal dynar(int xdim, int lags, std::vector<double> ph = {}, bool with_phi = true, double p0 = 1.0, double upper0 = 10.0, double sigma0 = 0.1) {
    const int n = xdim > 0 ? xdim : 1, L = lags > 0 ? lags : 1;
    std::vector<double> df(n), guess(n, 2.0), upper(n), init(n), mean((size_t)n * L), var((size_t)n * L, p0);
    if (ph.empty()) ph.assign((size_t)n * L, 0.0);
    for (int i = 0; i < n; ++i) {
      df[i] = i + 1; upper[i] = upper0 + i; init[i] = sigma0 * (i + 1);
      if (ph.size() == (size_t)n * L && ph[(size_t)i * L] == 0.0) ph[(size_t)i * L] = 0.1 * (i + 1);
      for (int j = 0; j < L; ++j) mean[(size_t)i * L + j] = 0.25 + i;
    }
    const SsgModelArgs args{nullptr, df.data(), guess.data(), upper.data(), init.data(), with_phi ? ph.data() : nullptr, mean.data(), var.data()};
    return ssg_append_dynreg_ar(q, initial(), family, xdim, lags, args);
  }
};

static void refused(const SsgRefusal &r, int code, const char *text, const char *what) {
  expect(r.code == code && same(r.text, text), what, r.code, 0);
  if (!(r.code == code && same(r.text, text))) std::printf("  got: %s\n", r.text ? r.text : "(appended)");
}

static void blocks_and_ids() {
  // [plain d = 2 | kind 4, 3 lags | AR dynamic regression xdim = 2, lags = 3 | level]
  List l;
  expect(l.dyn(2).code == BA_OK && l.add(4, {3}, {0.3, 0.2, 0.1}).code == BA_OK && l.dynar(2, 3).code == BA_OK && l.add(1).code == BA_OK, "the list");
  expect(l.q.nblocks == 5 && l.q.m == 2 + 3 + 6 + 1 && l.q.nvar == 2 + 1 + 2 + 1 && l.q.nar == 3 && l.q.nerr == 2 + 1 + 2 + 1, "m, nvar, nar, nerr", l.q.m, l.q.nerr);
  for (int i = 0; i < 2; ++i) {
    const SsgBlock &k = l.q.blk[2 + i];
    expect(k.kind == SSG_AR && k.dim == 3 && k.lags == 3 && k.nvar == 1, "a block per coefficient: an autoregression of `lags` components", i, k.dim);
    expect(k.first == 5 + 3 * i && k.var0 == 3 + i && k.err0 == 3 + i && k.ar_index == 1 + i, "first, var0, err0, autoregression slot", k.first, k.ar_index);
    expect(k.dynreg == 3 + i, "1 + its column of the table: behind the plain block's two", k.dynreg);
    expect(k.sid[0] == 12 + 16 * (1 + i), "the AR family's sampler id: 12 + 16 per earlier autoregression", k.sid[0]);
    expect(!k.ar_spike && !k.holiday && k.duration == 1, "no other mark");
    expect(ssg_abi_kind(l.q, 2 + i) == SSG_DYNAMIC_REGRESSION_AR && SSG_DYNAMIC_REGRESSION_AR == 14, "ssg_abi_kind: 14");
    const SsgKind &r = ssg_row_of(l.q, 2 + i);
    expect(r.stored == SSG_AR && r.nvar == 1 && r.nslot == 1 && r.nerr == 1 && r.ar_slot && r.member == SSG_FAM_AR && r.sampler[0].base == 12, "its row is kind 4's");
    expect(l.q.prior_df[3 + i] == i + 1 && l.q.prior_ss[3 + i] == (i + 1) * 4.0 && l.q.sigma_max[3 + i] == 10 + i, "priors by slot", i);
    expect(l.sigsq[3 + i] == (0.1 * (i + 1)) * (0.1 * (i + 1)), "the initial variances by slot", i);
    expect(l.phi[1 + i][0] == 0.1 * (i + 1) && l.phi[1 + i][1] == 0.0 && l.phi[1 + i][3] == 0.0, "phi by autoregression slot", i);
    for (int j = 0; j < 3; ++j) expect(l.q.a0[5 + 3 * i + j] == 0.25 + i && l.q.P0[5 + 3 * i + j] == 1.0, "a0, P0 by component", i, j);
  }
  expect(ssg_abi_kind(l.q, 0) == 12 && ssg_abi_kind(l.q, 1) == 4 && ssg_abi_kind(l.q, 4) == 1, "the other blocks keep their kinds");
  expect(l.q.blk[1].sid[0] == 12 && l.q.blk[4].sid[0] == 1 && l.q.blk[0].sid[0] == 10, "... and their sampler ids");
  expect(ssg_dyn_columns(l.q) == 4 && ssg_dyn_columns(l.q, 3) == 3 && ssg_dyn_columns(l.q, 1) == 2, "a column per block, not per component");
  expect(ssg_dyn_width(l.q.blk[0]) == 2 && ssg_dyn_width(l.q.blk[1]) == 0 && ssg_dyn_width(l.q.blk[2]) == 1, "ssg_dyn_width");
  expect(ssg_has(l.q, SSG_HAS_DYNREG) && !ssg_has(l.q, SSG_HAS_AR_SPIKE | SSG_HAS_CALENDAR | SSG_HAS_STUDENT_TREND), "the feature bit");
  // an autoregression after the model counts it in its family
  List t;
  expect(t.dynar(2, 2).code == BA_OK && t.add(4, {2}, {0.3, 0.2}).code == BA_OK && t.q.blk[2].sid[0] == 12 + 32 && t.q.blk[2].ar_index == 2, "kind 4 behind it: id 44, slot 2", t.q.blk[2].sid[0]);
  expect(t.q.blk[0].sid[0] == 12 && t.q.blk[1].sid[0] == 28 && t.q.blk[0].dynreg == 1 && t.q.blk[1].dynreg == 2, "ids 12, 28; columns 0, 1");
  // [level, xdim = 1, lags = 2] has the template's shape of blocks but not its kernel
  List one;
  int32_t tr = -1, ns = -1, lags = -1;
  expect(one.add(1).code == BA_OK && one.dynar(1, 2).code == BA_OK, "[level, xdim = 1]");
  ssg_template_shape(one.q, &tr, &ns, &lags);
  expect(tr == 0 && ns == 0 && lags == 0, "no template kernel", tr, lags);
  // a null initial_phi: zeros
  List z;
  z.phi[0][0] = z.phi[1][1] = 7.0;
  expect(z.dynar(2, 2, {}, false).code == BA_OK && z.phi[0][0] == 0.0 && z.phi[0][1] == 0.0 && z.phi[1][0] == 0.0 && z.phi[1][1] == 0.0, "initial_phi == NULL: zeros");
}

// ssg_finish's rule and ssg_pass_lds_doubles (ssg_simsmooth.h) restated
static int bl_rule(int m, int ld, int nerr, int nar, int ndyn) {
  int bl = 64;
  while (bl > 8 && (2 * bl * m + m * ld + bl * (nerr + 1) + 64 + 8 + nar * 16 * 17 + 2 * bl * ndyn) * 8 > 39 * 1024) bl /= 2;
  return bl;
}
static int lds_doubles(int m, int ld, int bl, int nerr, int nar, int ndyn) {
  return 2 * bl * m + m * ld + (bl * (nerr + 1) + 64 + 8) + nar * 16 * 17 + 2 * bl * ndyn;
}
static void launch_at_the_limit() {
  // xdim = 4, lags = 16: m = 64, all four autoregression slots, four columns
  List l;
  expect(l.dynar(4, 16).code == BA_OK, "xdim = 4, lags = 16");
  expect(l.q.m == 64 && l.q.nblocks == 4 && l.q.nar == 4 && l.q.nvar == 4 && l.q.nerr == 4 && l.q.ld == 65, "m = 64: LDC 65", l.q.m, l.q.ld);
  expect(ssg_dyn_columns(l.q) == 4, "four columns");
  // P (64 x 65) + the autoregressions' rows (4 x 272) + the fixed part (72) = 5320 doubles pass the 4992 of
  // four workgroups a CU before any step: bl falls to its floor of 8
  expect(l.q.bl == 8 && bl_rule(64, 65, 4, 4, 4) == 8, "8 steps per time block", l.q.bl);
  // 2 x 8 x 64 + 64 x 65 + (8 x 5 + 72) + 4 x 272 + 2 x 8 x 4 = 1024 + 4160 + 112 + 1088 + 64 doubles
  const int doubles = lds_doubles(l.q.m, l.q.ld, l.q.bl, l.q.nerr, l.q.nar, ssg_dyn_columns(l.q));
  expect(doubles == 6448 && doubles * 8 == 51584, "51 584 bytes of dynamic LDS", doubles);
  expect(doubles * 8 <= 65536 && 3 * doubles * 8 <= 160 * 1024, "under 64 KB (no attribute to raise), three workgroups a CU");
  // (the staging buffers start behind the autoregressions' rows and end with the allocation)
  const int sdyn0 = 2 * 8 * 64 + 64 * 65 + (8 * 5 + 72) + 4 * 272;
  expect(sdyn0 + 2 * l.q.bl * 4 == doubles, "the two staging buffers are the allocation's tail", sdyn0);
  // the instance: DR, by the table alone
  SsParams P{};
  double table[4] = {};
  P.T = 1;
  P.dyn = table; P.dyn_rows = 1; P.dyn_cols = 4;
  P.ssm.ndyn = ssg_dyn_columns(l.q);
  SsgChoice c = ssg_choose_kernel(P);
  expect(c.kernel == SSG_CHOICE_GENERAL && c.variant == SSG_V_DR, "ssg_choose_kernel: DR");
  P.ssm.tpl_trend = 1;
  c = ssg_choose_kernel(P);
  expect(c.kernel == SSG_CHOICE_GENERAL && c.variant == SSG_V_DR, "... whatever the template's shape says");
  P.dyn_cols = 64;   // (a column per component would be the plain form's count)
  expect(ssg_choose_kernel(P).kernel == SSG_CHOICE_INVALID, "a table of another width is refused");
}

static void limits() {
  List l;
  refused(l.dynar(0, 2), BA_E_INVALID, "a dynamic regression needs at least one predictor", "xdim = 0");
  refused(l.dynar(-1, 2), BA_E_INVALID, "a dynamic regression needs at least one predictor", "xdim = -1");
  refused(l.dynar(1, 0), BA_E_INVALID, "lags must be positive", "lags = 0");
  refused(l.dynar(1, 17), BA_E_INVALID, "more than 16 lags", "lags = 17");
  refused(l.dynar(5, 1), BA_E_INVALID, FIFTH_SLOT, "xdim = 5: a fifth autoregression slot");
  refused(l.dynar(9, 1), BA_E_INVALID, "more than 8 state models", "xdim = 9");
  expect(l.q.nblocks == 0, "nothing appended");
  expect(l.dynar(4, 16).code == BA_OK && l.q.m == 64, "xdim = 4, lags = 16 fills the state");
  refused(l.dynar(1, 1), BA_E_INVALID, FIFTH_SLOT, "a fifth slot behind four");
  refused(l.add(4, {1}, {0.5}), BA_E_INVALID, FIFTH_SLOT, "kind 4 behind four");
  refused(l.add(7, {1, 0}, {0, 1, 0, 1, 0, 0}), BA_E_INVALID, "more than 4 autoregression / semilocal state models", "a semilocal trend behind four");
  // the slots other models took
  List a;
  expect(a.add(4, {2}, {0.3, 0.2}).code == BA_OK && a.add(7, {1, 0}, {0, 1, 0, 1, 0, 0}).code == BA_OK, "an autoregression and a semilocal trend: two slots");
  refused(a.dynar(3, 2), BA_E_INVALID, FIFTH_SLOT, "2 + 3 slots");
  expect(a.q.nblocks == 2 && a.q.nar == 2 && a.q.m == 5, "all or none: the list is as it was", a.q.nblocks, a.q.m);
  expect(a.dynar(2, 2).code == BA_OK && a.q.nar == 4 && a.q.nblocks == 4, "2 + 2 slots");
  // the state dimension
  List s;
  expect(s.add(3, {50, 1, 0}).code == BA_OK, "49 seasonal components");
  refused(s.dynar(2, 8), BA_E_INVALID, "state dimension exceeds 64", "49 + 16");
  expect(s.dynar(3, 5).code == BA_OK && s.q.m == 64, "49 + 15");
  // the blocks
  List b;
  for (int i = 0; i < 6; ++i) expect(b.add(1).code == BA_OK, "six levels");
  refused(b.dynar(3, 1), BA_E_INVALID, "more than 8 state models", "6 + 3 blocks");
  expect(b.dynar(2, 1).code == BA_OK && b.q.nblocks == 8, "6 + 2 blocks");
  // the variance slots
  List v;
  for (int i = 0; i < 7; ++i) expect(v.add(2).code == BA_OK, "seven trends: 14 slots");
  expect(v.q.nblocks == 7 && v.q.nvar == 14, "14 slots in 7 blocks");
  List w;
  expect(w.dyn(14).code == BA_OK, "a plain dynamic regression of 14: 14 slots in one block");
  refused(w.dynar(3, 1), BA_E_INVALID, "more than 16 variance parameters", "14 + 3 slots");
  expect(w.q.nblocks == 1 && w.q.nvar == 14 && w.q.nar == 0 && w.q.m == 14 && ssg_dyn_columns(w.q) == 14, "all or none: two blocks went in and came out again", w.q.nblocks, w.q.nvar);
  expect(w.dynar(2, 1).code == BA_OK && w.q.nvar == 16 && w.q.blk[1].dynreg == 15 && w.q.blk[2].dynreg == 16, "14 + 2 slots; columns 14, 15");
  // the arrays
  List p;
  refused(p.dynar(2, 2, {}, true, 0.0), BA_E_INVALID, "initial state variances must be positive", "P0 = 0");
  refused(p.dynar(2, 2, {}, true, 1.0, -1.0), BA_E_INVALID, "sigma_max must be non-negative.", "a negative upper limit");
  refused(p.dynar(2, 2, {}, true, 1.0, 10.0, 0.0), BA_E_INVALID, "initial sigma must be positive", "sigma = 0: as kind 4");
  refused(p.dynar(2, 2, {0.5, 0.2, 0.7, 0.6}), BA_E_INVALID, "the initial autoregression coefficients are not stationary", "the second row is not stationary");
  expect(p.q.nblocks == 0 && p.q.m == 0 && p.q.nar == 0 && p.q.nvar == 0, "all or none: the first coefficient's block is taken back");
  refused(p.dynar(1, 2, {0.5, 0.5}), BA_E_INVALID, "the initial autoregression coefficients are not stationary", "a unit root");
  {
    double x[4] = {1, 1, 1, 1};
    const SsgModelArgs args{nullptr, x, x, x, nullptr, nullptr, x, x};
    refused(ssg_append_dynreg_ar(p.q, p.initial(), p.family, 2, 2, args), BA_E_INVALID, "null argument", "a null array");
  }
  expect(p.dynar(2, 2, {0.5, 0.2, 0.7, 0.2}).code == BA_OK && p.phi[1][0] == 0.7 && p.phi[1][1] == 0.2, "stationary rows are taken");
}

static void rule_book() {
  for (SsFamily f : {SS_FAMILY_STUDENT, SS_FAMILY_POISSON, SS_FAMILY_LOGIT}) {
    List l;
    l.family = f;
    refused(l.dynar(2, 2), BA_E_STATE, DYNREG_FAMILY, "appended under another family");
    List g;
    expect(g.add(1).code == BA_OK && g.dynar(2, 2).code == BA_OK, "[level, xdim = 2]");
    expect(same(ssg_refusal(&g.q, f, SSG_USE_LAUNCH), DYNREG_FAMILY), "launched under another family");
  }
  struct Pair { int kind; std::vector<int32_t> ip; std::vector<double> ph; const char *text; };
  const Pair pairs[] = {{8, {}, {0, 1, 500, 0, 1, 500, 10, 10}, DYNREG_STUDENT}, {10, {3}, {}, DYNREG_HOLIDAY}, {11, {12}, {}, DYNREG_CALSEAS}};
  for (const Pair &pr : pairs) {
    List a;
    expect(a.add(pr.kind, pr.ip, pr.ph).code == BA_OK, "the other block first", pr.kind);
    refused(a.dynar(2, 2), BA_E_STATE, pr.text, "... then the AR dynamic regression");
    expect(a.q.nblocks == 1, "the list is as it was");
    List b;
    expect(b.dynar(2, 2).code == BA_OK, "the AR dynamic regression first");
    refused(b.add(pr.kind, pr.ip, pr.ph), BA_E_STATE, pr.text, "... then the other block");
    expect(b.q.nblocks == 2, "the list is as it was");
  }
  // what goes with it: the plain form among them
  List ok;
  expect(ok.add(1).code == BA_OK && ok.add(2).code == BA_OK && ok.add(3, {7, 1, 0}).code == BA_OK && ok.add(5).code == BA_OK &&
             ok.add(6, {1}, {0.8, 0.6}).code == BA_OK && ok.dyn(2).code == BA_OK && ok.dynar(1, 2).code == BA_OK &&
             ok.add(9, {2, 0, 0, 1}, {0.3, 0.2, 0, 0, 0.5, 0.5, 1, 0, 0, 1}).code == BA_OK,
         "level, trend, seasonal, static intercept, trig, plain dynamic regression, spike-and-slab autoregression beside it");
  expect(ssg_refusal(&ok.q, SS_FAMILY_GAUSSIAN, SSG_USE_LAUNCH) == nullptr && ssg_refusal(&ok.q, SS_FAMILY_GAUSSIAN, SSG_USE_LOOKAHEAD) == nullptr &&
             ssg_refusal(&ok.q, SS_FAMILY_GAUSSIAN, SSG_USE_FORECAST) == nullptr &&
             ssg_refusal(&ok.q, SS_FAMILY_GAUSSIAN, SSG_USE_PREDICTION_ERRORS) == nullptr,
         "launch, look-ahead, forecast and prediction errors serve it");
  expect(same(ssg_refusal(&ok.q, SS_FAMILY_GAUSSIAN, SSG_USE_LOOKAHEAD, 0, 1), "the look-ahead does not carry a regression holiday's coefficients: use a look-ahead of 1"),
         "a regression holiday beside it: as beside the plain form");
}

static void predictor_table() {
  // [plain d = 2 | level | xdim = 2]: the model's blocks keep a column each
  List l;
  expect(l.dyn(2).code == BA_OK && l.add(1).code == BA_OK && l.dynar(2, 3).code == BA_OK, "[d = 2, level, xdim = 2]");
  std::vector<double> x[SSG_MAX_BLOCKS];
  x[0] = {1, 2, 3, 4, 5, 6, 7, 8};   // four rows of two
  x[2] = {-1, -2, -3};               // three rows of one
  x[3] = {10, 20, 30, 40};           // four rows of one
  expect(ssg_dyn_rows(l.q, x) == 3, "the shortest block's rows");
  const std::vector<double> t = ssg_pack_predictors(l.q, x, 3);
  const double want[12] = {1, 2, -1, 10, 3, 4, -2, 20, 5, 6, -3, 30};
  expect(t.size() == 12, "rows x columns");
  for (int i = 0; i < 12 && i < (int)t.size(); ++i) expect(t[i] == want[i], "the table, row-major, a column per coefficient", i);
}

int main() {
  blocks_and_ids();
  launch_at_the_limit();
  limits();
  rule_book();
  predictor_table();
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
