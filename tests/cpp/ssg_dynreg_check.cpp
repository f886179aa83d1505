// Host-only check of the dynamic regression's part of boom_amd/csrc/ssg_spec.h: the block's row and
// sampler ids, the append's limits and every refusal text, the predictor table, and that bl of a list
// without such a block is what it was.  The expectations are the documented rules (include/boom_amd.h at
// ba_ss_add_dynamic_regression) written out as literals or restated here.  Built with
// -fsanitize=address,undefined and run by tests/test_ssg_dynreg_cpu.py.
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
static bool same(const char *a, const char *b) { return (!a && !b) || (a && b && std::strcmp(a, b) == 0); }

static const char *const DYNREG_FAMILY = "the dynamic regression is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)";
static const char *const DYNREG_STUDENT = "a list that holds both a dynamic regression and a Student local linear trend is not built";
static const char *const DYNREG_HOLIDAY = "a list that holds both a dynamic regression and a random-walk holiday is not built";
static const char *const DYNREG_CALSEAS = "a list that holds both a dynamic regression and a calendar seasonal is not built";
static const char *const KIND_TEXT =
    "state model kind must be 1 (local level), 2 (local linear trend), 3 (seasonal), 4 (autoregression), 5 (static intercept), 6 (trig), 7 (semilocal linear trend), 8 (Student local linear trend), 9 (spike-and-slab autoregression), 10 (random-walk holiday) or 11 (calendar seasonal)";

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
  // a dynamic regression of d coefficients: df i + 1, guess 2, upper 10 + i, sigma 0.1 i (the first is 0)
  SsgRefusal dyn(int d, double p0 = 1.0, double upper0 = 10.0) {
    const int n = d > 0 ? d : 1;
    std::vector<double> df(n), guess(n, 2.0), upper(n), init(n), mean(n, 0.25), var(n, p0);
    for (int i = 0; i < n; ++i) { df[i] = i + 1; upper[i] = upper0 + i; init[i] = 0.1 * i; }
    const SsgModelArgs args{nullptr, df.data(), guess.data(), upper.data(), init.data(), nullptr, mean.data(), var.data()};
    return ssg_append_dynreg(q, initial(), family, d, args);
  }
};

static void refused(const SsgRefusal &r, int code, const char *text, const char *what) {
  expect(r.code == code && same(r.text, text), what, r.code, 0);
  if (!(r.code == code && same(r.text, text))) std::printf("  got: %s\n", r.text ? r.text : "(appended)");
}

static void row_and_ids() {
  List l;
  expect(l.dyn(3).code == BA_OK && l.add(1).code == BA_OK && l.dyn(2).code == BA_OK, "[d = 3, level, d = 2]");
  const SsgBlock &a = l.q.blk[0], &b = l.q.blk[2];
  expect(a.kind == SSG_LOCAL_LEVEL && a.dim == 3 && a.nvar == 3 && a.first == 0 && a.var0 == 0 && a.dynreg == 1 && a.err0 == 0,
         "the first block: a local level of dimension 3, columns from 0", a.dim, a.dynreg);
  expect(b.kind == SSG_LOCAL_LEVEL && b.dim == 2 && b.nvar == 2 && b.first == 4 && b.var0 == 4 && b.dynreg == 4 && b.err0 == 4,
         "the second block: columns from 3", b.first, b.dynreg);
  expect(!a.holiday && !a.ar_spike && a.ar_index == -1, "no other mark");
  expect(l.q.m == 6 && l.q.nvar == 6 && l.q.nerr == 6 && l.q.nar == 0, "m, nvar, nerr", l.q.m, l.q.nerr);
  // sampler ids: two blocks of d = 3 and 2 read 10, 26, 42 and 58, 74; a level between them keeps 1
  expect(a.sid[0] == 10 && b.sid[0] == 58 && l.q.blk[1].sid[0] == 1, "sid[0]", a.sid[0], b.sid[0]);
  const int want[5] = {10, 26, 42, 58, 74};
  for (int i = 0; i < 3; ++i) expect(a.sid[0] + 16 * i == want[i], "slot ids of the first block", i);
  for (int i = 0; i < 2; ++i) expect(b.sid[0] + 16 * i == want[3 + i], "slot ids of the second block", i);
  expect(ssg_abi_kind(l.q, 0) == 12 && ssg_abi_kind(l.q, 1) == 1 && ssg_abi_kind(l.q, 2) == 12, "ssg_abi_kind");
  const SsgKind &r = ssg_row_of(l.q, 2);
  expect(r.stored == SSG_LOCAL_LEVEL && r.dim == 2 && r.nvar == 2 && r.nslot == 2 && r.nerr == 0 && !r.ar_slot && !r.sigma_positive &&
             !r.zero_p0 && r.member == 0 && r.sampler[0].base == 10,
         "the block's row");
  expect(ssg_row_of(l.q, 0).dim == 3 && ssg_row_of(l.q, 0).nslot == 3, "... of the block's own dimension");
  expect(ssg_kind_row(12) == nullptr, "ssg_kind_row(12) stays out of the table");
  refused(l.add(12), BA_E_INVALID, KIND_TEXT, "ssg_append(kind 12) is refused as before");
  // priors and initial values by slot
  expect(l.q.prior_df[0] == 1 && l.q.prior_df[2] == 3 && l.q.prior_df[4] == 1 && l.q.prior_df[5] == 2, "prior df by slot");
  expect(l.q.prior_ss[1] == 2 * 4.0 && l.q.sigma_max[2] == 12 && l.q.sigma_max[5] == 11, "prior ss, sigma max by slot");
  expect(l.sigsq[0] == 0.0 && l.sigsq[2] == 0.2 * 0.2 && l.sigsq[5] == 0.1 * 0.1, "sigma may start at 0");
  expect(l.q.a0[5] == 0.25 && l.q.P0[0] == 1.0, "a0, P0");
  expect(ssg_dyn_columns(l.q) == 5 && ssg_dyn_columns(l.q, 2) == 3, "the table's columns");
  int32_t tr = -1, ns = -1, lags = -1;
  ssg_template_shape(l.q, &tr, &ns, &lags);
  expect(tr == 0 && ns == 0 && lags == 0, "no template");
  List one;
  expect(one.add(1).code == BA_OK && one.dyn(1).code == BA_OK, "[level, d = 1]");
  ssg_template_shape(one.q, &tr, &ns, &lags);
  expect(tr == 0, "no template for [level, d = 1] either");
  expect(ssg_has(one.q, SSG_HAS_DYNREG) && !ssg_has(one.q, SSG_HAS_CALENDAR | SSG_HAS_STUDENT_TREND | SSG_HAS_AR_SPIKE), "the feature bit");
}

static void limits() {
  List l;
  refused(l.dyn(0), BA_E_INVALID, "a dynamic regression needs at least one predictor", "d = 0");
  refused(l.dyn(-3), BA_E_INVALID, "a dynamic regression needs at least one predictor", "d = -3");
  refused(l.dyn(65), BA_E_INVALID, "state dimension exceeds 64", "d = 65");
  refused(l.dyn(17), BA_E_INVALID, "more than 16 variance parameters", "d = 17");
  expect(l.dyn(16).code == BA_OK && l.q.m == 16 && l.q.nvar == 16 && l.q.ld == 17, "d = 16 alone: SMALL at its edge", l.q.m, l.q.ld);
  expect(l.q.blk[0].sid[0] + 16 * 15 == 250, "the largest id is 250");
  refused(l.dyn(1), BA_E_INVALID, "more than 16 variance parameters", "a 17th slot");
  List s;
  expect(s.add(3, {50, 1, 0}).code == BA_OK, "49 seasonal components");
  expect(s.dyn(15).code == BA_OK && s.q.m == 64, "q.m + d = 64");
  refused(s.dyn(1), BA_E_INVALID, "state dimension exceeds 64", "q.m + d = 65");
  List v;
  for (int i = 0; i < 7; ++i) expect(v.add(2).code == BA_OK, "seven trends: 14 slots");
  refused(v.dyn(3), BA_E_INVALID, "more than 16 variance parameters", "q.nvar + d = 17");
  expect(v.dyn(2).code == BA_OK && v.q.nvar == 16 && v.q.nblocks == 8, "q.nvar + d = 16");
  refused(v.dyn(1), BA_E_INVALID, "more than 8 state models", "a ninth block");
  List p;
  refused(p.dyn(2, 0.0), BA_E_INVALID, "initial state variances must be positive", "P0 = 0");
  refused(p.dyn(2, -1.0), BA_E_INVALID, "initial state variances must be positive", "P0 < 0");
  refused(p.dyn(2, 1.0, -1.0), BA_E_INVALID, "sigma_max must be non-negative.", "a negative upper limit");
  {
    double x[2] = {1, 1};
    const SsgModelArgs args{nullptr, x, x, x, nullptr, nullptr, x, x};
    refused(ssg_append_dynreg(p.q, p.initial(), p.family, 2, args), BA_E_INVALID, "null argument", "a null array");
  }
  expect(p.q.nblocks == 0 && p.q.m == 0, "a refused append leaves the list alone");
}

static void rule_book() {
  // the three families, the block added on such data ...
  for (SsFamily f : {SS_FAMILY_STUDENT, SS_FAMILY_POISSON, SS_FAMILY_LOGIT}) {
    List l;
    l.family = f;
    refused(l.dyn(2), BA_E_STATE, DYNREG_FAMILY, "appended under another family");
    // ... and the list first, the family's launch after it
    List g;
    expect(g.add(1).code == BA_OK && g.dyn(2).code == BA_OK, "[level, d = 2]");
    expect(same(ssg_refusal(&g.q, f, SSG_USE_LAUNCH), DYNREG_FAMILY), "launched under another family");
  }
  // a Student trend, a holiday, a calendar seasonal: in both orders
  struct Pair { int kind; std::vector<int32_t> ip; std::vector<double> ph; const char *text; };
  const Pair pairs[] = {{8, {}, {0, 1, 500, 0, 1, 500, 10, 10}, DYNREG_STUDENT}, {10, {3}, {}, DYNREG_HOLIDAY}, {11, {12}, {}, DYNREG_CALSEAS}};
  for (const Pair &pr : pairs) {
    List a;
    expect(a.add(pr.kind, pr.ip, pr.ph).code == BA_OK, "the other block first", pr.kind);
    refused(a.dyn(2), BA_E_STATE, pr.text, "... then the dynamic regression");
    expect(a.q.nblocks == 1, "the list is as it was");
    List b;
    expect(b.dyn(2).code == BA_OK, "the dynamic regression first");
    refused(b.add(pr.kind, pr.ip, pr.ph), BA_E_STATE, pr.text, "... then the other block");
    expect(b.q.nblocks == 1, "the list is as it was");
  }
  // what goes with it
  List ok;
  expect(ok.add(1).code == BA_OK && ok.add(2).code == BA_OK && ok.add(3, {7, 1, 0}).code == BA_OK && ok.add(4, {2}, {0.3, 0.2}).code == BA_OK &&
             ok.add(5).code == BA_OK && ok.add(6, {1}, {0.8, 0.6}).code == BA_OK && ok.add(9, {2, 0, 0, 1}, {0.3, 0.2, 0, 0, 0.5, 0.5, 1, 0, 0, 1}).code == BA_OK &&
             ok.dyn(2).code == BA_OK,
         "level, trend, seasonal, autoregression, static intercept, trig, spike-and-slab autoregression beside it");
  expect(ssg_refusal(&ok.q, SS_FAMILY_GAUSSIAN, SSG_USE_LAUNCH) == nullptr && ssg_refusal(&ok.q, SS_FAMILY_GAUSSIAN, SSG_USE_LOOKAHEAD) == nullptr &&
             ssg_refusal(&ok.q, SS_FAMILY_GAUSSIAN, SSG_USE_FORECAST) == nullptr &&
             ssg_refusal(&ok.q, SS_FAMILY_GAUSSIAN, SSG_USE_PREDICTION_ERRORS) == nullptr,
         "launch, look-ahead, forecast and prediction errors serve it");
}

// bl: the rule of ssg_finish restated, with the predictors' staging buffers (2 x bl x columns)
static int bl_rule(int m, int ld, int nerr, int nar, int ndyn) {
  int bl = 64;
  while (bl > 8 && (2 * bl * m + m * ld + bl * (nerr + 1) + 64 + 8 + nar * 16 * 17 + 2 * bl * ndyn) * 8 > 39 * 1024) bl /= 2;
  return bl;
}
static void ld_and_bl() {
  // lists without such a block: the literals of tests/cpp/ssg_spec_check.cpp (one seasonal of dimension m)
  struct Row { int m, ld, bl; };
  const Row rows[] = {{16, 17, 64}, {17, 33, 64}, {29, 33, 64}, {30, 33, 32}, {32, 33, 32}, {33, 61, 32}, {38, 61, 32}, {39, 61, 16},
                      {52, 61, 16}, {53, 61, 8},  {60, 61, 8},  {61, 65, 8},  {64, 65, 8}};
  for (const Row &r : rows) {
    List l;
    expect(l.add(3, {r.m + 1, 1, 0}).code == BA_OK && l.q.ld == r.ld && l.q.bl == r.bl, "ld, bl without a dynamic block", r.m, l.q.bl);
    expect(bl_rule(r.m, r.ld, 1, 0, 0) == r.bl, "the restated rule gives the literals", r.m);
  }
  List a;
  for (int i = 0; i < 4; ++i) expect(a.add(4, {13}).code == BA_OK, "autoregression of 13 lags");
  expect(a.q.bl == 8 && a.q.ld == 61, "four autoregression slots: bl 8 as before", a.q.bl);
  // with one: the staging buffers count.  12 seasons + d = 10: m = 21, nerr = 11 -- 4221 doubles at 64
  // steps without the buffers, 5501 with them (the limit is 4992): 64 steps without, 32 with
  List d;
  expect(d.add(3, {12, 1, 0}).code == BA_OK && d.dyn(10).code == BA_OK, "[12 seasons, d = 10]");
  expect(bl_rule(21, 33, 11, 0, 0) == 64 && bl_rule(21, 33, 11, 0, 10) == 32, "the restated rule: 64 without, 32 with");
  expect(d.q.m == 21 && d.q.nerr == 11 && d.q.ld == 33 && d.q.bl == 32, "bl counts the predictors' staging", d.q.m, d.q.bl);
  // the lists of the GPU test keep 64 steps, but for d = 16 alone (5528 doubles at 64 steps: 32)
  List s;
  expect(s.add(1).code == BA_OK && s.add(3, {4, 1, 0}).code == BA_OK && s.dyn(3).code == BA_OK && s.q.bl == 64 && s.q.ld == 17, "level + 4 seasons + d = 3");
  List e;
  expect(e.dyn(16).code == BA_OK && e.q.bl == 32 && e.q.bl == bl_rule(16, 17, 16, 0, 16), "d = 16 alone", e.q.bl);
  List t;
  expect(t.add(3, {20, 1, 0}).code == BA_OK && t.dyn(3).code == BA_OK && t.q.bl == 64 && t.q.ld == 33, "20 seasons + d = 3");
}

static void predictor_table() {
  List l;
  expect(l.dyn(2).code == BA_OK && l.add(1).code == BA_OK && l.dyn(1).code == BA_OK, "[d = 2, level, d = 1]");
  std::vector<double> x[SSG_MAX_BLOCKS];
  x[0] = {1, 2, 3, 4, 5, 6, 7, 8};   // four rows of two
  x[2] = {-1, -2, -3};               // three rows of one
  x[1] = {9, 9};                     // (predictors the list has no block for are not read)
  expect(ssg_dyn_rows(l.q, x) == 3, "the shortest block's rows");
  const std::vector<double> t = ssg_pack_predictors(l.q, x, 3);
  const double want[9] = {1, 2, -1, 3, 4, -2, 5, 6, -3};
  expect(t.size() == 9, "rows x columns");
  for (int i = 0; i < 9 && i < (int)t.size(); ++i) expect(t[i] == want[i], "the table, row-major, state order", i);
  List none;
  expect(none.add(1).code == BA_OK && ssg_dyn_rows(none.q, x) == -1 && ssg_dyn_columns(none.q) == 0, "no dynamic block");
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double fin[4] = {1, -2, 0, 4}, bad1[4] = {1, 2, inf, 4}, bad2[4] = {1, 2, 3, nan};
  expect(ssg_dyn_check(fin, 2, 2) == -1 && ssg_dyn_check(bad1, 2, 2) == 2 && ssg_dyn_check(bad2, 2, 2) == 3, "predictors must be finite");
}

int main() {
  row_and_ids();
  limits();
  rule_book();
  ld_and_bl();
  predictor_table();
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
