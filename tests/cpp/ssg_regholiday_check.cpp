// Host-only check of the regression holiday's host arithmetic (boom_amd/csrc/ssg_regholiday.h), its row
// of the rule book (ssg_refusal, ssg_spec.h) and the kernel choice of a launch that carries a series per
// chain (ssg_choose_kernel, ssg_instances.h): the packing of the shared table, the active steps and the
// counts, every refusal and its text, and that the choice is never the template kernel.  The expectations
// are the documented rules (include/boom_amd.h at ba_ss_add_regression_holiday) written
// out as literals.  Built with -fsanitize=address,undefined and run by tests/test_ssg_regholiday_cpu.py.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../boom_amd/csrc/ssg_instances.h"
#include "../../boom_amd/csrc/ssg_regholiday.h"
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

static const char *const FAMILY = "the regression holiday is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)";
static const char *const LOOKAHEAD = "the look-ahead does not carry a regression holiday's coefficients: use a look-ahead of 1";

static RhModel model(std::vector<int32_t> widths, std::vector<int32_t> calendar) {
  RhModel m;
  m.widths = widths;
  m.initial.assign((size_t)m.ncoef(), 0.0);
  m.calendar = calendar;
  return m;
}

int main() {
  // ---- the arguments of an add
  {
    std::vector<RhModel> none;
    const int32_t w[3] = {3, 2, 1}, w0[2] = {3, 0};
    const double c[6] = {0, 1, 2, 3, 4, 5};
    double bad[6] = {0, 1, 2, 3, 4, 5};
    bad[4] = 1.0 / 0.0;
    expect(rh_add_refusal(none, true, 3, w, 0.0, 1.0, nullptr) == nullptr, "a plain add");
    expect(rh_add_refusal(none, true, 3, w, 0.5, 2.0, c) == nullptr, "an add with coefficients");
    expect(same(rh_add_refusal(none, true, 3, nullptr, 0.0, 1.0, nullptr), "null argument"), "null widths");
    expect(same(rh_add_refusal(none, true, 0, w, 0.0, 1.0, nullptr), "a regression holiday model needs at least one holiday"), "no holiday");
    expect(same(rh_add_refusal(none, false, 3, w, 0.0, 1.0, nullptr),
                "a regression holiday model goes on a list of state models: add a state model first"), "no state model");
    expect(same(rh_add_refusal(none, true, 2, w0, 0.0, 1.0, nullptr), "a holiday's width must be at least 1"), "width 0");
    expect(same(rh_add_refusal(none, true, 3, w, 0.0 / 0.0, 1.0, nullptr), "the prior mean must be finite"), "prior mean");
    for (double sd : {0.0, -1.0, 1.0 / 0.0, 0.0 / 0.0})
      expect(same(rh_add_refusal(none, true, 3, w, 0.0, sd, nullptr), "the prior standard deviation must be positive and finite"), "prior sd");
    expect(same(rh_add_refusal(none, true, 3, w, 0.0, 1.0, bad), "the initial coefficients must be finite"), "coefficients");
    // the limits: 4 models, 256 coefficients together
    std::vector<RhModel> four(4, model({1}, {}));
    expect(same(rh_add_refusal(four, true, 3, w, 0.0, 1.0, nullptr), "more than 4 regression holiday models"), "a fifth model");
    std::vector<RhModel> big(1, model({250}, {}));
    const int32_t w6[1] = {6}, w7[1] = {7}, w300[1] = {300};
    expect(rh_add_refusal(big, true, 1, w6, 0.0, 1.0, nullptr) == nullptr, "256 coefficients");
    expect(same(rh_add_refusal(big, true, 1, w7, 0.0, 1.0, nullptr), "more than 256 regression holiday coefficients"), "257 coefficients");
    expect(same(rh_add_refusal(none, true, 1, w300, 0.0, 1.0, nullptr), "more than 256 regression holiday coefficients"), "a width of 300");
  }
  // ---- a calendar's entries
  {
    const int32_t ok[5] = {-1, 0, 5, -1, 3}, low[3] = {0, -2, 1}, high[3] = {0, 1, 6};
    expect(rh_calendar_check(ok, 5, 6) == -1, "entries in {-1} u [0, 6)");
    expect(rh_calendar_check(low, 3, 6) == 1, "an entry below -1");
    expect(rh_calendar_check(high, 3, 6) == 2, "an entry past the coefficients");
  }
  // ---- the calendars against a launch and a forecast
  {
    std::vector<RhModel> ms{model({2}, std::vector<int32_t>(12, -1)), model({1}, std::vector<int32_t>(10, -1))};
    int code = -1;
    expect(rh_launch_refusal(ms, 10, 0, &code).empty(), "calendars that cover the series");
    expect(rh_launch_refusal(ms, 11, 0, &code) == "the calendar of regression holiday model 1 has 10 entries, the series has 11 time points" &&
               code == BA_E_STATE, "a calendar shorter than the series", code);
    expect(rh_launch_refusal(ms, 10, 2, &code) ==
                   "the calendar of regression holiday model 1 has 10 entries: a forecast of horizon 2 needs 12 (the series' 10 and the horizon)" &&
               code == BA_E_INVALID, "a calendar shorter than T + horizon", code);
    ms[0].calendar.clear();
    expect(rh_launch_refusal(ms, 10, 0, &code) == "regression holiday model 0 has no calendar: call ba_ss_set_regression_holiday_calendar first" &&
               code == BA_E_STATE, "no calendar", code);
  }
  // ---- the packing: T = 6, model 0 of widths (2, 1), model 1 of width 2; t = 2 is missing
  {
    //                                  t:  0   1   2   3   4   5 | 6   7
    std::vector<RhModel> ms{model({2, 1}, {0, 1, 0, -1, -1, 0, 2, -1}), model({2}, {-1, 1, 1, -1, -1, -1, 0})};
    const uint8_t obs[6] = {1, 1, 0, 1, 1, 1};
    const RhPacked K = rh_pack(ms, 6, obs);
    expect(K.count == 7, "the table has the shortest calendar's entries", (int)K.count);
    expect(K.first[0] == 0 && K.first[1] == 3 && K.first[2] == 5 && K.first[3] == 5 && K.first[4] == 5, "the models' first coefficients");
    expect(K.table.size() == 7 * RH_MAX_MODELS, "the table's size");
    const int32_t want[7][2] = {{0, -1}, {1, 4}, {0, 4}, {-1, -1}, {-1, -1}, {0, -1}, {2, 3}};
    for (int t = 0; t < 7; ++t) {
      expect(K.table[t * RH_MAX_MODELS] == want[t][0] && K.table[t * RH_MAX_MODELS + 1] == want[t][1], "a table entry", t);
      expect(K.table[t * RH_MAX_MODELS + 2] == -1 && K.table[t * RH_MAX_MODELS + 3] == -1, "no third or fourth model", t);
    }
    expect(K.steps == std::vector<int32_t>({0, 1, 2, 5}), "the active steps of [0, T), ascending (a missing day is one)");
    // coefficient 0: t = 0, 5 (t = 2 is missing); 1: t = 1; 2: active past T only; model 1: 3 never, 4: t = 1 (t = 2 is missing)
    expect(K.counts == std::vector<double>({2.0, 1.0, 0.0, 0.0, 1.0}), "the counts");
    const RhPacked all = rh_pack(ms, 6, nullptr);
    expect(all.counts == std::vector<double>({3.0, 1.0, 0.0, 0.0, 2.0}), "the counts with every step observed");
  }
  // ---- the rule book's row
  {
    SsgSpec q{};
    const SsFamily others[3] = {SS_FAMILY_STUDENT, SS_FAMILY_POISSON, SS_FAMILY_LOGIT};
    expect(ssg_refusal(&q, SS_FAMILY_GAUSSIAN, SSG_USE_APPEND, SSG_REGRESSION_HOLIDAY) == nullptr, "Gaussian: appended");
    expect(ssg_refusal(&q, SS_FAMILY_GAUSSIAN, SSG_USE_LAUNCH, 0, 2) == nullptr, "Gaussian: launched");
    for (SsFamily f : others) {
      expect(same(ssg_refusal(&q, f, SSG_USE_APPEND, SSG_REGRESSION_HOLIDAY), FAMILY), "family first, then the model", (int)f);
      expect(same(ssg_refusal(&q, f, SSG_USE_LAUNCH, 0, 1), FAMILY), "the model first, then the family's launch", (int)f);
      expect(ssg_refusal(&q, f, SSG_USE_LAUNCH, 0, 0) == nullptr, "a list without the model", (int)f);
    }
    expect(same(ssg_refusal(&q, SS_FAMILY_GAUSSIAN, SSG_USE_LOOKAHEAD, 0, 1), LOOKAHEAD), "a look-ahead above 1");
    expect(ssg_refusal(&q, SS_FAMILY_GAUSSIAN, SSG_USE_LOOKAHEAD, 0, 0) == nullptr, "a look-ahead without the model");
    expect(ssg_refusal(&q, SS_FAMILY_GAUSSIAN, SSG_USE_FORECAST, 0, 1) == nullptr, "the forecast is built");
    expect(ssg_refusal(&q, SS_FAMILY_GAUSSIAN, SSG_USE_PREDICTION_ERRORS, 0, 1) == nullptr, "the prediction errors are built");
  }
  // ---- the kernel choice of a launch with a series per chain: never the template kernel
  {
    double dummy = 0.0;
    uint64_t cal = 0;
    for (int tpl = 0; tpl <= 2; ++tpl)
      for (int table = 0; table < 4; ++table) {
        SsParams P{};
        P.T = 10;
        P.ssm.tpl_trend = tpl;   // (a forced choice through ba_ss_set_tuning leaves the shape in the launch)
        P.ssm.tpl_nseasons = 4;
        P.y_stride = 10;
        if (table == 1) { P.qw = &dummy; }
        if (table == 2) { P.cal = &cal; P.cal_count = 10; }
        if (table == 3) { P.dyn = &dummy; P.dyn_rows = 10; P.dyn_cols = 1; P.ssm.ndyn = 1; }
        const SsgChoice c = ssg_choose_kernel(P);
        const SsgVariant want = table == 1 ? SSG_V_QT : table == 2 ? SSG_V_HD : table == 3 ? SSG_V_DR : SSG_V_PLAIN;
        expect(c.kernel == SSG_CHOICE_GENERAL && c.variant == want, "a series per chain: the general kernel", tpl, table);
        P.y_stride = 0;
        const SsgChoice d = ssg_choose_kernel(P);
        expect(d.kernel == (tpl > 0 && table == 0 ? SSG_CHOICE_TEMPLATE : SSG_CHOICE_GENERAL), "the shared series: as before", tpl, table);
      }
  }
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
