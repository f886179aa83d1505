// Host-only check of boom_amd/csrc/ssg_instances.h: which kernel serves a state draw of the structural
// model.  Every on/off combination of the four tables a launch can carry (h, qw, cal, dyn), with and
// without a template shape, with table sizes that fit the series and sizes that do not.  The expected
// choices are written out below by hand from the rules of launch_ssm_simsmooth (template kernel iff a
// template shape and no table; precedence dyn, cal, qw, h, plain; two tables at once are refused; a table
// shorter than the series, or a column count that is not the list's, is refused) -- not computed by the
// function under test.  Built with -fsanitize=address,undefined and run by tests/test_ssg_instances_cpu.py.
#include <cstdio>

#include "../../boom_amd/csrc/ssg_instances.h"

using namespace boom_amd;

static int failures = 0, checks = 0;

// one letter per choice: T template kernel; general kernel P plain, H HT, Q QT, C HD (calendar), D DR; x refused
static char letter(const SsgChoice &c) {
  if (c.kernel == SSG_CHOICE_INVALID) return 'x';
  if (c.kernel == SSG_CHOICE_TEMPLATE) return 'T';
  switch (c.variant) {
    case SSG_V_PLAIN: return 'P';
    case SSG_V_HT: return 'H';
    case SSG_V_QT: return 'Q';
    case SSG_V_HD: return 'C';
    case SSG_V_DR: return 'D';
  }
  return '?';
}

// the table sizes of a launch of T = 100 steps whose list has 3 dynamic regression columns
struct Sizes {
  const char *name;
  long long dyn_rows;
  int dyn_cols, ndyn;
  long long cal_count;
  // entry `mask` = the choice when h (bit 0), qw (bit 1), cal (bit 2), dyn (bit 3) are set; without / with a template shape
  const char *expect_general, *expect_template;
};
static const Sizes CASES[] = {
    //                                       mask: 0123456789abcdef    0123456789abcdef
    {"tables longer than the series", 120, 3, 3, 120, "PHQxCxxxDxxxxxxx", "THQxCxxxDxxxxxxx"},
    {"tables of exactly T entries", 100, 3, 3, 100, "PHQxCxxxDxxxxxxx", "THQxCxxxDxxxxxxx"},
    {"dyn_rows < T", 99, 3, 3, 120, "PHQxCxxxxxxxxxxx", "THQxCxxxxxxxxxxx"},
    {"dyn_cols < 1", 120, 0, 0, 120, "PHQxCxxxxxxxxxxx", "THQxCxxxxxxxxxxx"},
    {"dyn_cols != ssm.ndyn", 120, 2, 3, 120, "PHQxCxxxxxxxxxxx", "THQxCxxxxxxxxxxx"},
    {"cal_count < T", 120, 3, 3, 99, "PHQxxxxxDxxxxxxx", "THQxxxxxDxxxxxxx"},
};

int main() {
  static const double h[1] = {1.0}, qw[1] = {1.0}, dyn[1] = {0.0};
  static const uint64_t cal[1] = {SSG_CAL_NONE};
  for (const Sizes &S : CASES)
    for (int tpl = 0; tpl <= 1; ++tpl)
      for (int mask = 0; mask < 16; ++mask) {
        SsParams P{};
        P.T = 100;
        P.ssm.tpl_trend = tpl;
        P.ssm.ndyn = S.ndyn;
        P.dyn_rows = S.dyn_rows;
        P.dyn_cols = S.dyn_cols;
        P.cal_count = S.cal_count;
        P.h = (mask & 1) ? h : nullptr;
        P.qw = (mask & 2) ? qw : nullptr;
        P.cal = (mask & 4) ? cal : nullptr;
        P.dyn = (mask & 8) ? dyn : nullptr;
        const char want = (tpl ? S.expect_template : S.expect_general)[mask];
        const char got = letter(ssg_choose_kernel(P));
        ++checks;
        if (got != want) {
          std::printf("FAIL %s, tpl_trend %d, h %d qw %d cal %d dyn %d: chose %c, expected %c\n", S.name, tpl, mask & 1,
                      (mask >> 1) & 1, (mask >> 2) & 1, (mask >> 3) & 1, got, want);
          ++failures;
        }
      }
  // a local linear trend's template shape (tpl_trend = 2) is a template shape too
  {
    SsParams P{};
    P.T = 100;
    P.ssm.tpl_trend = 2;
    ++checks;
    if (letter(ssg_choose_kernel(P)) != 'T') { std::printf("FAIL tpl_trend 2 without tables\n"); ++failures; }
  }
  std::printf("ssg_instances_check: %d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
