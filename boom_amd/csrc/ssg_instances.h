// Which kernel serves a state draw of the structural model (launch_ssm_simsmooth, ssm_kernel.hip): the
// template kernel (ssm_template_kernel.hip) or one variant of the general kernel (ssg_simsmooth.h).  Plain
// C++ over kalman_params.h, so that the choice is checked on the host (tests/cpp/ssg_instances_check.cpp).
#pragma once
#include "kalman_params.h"

namespace boom_amd {

// What a list adds to the general kernel's per-step code: at most one of
//   HT  a per-step observation variance (SsParams::h: the observation families),
//   QT  a Student local linear trend's per-step state variances (SsParams::qw),
//   HD  a packed calendar (SsParams::cal: random-walk holidays, calendar seasonals),
//   DR  a predictor table (SsParams::dyn: dynamic regressions)
// -- the rule book (ssg_refusal, ssg_spec.h) refuses a list that would need two.
enum SsgVariant { SSG_V_PLAIN, SSG_V_HT, SSG_V_QT, SSG_V_HD, SSG_V_DR };

enum SsgKernelChoice { SSG_CHOICE_INVALID, SSG_CHOICE_TEMPLATE, SSG_CHOICE_GENERAL };
struct SsgChoice {
  SsgKernelChoice kernel;
  SsgVariant variant;   // (SSG_CHOICE_GENERAL only)
};

// The launch's kernel, from the tables the launch carries.  Invalid: two tables at once, or a table
// shorter than the series (every step reads its calendar entry / its row of predictors; the kernel's
// staging buffers are sized by ssm.ndyn columns).  A series per chain (y_stride: the Poisson family's with
// h, a list with regression holiday models without) is the general kernel's whatever the shape: the
// template kernel reads the shared series.
inline SsgChoice ssg_choose_kernel(const SsParams &P) {
  const SsgChoice invalid{SSG_CHOICE_INVALID, SSG_V_PLAIN};
  if (P.ssm.tpl_trend > 0 && !P.h && !P.qw && !P.cal && !P.dyn && P.y_stride == 0) return {SSG_CHOICE_TEMPLATE, SSG_V_PLAIN};
  if (P.dyn) {
    if (P.h || P.qw || P.cal) return invalid;
    if (P.dyn_rows < P.T || P.dyn_cols < 1 || P.dyn_cols != P.ssm.ndyn) return invalid;
    return {SSG_CHOICE_GENERAL, SSG_V_DR};
  }
  if (P.cal) {
    if (P.h || P.qw) return invalid;
    if (P.cal_count < P.T) return invalid;
    return {SSG_CHOICE_GENERAL, SSG_V_HD};
  }
  if (P.qw) {
    if (P.h) return invalid;
    return {SSG_CHOICE_GENERAL, SSG_V_QT};
  }
  return {SSG_CHOICE_GENERAL, P.h ? SSG_V_HT : SSG_V_PLAIN};
}

}  // namespace boom_amd
