// The Q_t instances of the general structural kernel (ssg_simsmooth.h): a list that holds a Student
// local linear trend, whose two state errors have the per-step variances sigma^2 / w_t.
#include "ssg_simsmooth.h"

namespace boom_amd {

hipError_t launch_ssg_qt(hipStream_t stream, const SsParams &P, int draw_variances, size_t lds) { return ssg_launch_variant<SSG_V_QT>(stream, P, draw_variances, lds); }

}  // namespace boom_amd
