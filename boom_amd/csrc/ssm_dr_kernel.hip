// The dynamic regression's instances of the general structural kernel (ssg_simsmooth.h): a list that
// holds a dynamic regression block, whose observation row is a row of data.
#include "ssg_simsmooth.h"

namespace boom_amd {

hipError_t launch_ssg_dr(hipStream_t stream, const SsParams &P, int draw_variances, size_t lds) { return ssg_launch_variant<SSG_V_DR>(stream, P, draw_variances, lds); }

}  // namespace boom_amd
