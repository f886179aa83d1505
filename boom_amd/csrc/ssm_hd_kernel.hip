// The calendar instances of the general structural kernel (ssg_simsmooth.h): a list that holds a
// random-walk holiday block, whose observation row and state-error row move with a calendar, or a
// calendar seasonal, whose season starts are read from the same table.
#include "ssg_simsmooth.h"

namespace boom_amd {

hipError_t launch_ssg_hd(hipStream_t stream, const SsParams &P, int draw_variances, size_t lds) { return ssg_launch_variant<SSG_V_HD>(stream, P, draw_variances, lds); }

}  // namespace boom_amd
