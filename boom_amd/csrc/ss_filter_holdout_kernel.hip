// The holdout instance of the filter kernel (ba_ss_holdout_prediction_errors): ss_filter_kernel.hip's body,
// compiled here as ss_filter_kernel<true> in a translation unit of its own, so that the in-sample instance's
// code stays what it is without it.
#define SS_FILTER_HOLDOUT_UNIT 1
#include "ss_filter_kernel.hip"
