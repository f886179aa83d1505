// The dynamic regression's instances of the general structural kernel (ssg_simsmooth.h): a list that
// holds a dynamic regression block, whose observation row is a row of data.
#include "ssg_simsmooth.h"

namespace boom_amd {

hipError_t launch_ssg_dr(hipStream_t stream, const SsParams &P, int draw_variances, size_t lds) {
  const dim3 grid(P.chain_count), block(2 * WAVE);
  // (more than 64 KB of dynamic LDS has to be asked for -- per device, so every time)
  auto go = [&](auto kernel) -> hipError_t {
    if (lds > 65536) {
      const hipError_t e2 = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e2 != hipSuccess) return e2;
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, P, draw_variances);
    return hipSuccess;
  };
  // (every step reads its row of the table; the staging buffers are sized by the launch's column count)
  if (!P.dyn || P.dyn_rows < P.T || P.dyn_cols < 1 || P.dyn_cols != P.ssm.ndyn) return hipErrorInvalidValue;
  const bool glob = P.ssm.glob != 0;   // (a trig or semilocal block in the list)
  switch (P.ssm.ld) {   // ssg_leading_dimension(m)
    case 17: return glob ? go(ssg_simsmooth_kernel<true, 17, true, false, false, false, true>) : go(ssg_simsmooth_kernel<true, 17, false, false, false, false, true>);
    case 33: return glob ? go(ssg_simsmooth_kernel<false, 33, true, false, false, false, true>) : go(ssg_simsmooth_kernel<false, 33, false, false, false, false, true>);
    case 61: return glob ? go(ssg_simsmooth_kernel<false, 61, true, false, false, false, true>) : go(ssg_simsmooth_kernel<false, 61, false, false, false, false, true>);
    case 65: return glob ? go(ssg_simsmooth_kernel<false, 65, true, false, false, false, true>) : go(ssg_simsmooth_kernel<false, 65, false, false, false, false, true>);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace boom_amd
