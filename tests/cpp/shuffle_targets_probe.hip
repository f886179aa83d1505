// Test-only probe of the shuffle's targets, for tests/test_shuffle_targets_gpu.py.
//
// One kernel per number of wavefronts W instantiates the product's own fork_shuffle_targets<W>
// (ssvs_device.h) -- called as the sweep kernel calls it after the fork's command barrier: the
// master with wave 0, every other wavefront with its own number -- or the all-threads
// shuffle_targets of the unforked path, and restates neither.  oth lives in dynamic LDS with the
// spare entry the product's arrays have; all p + 1 entries hold a sentinel before the call and
// are copied out after it, so what the call left alone can be seen.
//
// The exported wrapper checks ON THE HOST that the request is one the routines are defined for
// (ST_BAD_REQUEST instead of a launch where it is not), launches on the null stream,
// synchronises and returns the hipError_t.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ssvs_device.h"

using namespace boom_amd;

namespace {

enum : int { ST_BAD_REQUEST = -1, ST_MAX_P = 4096 };

template <int W>
__global__ void __launch_bounds__(64 * W) targets_kernel(int forked, int p, PhiloxKey key, uint64_t pos,
                                                         uint16_t sentinel, uint16_t *out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  lds_u16 *oth = to_lds<uint16_t>(smem);
  const int tid = (int)threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  for (int i = tid; i <= p; i += WAVE * W) oth[i] = sentinel;
  __syncthreads();   // (the command barrier's place)
  if (forked) {
    if (wave == 0) fork_shuffle_targets<W>(key, pos, p, 0, lane, oth);
    else fork_shuffle_targets<W>(key, pos, p, wave, lane, oth);
  } else {
    shuffle_targets(key, pos, p, tid, WAVE * W, oth);
  }
  __syncthreads();
  for (int i = tid; i <= p; i += WAVE * W) out[i] = oth[i];
}

}  // namespace

extern "C" {

// out: p + 1 entries (entry 0 and the spare entry p come back as the sentinel)
int st_targets(int waves, int forked, int p, uint32_t seed_lo, uint32_t seed_hi, uint32_t chain, uint32_t stream,
               uint64_t pos, uint16_t sentinel, uint16_t *out, size_t nout) {
  if (!out || (waves != 2 && waves != 4) || p < 2 || p > ST_MAX_P || nout < (size_t)p + 1) return ST_BAD_REQUEST;
  const PhiloxKey key{seed_lo, seed_hi, chain, stream};
  const size_t n = (size_t)p + 1;
  const unsigned bytes = (unsigned)((n * 2 + 15) & ~(size_t)15);
  uint16_t *dout = nullptr;
  hipError_t e = hipMalloc((void **)&dout, n * 2);
  if (e == hipSuccess) e = hipMemset(dout, 0, n * 2);
  if (e == hipSuccess) {
    if (waves == 2)
      hipLaunchKernelGGL(targets_kernel<2>, dim3(1), dim3(128), bytes, nullptr, forked, p, key, pos, sentinel, dout);
    else
      hipLaunchKernelGGL(targets_kernel<4>, dim3(1), dim3(256), bytes, nullptr, forked, p, key, pos, sentinel, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, n * 2, hipMemcpyDeviceToHost);
  if (dout) (void)hipFree(dout);
  return (int)e;
}

}  // extern "C"
