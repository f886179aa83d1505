// Test-only probe of the parallel Fisher-Yates shuffle, for tests/test_parallel_shuffle_gpu.py
// and tests/test_isa_lds_chains.py.
//
// One small kernel per template flag instantiates the product's own parallel_shuffle<MASKED>
// (ssvs_device.h) and restates none of it.  A Chain's perm, perm_alt, oth, last and pred are
// bound in dynamic LDS at the offsets the product's layout (ssvs_lds_layout) gives them, so the
// spare entry the routine relies on is the layout's, not the probe's.  The bound region is
// filled with a byte pattern first: whatever the routine reads without having written it is
// garbage here as it is in the product.  One wavefront runs the routine twice on the same
// targets; the order after each call is copied out.
//
// The exported wrapper takes host arrays with explicit lengths, checks ON THE HOST that the
// request is one the routine is defined for (SP_BAD_REQUEST instead of a launch where it is
// not), launches on the null stream, synchronises and returns the hipError_t.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ssvs_device.h"

using namespace boom_amd;

namespace {

enum : int { SP_BAD_REQUEST = -1, SP_KCAP = 16, SP_MAX_P = 4096 };

// out[0 .. p): the order after one call; out[p .. 2p): after a second call on that order
template <bool MASKED>
__global__ void __launch_bounds__(64) shuffle_kernel(int p, const uint16_t *perm, const uint16_t *oth, uint16_t *out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const SsvsLds lay = ssvs_lds_layout(p, SP_KCAP);
  const int lane = (int)(threadIdx.x & 63);
  const uint32_t bytes = lay.gam - lay.perm0;   // perm0, perm1, oth, last, pred: contiguous
  for (uint32_t b = lane; b < bytes; b += WAVE) smem[b] = (unsigned char)0xA5;
  __syncthreads();
  Chain ch;
  ch.lane = lane;
  ch.p = p;
  ch.perm = to_lds<uint16_t>(smem);
  ch.perm_alt = to_lds<uint16_t>(smem + (lay.perm1 - lay.perm0));
  ch.oth = to_lds<uint16_t>(smem + (lay.oth - lay.perm0));
  ch.last = to_lds<uint32_t>(smem + (lay.last - lay.perm0));
  ch.pred = to_lds<uint16_t>(smem + (lay.pred - lay.perm0));
  for (int i = lane; i < p; i += WAVE) {
    ch.perm[i] = perm[i];
    ch.oth[i] = oth[i];
  }
  wave_sync();
  StampCtx sx;
  sx.last = 0;
  for (int call = 0; call < 2; ++call) {
    parallel_shuffle<MASKED>(ch, sx);
    for (int i = lane; i < p; i += WAVE) out[(size_t)call * p + i] = ch.perm[i];
    wave_sync();
  }
}

}  // namespace

extern "C" {

// bytes of dynamic LDS a launch at p binds
int sp_lds_bytes(int p) {
  if (p < 2 || p > SP_MAX_P) return SP_BAD_REQUEST;
  const SsvsLds lay = ssvs_lds_layout(p, SP_KCAP);
  return (int)(lay.gam - lay.perm0);
}

// perm, oth: p entries (oth[i] in [0, i] for i >= 1; oth[0] is not read); out: 2 p entries
int sp_shuffle(int masked, int p, const uint16_t *perm, const uint16_t *oth, uint16_t *out, size_t nout) {
  if (!perm || !oth || !out || p < 2 || p > SP_MAX_P || nout < 2 * (size_t)p) return SP_BAD_REQUEST;
  for (int i = 1; i < p; ++i)
    if (oth[i] > i) return SP_BAD_REQUEST;
  const SsvsLds lay = ssvs_lds_layout(p, SP_KCAP);
  const uint32_t bytes = lay.gam - lay.perm0;
  // the five arrays with their spare entries, as the routine indexes them
  if (bytes < 6u * 2u * ((uint32_t)p + 1u) || bytes > 64u * 1024u) return SP_BAD_REQUEST;
  uint16_t *dp = nullptr, *dt = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc((void **)&dp, (size_t)p * 2);
  if (e == hipSuccess) e = hipMalloc((void **)&dt, (size_t)p * 2);
  if (e == hipSuccess) e = hipMalloc((void **)&dout, (size_t)p * 4);
  if (e == hipSuccess) e = hipMemcpy(dp, perm, (size_t)p * 2, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dt, oth, (size_t)p * 2, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    if (masked)
      hipLaunchKernelGGL(shuffle_kernel<true>, dim3(1), dim3(64), bytes, nullptr, p, dp, dt, dout);
    else
      hipLaunchKernelGGL(shuffle_kernel<false>, dim3(1), dim3(64), bytes, nullptr, p, dp, dt, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)p * 4, hipMemcpyDeviceToHost);
  if (dp) (void)hipFree(dp);
  if (dt) (void)hipFree(dt);
  if (dout) (void)hipFree(dout);
  return (int)e;
}

}  // extern "C"
