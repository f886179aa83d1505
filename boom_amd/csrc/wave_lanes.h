// Cross-lane moves of one wavefront for values held one per lane (DPP / v_readlane: no LDS round trip)
// and the wave's LDS hand-off.  Shared by the state-space kernels: the general structural kernel
// (ssg_device.h), its template (ssm_template_kernel.hip), the prediction-error filter
// (ss_filter_kernel.hip) and, through stream_normals.h, the local-level kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace boom_amd {

namespace {

constexpr int WAVE = 64;

// LDS hand-off between the lanes of one wavefront (DS operations of a wave
// complete in order: only the compiler has to be told)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double sdpp(double x, double fill) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
  const unsigned long long f = __builtin_bit_cast(unsigned long long, fill);
  const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)f, (int)(unsigned)u, CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(f >> 32), (int)(unsigned)(u >> 32), CTRL, ROW_MASK, 0xf, false);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// value of lane `src` (wave-uniform src)
__device__ __forceinline__ double rl(double x, int src) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, src);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// a 64-bit word of lane `src` (wave-uniform src)
__device__ __forceinline__ unsigned long long rlw(unsigned long long u, int src) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, src);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}
// sum over the first 16 lanes (the others hold 0), everywhere
__device__ __forceinline__ double row_total(double x) {
  x += sdpp<0x111, 0xf>(x, 0.0);  // row_shr:1
  x += sdpp<0x112, 0xf>(x, 0.0);
  x += sdpp<0x114, 0xf>(x, 0.0);
  x += sdpp<0x118, 0xf>(x, 0.0);
  return rl(x, 15);
}
// sum over the wave (lanes that do not take part hold 0), everywhere.  SMALL: the state
// has at most 16 components -- one row of lanes
template <bool SMALL>
__device__ __forceinline__ double wsum(double x) {
  x += sdpp<0x111, 0xf>(x, 0.0);
  x += sdpp<0x112, 0xf>(x, 0.0);
  x += sdpp<0x114, 0xf>(x, 0.0);
  x += sdpp<0x118, 0xf>(x, 0.0);
  if (SMALL) return rl(x, 15);
  return ((rl(x, 15) + rl(x, 31)) + rl(x, 47)) + rl(x, 63);
}
// the value of lane - 1 (lane 0: 0) / of lane + 1 (lane 63: 0): wave_shr:1 / wave_shl:1
__device__ __forceinline__ double from_below(double x) { return sdpp<0x138, 0xf>(x, 0.0); }
__device__ __forceinline__ double from_above(double x) { return sdpp<0x130, 0xf>(x, 0.0); }

}  // namespace

}  // namespace boom_amd
