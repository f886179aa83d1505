// Device helpers of the latent-data imputation kernels (probit_kernel.hip, student_kernel.hip,
// quantile_kernel.hip, mlogit_kernel.hip).  They take plain values and pointers, not a
// parameter struct, so every family's kernel calls them with the fields of its own struct.
// The two scalars come by const reference: the kernels pass fields of their kernel argument,
// and read where the helper uses them -- as the per-family copies these replace did -- the
// compiler emits the copies' code instruction for instruction (by value one kernel's register
// count moved: DESIGN 3.13).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace boom_amd {

// how many uniforms a slot of an imputer's substream hands out before the draw goes on in the
// spill stream (device_rng.h): the whole stride, or what ba_set_slot_limit asked for (tests)
__device__ __forceinline__ uint32_t slot_serve(const int32_t &slot_limit, uint32_t stride) {
  return (slot_limit > 0 && (uint32_t)slot_limit < stride) ? (uint32_t)slot_limit : stride;
}

// The chain's included variables and their coefficients, in ascending order (the
// order x_i'beta is summed in), to LDS; returns how many there are (beyond
// KMAX only counted).  All 256 threads: 256 variables per round, a
// variable's place = included ones in earlier rounds + earlier waves + earlier lanes.
template <int KMAX>
__device__ __forceinline__ int included_coefficients(const uint8_t *gamma, const double *beta, const int &p,
                                                     int chain, int *s_idx, double *s_beta) {
  __shared__ int s_wave_count[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint8_t *g = gamma + (size_t)chain * p;
  const double *b = beta + (size_t)chain * p;
  int base = 0;
  for (int j0 = 0; j0 < p; j0 += 256) {
    const int j = j0 + tid;
    const bool inc = j < p && g[j] != 0;
    const unsigned long long m = __ballot(inc);
    if (lane == 0) s_wave_count[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = s_wave_count[w];
      before += (w < wave) ? c : 0;
      total += c;
    }
    if (inc) {
      const int pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
      if (pos < KMAX) { s_idx[pos] = j; s_beta[pos] = b[j]; }
    }
    base += total;
    __syncthreads();
  }
  return base;
}

}  // namespace boom_amd
