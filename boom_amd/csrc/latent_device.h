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

#include "device_rng.h"

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

// sum over the workgroup's 256 threads, in a fixed order; every thread gets the result
// (s_red: four doubles of LDS)
__device__ __forceinline__ double stu_block_sum(double v, double *s_red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();   // (s_red may still be read from the previous call)
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// ScalarSliceSampler::draw (Samplers/ScalarSliceSampler.cpp:75-253) for a target bounded below at 0:
// find_limits -> find_upper_limit from x + dx, then draw / contract.  S.logf(x) is the log density
// (every thread of the workgroup calls it: it may reduce over the workgroup), S.note(a, b) is told
// every pair the sampler compares.  unimodal: the sampler's switch -- true doubles the upper limit
// only while it is inside the slice, false adds the random doublings (a uniform each).  x: the
// current value; dx: the suggested width, in and out; out: the draw.  Returns 0, or 1 where the
// reference reports an error.  Every thread reads the same numbers from its own copy of rng.
template <class Target, class R>
__device__ __forceinline__ int slice_draw_lower0(Target &S, R &rng, const bool unimodal, const double x, double &dx,
                                                 double &out) {
  int err = 0;
  const double logp_slice = S.logf(x) - d_rexp(rng, 1.0);
  if (!isfinite(logp_slice)) err = 1;                        // check_finite
  double lo = 0.0, hi = 0.0;
  if (!err) {
    hi = x + dx;
    double logphi = S.logf(hi);
    S.note(logphi, logp_slice);
    int doublings = 0;
    while (logphi >= logp_slice || (!unimodal && d_runif(rng, 0.0, 1.0) > .5)) {
      hi = x + 2 * (hi - x);                                   // double_hi
      if (!isfinite(hi)) { err = 1; break; }
      logphi = S.logf(hi);
      S.note(logphi, logp_slice);
      if (++doublings > 100) { err = 1; break; }
    }
    if (!err && (!isfinite(hi) || isnan(logphi))) err = 1;   // check_upper_limit
  }
  if (!err) {
    int tries = 0;
    for (;;) {
      const double cand = d_runif(rng, lo, hi);
      const double lp = S.logf(cand);
      S.note(lp, logp_slice);
      if (!(lp < logp_slice)) { out = cand; break; }
      if (cand > x) hi = cand; else lo = cand;                 // contract
      dx = hi - lo;
      if (++tries > 100) { err = 1; break; }
    }
  }
  return err;
}

}  // namespace boom_amd
