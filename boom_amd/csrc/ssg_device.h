// Device helpers of the general structural state-space kernel (ssm_kernel.hip: one chain per
// workgroup, any state dimension <= 64): the semilocal slope's sampler, the block list and the
// transition's action on lane-distributed vectors; the cross-lane moves are wave_lanes.h's, the
// ArPosteriorSampler is ar_sampler_device.h's.  See ssg_simsmooth.h for the model.
#pragma once
#include <hip/hip_runtime.h>

#include "ar_sampler_device.h"
#include "ar_trunc_device.h"
#include "device_rng.h"
#include "kalman_params.h"
#include "stream_normals.h"
#include "wave_lanes.h"

namespace boom_amd {

namespace {

__device__ __forceinline__ int sprev(int c, int ns) { return c == 0 ? ns - 1 : c - 1; }   // the cursor after a move
__device__ __forceinline__ int snext(int c, int ns) { return c + 1 == ns ? 0 : c + 1; }   // ... before it
// how many of the times 1 .. t start a new season (u % duration == phase)
__device__ __forceinline__ int seasons_started(int t, int duration, int phase) {
  if (t < 0) return 0;
  return (t >= phase ? (t - phase) / duration + 1 : 0) - (phase == 0 ? 1 : 0);
}

// a block of `n` doubles between HBM and LDS, by one wave
__device__ __forceinline__ void blk_load(double *lds, const double *g, int n, int lane) {
  for (int i = lane; i < n; i += WAVE) lds[i] = g[i];
  wave_lds_sync();
}
__device__ __forceinline__ void blk_store(double *g, const double *lds, int n, int lane) {
  wave_lds_sync();
  for (int i = lane; i < n; i += WAVE) g[i] = lds[i];
  wave_lds_sync();
}

// ---- NonzeroMeanAr1Sampler::draw (NonzeroMeanAr1Sampler.cpp:51-155) for a semilocal trend's slope
// model, on its Ar1Suf (NonzeroMeanAr1Model.cpp:39-128; suf = sumsq, sum, cross, n, first, last):
// draw_mu, draw_phi (a normal; truncated to [lo, 1] under force_stationary), draw_sigma -- one
// generator, every lane of the (whole) wave the same numbers.  In / out: mu, phi, sigsq.
__device__ __forceinline__ int semilocal_slope_draw(const double *suf, const double *prior, bool truncate, bool positive,
                                                    double prior_df, double prior_ss, double sigma_max, SeqRng &rng,
                                                    double &mu, double &phi, double &sigsq) {
  const double a1_sumsq = suf[0], a1_sum = suf[1], a1_cross = suf[2], n = suf[3], a1_first = suf[4], a1_last = suf[5];
  const double lag_sumsq = a1_sumsq - a1_last * a1_last;
  const double lag_sum = a1_sum - a1_last;
  const double sum_excluding_first = a1_sum - a1_first;
  const double sumsq_excluding_first = a1_sumsq - a1_first * a1_first;
  {  // draw_mu
    const double psig = prior[1] * prior[1];
    const double omp = 1 - phi;
    double ivar = (1 + (n - 1) * (omp * omp)) / sigsq;
    ivar += 1.0 / psig;
    double mean = (1 - phi) * (sum_excluding_first - phi * lag_sum) + a1_first;
    mean /= sigsq;
    mean += prior[0] / psig;
    mean /= ivar;
    mu = d_rnorm(rng, mean, sqrt(1.0 / ivar));
  }
  {  // draw_phi
    const double psig = prior[3] * prior[3];
    double ivar = lag_sumsq - 2 * lag_sum * mu + (n - 1) * mu * mu;   // centered_lag_sumsq(mu)
    ivar /= sigsq;
    ivar += 1.0 / psig;
    double mean = a1_cross - mu * (sum_excluding_first + lag_sum) + (n - 1) * mu * mu;   // centered_cross(mu)
    mean /= sigsq;
    mean += prior[2] / psig;
    mean /= ivar;
    const double sd = sqrt(1.0 / ivar);
    if (truncate) {
      int bad = 0;
      phi = ar_rtrun_norm_2(rng, mean, sd, positive ? 0.0 : -1.0, 1.0, &bad);
      if (bad) return CHAIN_RNG_BRANCH;
    } else {
      phi = d_rnorm(rng, mean, sd);
    }
  }
  {  // draw_sigma: model_sumsq(mu, phi), df = n
    const double d0 = a1_first - mu, mp = mu * (1 - phi);
    double ss = d0 * d0;
    ss += sumsq_excluding_first - 2 * phi * a1_cross - 2 * (1 - phi) * mu * sum_excluding_first +
          phi * phi * lag_sumsq + 2 * phi * (1 - phi) * mu * lag_sum + (n - 1) * (mp * mp);
    int bad = 0;
    sigsq = d_draw_variance(rng, n + prior_df, ss + prior_ss, sigma_max, &bad);
    if (bad) return CHAIN_RNG_BRANCH;
  }
  return CHAIN_OK;
}

// ---- the block list: lane b of each of three registers holds block b (so that all blocks
// advance in one vector operation and a loop over blocks is a ROLLED loop that fetches its
// block with v_readlane -- eight unrolled copies of every per-block code path made a kernel
// of 60 000 instructions that ran out of the instruction cache).
struct Blocks : SsgBlockWord {
  unsigned desc;   // the block's word (SsgBlockWord: bits 0 - 24) | bit 25: a random-walk holiday (set and read by the
                   // HD instances of ssg_simsmooth_kernel only) | bit 26: a dynamic regression (its DR instances only)
  unsigned dp;     // seasonal: duration (16 bits) | phase (16)  (a calendar seasonal: 1 | 0xffff, its closed forms never fire)
  unsigned rc;     // seasonal: (index of the step's transition + 1 - phase) mod duration (16 bits: 0 = it moves) |
                   //           the rotating layout's cursor (16): physical slot of the block's first component
  int nb;
  unsigned always;     // bit b: block b's transition is never the identity (trend, autoregression)
  unsigned seasmask;   // bit b: block b is seasonal
  unsigned armask;     // bit b: block b is an autoregression
  unsigned trigmask;   // bit b: block b is a trig model (pairs of components that rotate)
  unsigned slmask;     // bit b: block b is a semilocal linear trend (level, slope, the slope's long-run mean)
  static __device__ __forceinline__ bool holiday_of(unsigned d) { return ((d >> 25) & 1u) != 0; }
  static __device__ __forceinline__ bool dynreg_of(unsigned d) { return ((d >> 26) & 1u) != 0; }
  // block b's words, wave-uniform
  __device__ __forceinline__ unsigned udesc(int b) const { return (unsigned)__builtin_amdgcn_readlane((int)desc, b); }
  __device__ __forceinline__ unsigned urc(int b) const { return (unsigned)__builtin_amdgcn_readlane((int)rc, b); }
  __device__ __forceinline__ void load(const SsgSpec &Q, int nblocks, int lane) {
    nb = nblocks;
    desc = 0; dp = 1; rc = 0;
    if (lane < nblocks) {
      const SsgBlock &K = Q.blk[lane];
      desc = pack(K);
      dp = (unsigned)K.duration | ((unsigned)K.phase << 16);
    }
    const int kd = kind_of(desc);
    always = (unsigned)__ballot(kd == SSG_LOCAL_LINEAR_TREND || kd == SSG_AR || kd == SSG_TRIG || kd == SSG_SEMILOCAL);
    slmask = (unsigned)__ballot(kd == SSG_SEMILOCAL);
    seasmask = (unsigned)__ballot(kd == SSG_SEASONAL);
    armask = (unsigned)__ballot(kd == SSG_AR);
    trigmask = (unsigned)__ballot(kd == SSG_TRIG);
  }
  // the layout of time t; the transitions are walked from index t + shift on (0: the
  // transition OUT of the time, T_t; -1: the one INTO it, T_{t-1})
  __device__ __forceinline__ void seek(int t, int shift) {
    if (kind_of(desc) == SSG_SEASONAL) {
      const int d = (int)(dp & 0xffffu), ph = (int)(dp >> 16), n = dim_of(desc);
      const int q = seasons_started(t, d, ph) % n;
      const int c = q == 0 ? 0 : n - q;
      int r = (t + shift + 1 - ph) % d;
      if (r < 0) r += d;
      rc = (unsigned)r | ((unsigned)c << 16);
    }
  }
  // bit b = block b's transition of this step is not the identity
  __device__ __forceinline__ unsigned moving() const {
    return always | (unsigned)__ballot(kind_of(desc) == SSG_SEASONAL && (rc & 0xffffu) == 0u);
  }
  // one step on / back: the layout after (before) the transitions `mv`, the next (previous) transition's phase
  __device__ __forceinline__ void advance(unsigned mv, int lane) {
    if (kind_of(desc) == SSG_SEASONAL) {
      int r = (int)(rc & 0xffffu) + 1, c = (int)(rc >> 16);
      if (r == (int)(dp & 0xffffu)) r = 0;
      if ((mv >> lane) & 1u) c = sprev(c, dim_of(desc));
      rc = (unsigned)r | ((unsigned)c << 16);
    }
  }
  __device__ __forceinline__ void retreat(unsigned mv, int lane) {
    if (kind_of(desc) == SSG_SEASONAL) {
      int r = (int)(rc & 0xffffu), c = (int)(rc >> 16);
      r = r == 0 ? (int)(dp & 0xffffu) - 1 : r - 1;
      if ((mv >> lane) & 1u) c = snext(c, dim_of(desc));
      rc = (unsigned)r | ((unsigned)c << 16);
    }
  }
};

// per-lane constants of the lane's component
struct LaneInfo {
  int blk, kind, first, dim;    // its block (kind 0: the lane holds no component)
  int cur;                      // seasonal: its block's cursor (a per-lane copy)
  double phi;                   // autoregression: the lane's coefficient; semilocal trend: the slope's AR(1) coefficient (every lane of the block)
  double tc = 0.0, ts = 0.0;    // trig: cosine and sine of the lane's pair
  __device__ __forceinline__ bool moves(unsigned mv) const { return kind == SSG_SEASONAL && ((mv >> blk) & 1u); }
  // trig: is this the second component of its pair?
  __device__ __forceinline__ bool todd(int lane) const { return ((lane - first) & 1) != 0; }
  // is this a lane Z selects in its block (the block's first component; trig: every pair's first)?
  template <bool GLOB = true>
  __device__ __forceinline__ bool zsel(int lane) const {
    if (GLOB && kind == SSG_TRIG) return !todd(lane);
    return kind != 0 && lane == first + cur;
  }
};

// Z'x
template <bool SMALL, bool GLOB = true>
__device__ __forceinline__ double zdot(const LaneInfo &L, double x, int lane) {
  return wsum<SMALL>(L.template zsel<GLOB>(lane) ? x : 0.0);
}
// y = T x for a vector held one component per lane, in the layout the cursors say; mv:
// bit b = block b's transition moves at this step (seasonal: the step into a new season);
// the result is in the next layout (the caller advances the cursors)
// GLOB: the list holds a trig or a semilocal-linear-trend block (round 6); lists without them run
// the instance that does not carry their code in its per-step loops
template <bool SMALL, bool GLOB = false>
__device__ __forceinline__ double vecT(const Blocks &B, const LaneInfo &L, double x, int lane, unsigned mv) {
  double y = x;
  // (cross-lane moves read INACTIVE lanes as nothing: they stay outside the per-lane branches)
  const double above = from_above(x);
  if (L.kind == SSG_LOCAL_LINEAR_TREND && lane == L.first) y = x + above;
  // autoregression: new[0] = phi'old, new[i] = old[i - 1]  (AutoRegressionTransitionMatrix, SparseMatrix.cpp:1261-1310)
  if (B.armask) {
    const double below = from_below(x);
    if (L.kind == SSG_AR) y = below;
    unsigned am = B.armask;
    while (am) {
      const int b = __ffs((int)am) - 1;
      am &= am - 1;
      const double tot = wsum<SMALL>(L.blk == b ? L.phi * x : 0.0);
      if (L.blk == b && lane == L.first) y = tot;
    }
  }
  // semilocal trend: (level, slope, mean) -> (level + slope, phi slope + (1 - phi) mean, mean)
  // (SemilocalLinearTrendMatrix::multiply, SemilocalLinearTrend.cpp:36-46)
  if (GLOB && L.kind == SSG_SEMILOCAL) {
    if (lane == L.first) y = x + above;
    else if (lane == L.first + 1) y = L.phi * x + (1 - L.phi) * above;
  }
  // trig: every pair rotates, (x0, x1) -> (c x0 + s x1, -s x0 + c x1)  (the DenseMatrix blocks of
  // TrigStateModel.cpp:144-153)
  if (GLOB && B.trigmask) {
    const double below = from_below(x);
    if (L.kind == SSG_TRIG) y = L.todd(lane) ? -L.ts * below + L.tc * x : L.tc * x + L.ts * above;
  }
  // seasonal, a step into a new season: the slot of the component that drops out receives
  // -(sum over the block)
  unsigned sm = mv & B.seasmask;
  while (sm) {
    const int b = __ffs((int)sm) - 1;
    sm &= sm - 1;
    const double tot = wsum<SMALL>(L.blk == b ? x : 0.0);
    if (L.blk == b && lane == L.first + sprev(L.cur, L.dim)) y = -tot;
  }
  return y;
}
// y = T' x; the cursors are those of x's layout (time t + 1); mv as above for the step t -> t + 1
template <bool GLOB = false>
__device__ __forceinline__ double vecTt(const Blocks &B, const LaneInfo &L, double x, int lane, unsigned mv) {
  double y = x;
  const double below = from_below(x);
  if (L.kind == SSG_LOCAL_LINEAR_TREND && lane == L.first + 1) y = below + x;
  if (B.armask) {
    // out[i] = phi_i x[0] + x[i + 1]  (Tmult, SparseMatrix.cpp:1286-1295)
    const double above = from_above(x);
    unsigned am = B.armask;
    while (am) {
      const int b = __ffs((int)am) - 1;
      am &= am - 1;
      const double firstv = rl(x, Blocks::first_of(B.udesc(b)));
      if (L.blk == b) y = L.phi * firstv + ((lane + 1 < L.first + L.dim) ? above : 0.0);
    }
  }
  // semilocal trend: Tmult (SemilocalLinearTrend.cpp:65-76): (r0, r1, r2) -> (r0, r0 + phi r1, (1 - phi) r1 + r2)
  if (GLOB && L.kind == SSG_SEMILOCAL) {
    if (lane == L.first + 1) y = below + L.phi * x;
    else if (lane == L.first + 2) y = (1 - L.phi) * below + x;
  }
  if (GLOB && B.trigmask) {
    // the rotations' transposes: (x0, x1) -> (c x0 - s x1, s x0 + c x1)
    const double above = from_above(x);
    if (L.kind == SSG_TRIG) y = L.todd(lane) ? L.ts * below + L.tc * x : L.tc * x + -L.ts * above;
  }
  unsigned sm = mv & B.seasmask;
  while (sm) {
    const int b = __ffs((int)sm) - 1;
    sm &= sm - 1;
    const int c1 = Blocks::first_of(B.udesc(b)) + (int)(B.urc(b) >> 16);
    const double firstv = rl(x, c1);
    if (L.blk == b) y = (lane == c1) ? -firstv : x - firstv;
  }
  return y;
}
__device__ __forceinline__ void advance(Blocks &B, LaneInfo &L, unsigned mv, int lane) {
  B.advance(mv, lane);
  if (L.moves(mv)) L.cur = sprev(L.cur, L.dim);
}
__device__ __forceinline__ void retreat(Blocks &B, LaneInfo &L, unsigned mv, int lane) {
  B.retreat(mv, lane);
  if (L.moves(mv)) L.cur = snext(L.cur, L.dim);
}
// the layout of time t (see Blocks::seek)
__device__ __forceinline__ void seek(Blocks &B, LaneInfo &L, int t, int shift) {
  B.seek(t, shift);
  // (every lane takes part: a lane that is switched off is read as 0 by the others)
  const unsigned mine = (unsigned)__shfl((int)B.rc, L.blk < 0 ? 0 : L.blk);
  __builtin_amdgcn_wave_barrier();
  L.cur = (L.kind == SSG_SEASONAL) ? (int)(mine >> 16) : 0;
}

}  // namespace

}  // namespace boom_amd
