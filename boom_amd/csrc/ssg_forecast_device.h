// One forecast step of the structural state, shared by the forecast kernels of every
// observation family (ssm_kernel.hip: Gaussian; ss_family_forecast_kernel.hip: Student-t,
// Poisson, logit): simulate_next_state (StateSpaceModelBase.cpp:439-443) through
// advance_to_timestamp (:455-459), the state errors model by model in the reference's order
// on the chain's forecast stream.  One wavefront per chain, lane = state component (logical
// order; the horizon is short, a seasonal block simply shifts).
#pragma once
#include "device_rng.h"
#include "kalman_params.h"
#include "ssg_device.h"

namespace boom_amd {

namespace {

// st <- T_tm st + the state errors of time tm (lanes past the state dimension hold 0);
// returns Z'st of the new state: the blocks' first components (a trig block: every pair's
// first), in state order.  cal: the packed calendar of the list's random-walk holidays (entries up
// to tm + 2; nullptr: the list has none).  Such a block's error of time tm lands on its position at
// time tm + 1 -- drawn only where that time is active, as the reference does -- and the returned
// Z'st is that of time tm + 2, the time simulate_multiplex_forecast observes the new state at.
// A calendar seasonal steps into a new season where entry tm + 1 carries SSG_CAL_SEASON.
// dyn: the predictor table of the list's dynamic regressions (dyn_cols columns, rows up to tm + 2; nullptr:
// none).  Such a block advances with one error per coefficient, in order, and the returned Z'st weighs its
// components with row tm + 2 of the table.  An autoregression block with SsgBlock::dynreg set (one coefficient
// of an AR dynamic regression) advances as an autoregression and weighs its first component with its column.
__device__ __forceinline__ double ssg_forecast_step(const SsmParams &M, const SsgSpec &Q, int chain, int lane, int tm,
                                                    SeqRng &rng, double &st, const uint64_t *cal = nullptr,
                                                    const double *dyn = nullptr, int dyn_cols = 0) {
  const int m = M.m, nb = M.nblocks;
  double nx = st;
  for (int b = 0; b < nb; ++b) {
    const SsgBlock &K = Q.blk[b];
    const int f = K.first, n = K.dim;
    const bool mine = lane >= f && lane < f + n;
    const double *sg = M.var_sigsq + (size_t)chain * SSG_MAX_VAR + K.var0;
    if (K.kind == SSG_LOCAL_LEVEL && K.holiday) {
      const int k = cal ? (int)((cal[tm + 1] >> (8 * b)) & 0xffu) : SSG_CAL_OFF;
      if (!(k & SSG_CAL_OFF)) {
        const double e0 = d_rnorm(rng, 0.0, sqrt(sg[0]));
        if (lane == f + k) nx = st + e0;
      }
    } else if (K.kind == SSG_LOCAL_LEVEL && K.dynreg) {
      for (int q = 0; q < n; ++q) {
        const double eq = d_rnorm(rng, 0.0, sqrt(sg[q]));
        if (lane == f + q) nx = st + eq;
      }
    } else if (K.kind == SSG_LOCAL_LEVEL) {
      const double e0 = d_rnorm(rng, 0.0, sqrt(sg[0]));
      if (lane == f) nx = st + e0;
    } else if (K.kind == SSG_LOCAL_LINEAR_TREND) {
      const double z0 = d_rnorm(rng, 0.0, 1.0), z1 = d_rnorm(rng, 0.0, 1.0);
      const double x1 = rl(st, f + 1);
      if (lane == f) nx = (st + x1) + (sqrt(sg[0]) * z0 + 0.0);
      if (lane == f + 1) nx = st + (sqrt(sg[1]) * z1 + 0.0);
    } else if (K.kind == SSG_SEMILOCAL) {
      const double *ph = M.ar_phi + ((size_t)chain * SSG_MAX_AR + K.ar_index) * AR_MAX;
      const double e0 = d_rnorm(rng, 0.0, sqrt(sg[0])), e1 = d_rnorm(rng, 0.0, sqrt(sg[1]));
      const double above = from_above(st);
      if (lane == f) nx = (st + above) + e0;
      else if (lane == f + 1) nx = (ph[0] * st + (1 - ph[0]) * above) + e1;
    } else if (K.kind == SSG_TRIG) {
      // rnorm_mt(rng, 0, sigma) per component, in order (TrigStateModel.cpp:218-223), on the rotated state
      const double sd = sqrt(sg[0]);
      const double above = from_above(st), below = from_below(st);
      const double c = mine ? Q.trig_c[lane] : 0.0, sn = mine ? Q.trig_s[lane] : 0.0;
      double e4 = 0.0;
      for (int q = 0; q < n; ++q) {
        const double eq = d_rnorm(rng, 0.0, sd);
        if (lane == f + q) e4 = eq;
      }
      if (mine) nx = (((lane - f) & 1) ? -sn * below + c * st : c * st + sn * above) + e4;
    } else if (K.kind == SSG_SEASONAL) {
      // (a calendar seasonal: the season flag of time tm + 1 in the packed calendar)
      const bool starts = ssg_is_calendar(K) ? (cal && ((cal[tm + 1] >> (8 * b)) & (uint64_t)SSG_CAL_SEASON) != 0)
                                     : (tm + 1) % K.duration == K.phase;
      if (starts) {
        const double e2 = d_rnorm(rng, 0.0, sqrt(sg[0]));
        // (first = 0 - s_0 - s_1 - ..., SeasonalStateSpaceMatrix::multiply)
        double firstv = 0.0;
        for (int q = 0; q < n; ++q) firstv -= rl(st, f + q);
        const double below = from_below(st);
        if (lane == f) nx = firstv + e2; else if (mine) nx = below;
      }
    } else {
      const double *ph = M.ar_phi + ((size_t)chain * SSG_MAX_AR + K.ar_index) * AR_MAX;
      const double e3 = d_rnorm(rng, 0.0, 1.0) * sqrt(sg[0]);
      // (first = sum of phi_i s_i from the last lag down, AutoRegressionTransitionMatrix::multiply_inplace)
      double firstv = 0.0;
      for (int q = n - 1; q >= 0; --q) firstv += ph[q] * rl(st, f + q);
      const double below = from_below(st);
      if (lane == f) nx = firstv + e3; else if (mine) nx = below;
    }
  }
  st = (lane < m) ? nx : 0.0;
  double zs = 0.0;
  for (int b = 0; b < nb; ++b) {
    const SsgBlock &K = Q.blk[b];
    if (K.holiday) {   // (the position Z selects at the new state's time, if that time is active)
      const int k = cal ? (int)((cal[tm + 2] >> (8 * b)) & 0xffu) : SSG_CAL_OFF;
      if (!(k & SSG_CAL_OFF)) zs += rl(st, K.first + k);
      continue;
    }
    if (K.dynreg) {   // (Z = the predictors of the new state's time)
      const double *x = dyn + (size_t)(tm + 2) * dyn_cols + (K.dynreg - 1);
      for (int i = 0; i < (K.kind == SSG_AR ? 1 : K.dim); ++i) {
        const double zv = x[i] * rl(st, K.first + i);
        zs = (b == 0 && i == 0) ? zv : zs + zv;
      }
      continue;
    }
    for (int i = 0; i < (K.kind == SSG_TRIG ? K.dim : 1); i += 2) {
      const double zv = rl(st, K.first + i);
      zs = (b == 0 && i == 0) ? zv : zs + zv;
    }
  }
  return zs;
}

}  // namespace

}  // namespace boom_amd
