// One-step prediction errors and log likelihood of every chain's current draw:
// ScalarStateSpaceModelBase::one_step_prediction_errors (StateSpaceModelBase.cpp:682-691) and
// the log likelihood bsts stores beside it -- a forward-only scalar Kalman filter
// (ScalarMarginalDistribution::update, ScalarKalmanFilter.cpp:41-83) at the chain's parameters,
// for any list of state models of state dimension <= 64 and for the local-level path (a
// one-block list).  The kernel observes: it writes its outputs and nothing else, reads no
// random stream and does not touch the chains' status.
//
// One wavefront per chain.  The state variance P (m x m) sits in LDS at an odd leading
// dimension ld > m, column m of every row carries the state mean a.  Per step
//   PZ = P Z, F = Z'PZ + sigma^2, v = y* - Z'a;
//   observed: a += PZ v / F, P -= PZ PZ' / F  (the filtered form; (PZ_i PZ_j) / F is symmetric to the bit)
//   P <- T P T' + RQR, a <- T a: T is applied by ONE lane per column (rows of the blocks that
//   move, in place; the a column with them), then by one lane per row -- no cross-lane moves,
//   rows of blocks whose transition is the identity at this step are not touched -- and the
//   upper triangle is mirrored into the lower one where a transition moved.
// y*_t = y_t - x_t'beta (included coefficients) is computed first, a step per lane, into the
// chain's output row; the serial pass reads it back 64 steps at a time and overwrites it.
// log F, v^2 / F and v / sqrt F are taken after every block of 64 steps, a step per lane, and
// the log likelihood's terms summed in step order: the logarithm is off the serial path.
//
// The same kernel body serves the one-step HOLDOUT prediction errors (StateSpaceRegressionModel::
// one_step_holdout_prediction_errors, StateSpaceRegressionModel.cpp:280-305) as its second instance: the
// caller's rows behind the series, filtered from the chain's drawn final state with the variance RQR_{T-1}.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ktimer.h"
#include "ss_filter_params.h"
#include "wave_lanes.h"

namespace boom_amd {

namespace {

// lane b: block b's word (SsgBlockWord: bits 0 - 24) | bit 25: the block has a variance (a static intercept has none)
struct SsfBlocks : SsgBlockWord {
  unsigned desc;
  int nb;
  static __device__ __forceinline__ bool has_var(unsigned d) { return ((d >> 25) & 1u) != 0; }
  __device__ __forceinline__ unsigned at(int b) const { return (unsigned)__builtin_amdgcn_readlane((int)desc, b); }
};

// x <- T_t x for a state vector in LDS, component k at x[k * s], by one lane.  mv: bit b =
// seasonal block b steps into a new season.  Rows of identity transitions are not read.
__device__ __forceinline__ void ssf_apply_T(const SsfBlocks &B, unsigned mv, const double *s_phi, const double *s_tc,
                                            const double *s_ts, double *x, int s) {
  for (int b = 0; b < B.nb; ++b) {
    const unsigned d = B.at(b);
    const int kd = SsfBlocks::kind_of(d), f = SsfBlocks::first_of(d), n = SsfBlocks::dim_of(d);
    double *xb = x + f * s;
    if (kd == SSG_LOCAL_LINEAR_TREND) {
      xb[0] = xb[0] + xb[s];
    } else if (kd == SSG_SEMILOCAL) {
      // (level, slope, mean) -> (level + slope, phi slope + (1 - phi) mean, mean)
      const double ph = s_phi[SsfBlocks::arx_of(d) * AR_MAX];
      const double v0 = xb[0], v1 = xb[s], v2 = xb[2 * s];
      xb[0] = v0 + v1;
      xb[s] = ph * v1 + (1 - ph) * v2;
    } else if (kd == SSG_TRIG) {
      for (int q = 0; q < n; q += 2) {
        const double c = s_tc[f + q], sn = s_ts[f + q];
        const double x0 = xb[q * s], x1 = xb[(q + 1) * s];
        xb[q * s] = c * x0 + sn * x1;
        xb[(q + 1) * s] = -sn * x0 + c * x1;
      }
    } else if (kd == SSG_SEASONAL) {
      if ((mv >> b) & 1u) {
        // first = -(sum over the block), the others move down one place
        double prev = xb[0], tot = prev;
        for (int q = 1; q < n; ++q) {
          const double cur = xb[q * s];
          tot += cur;
          xb[q * s] = prev;
          prev = cur;
        }
        xb[0] = -tot;
      }
    } else if (kd == SSG_AR) {
      // first = phi'x, the others move down one place
      const double *ph = s_phi + SsfBlocks::arx_of(d) * AR_MAX;
      double prev = xb[0], tot = ph[0] * prev;
      for (int q = 1; q < n; ++q) {
        const double cur = xb[q * s];
        tot += ph[q] * cur;
        xb[q * s] = prev;
        prev = cur;
      }
      xb[0] = tot;
    }
  }
}

// the variance one lane's diagonal entry of P gains with RQR_t: its own every step (a Student trend's divided by
// the step's weight), a seasonal's first component where the block moves at t, a holiday's entry where the
// calendar's entry t + 1 puts the block
__device__ __forceinline__ double ssf_rqr_diag(double qdiag, int stu, double wl, double ws, int seas_first, unsigned mv,
                                               double seas_var, bool hgain, double hvar) {
  double q = qdiag;
  if (stu) q = qdiag / (stu == 1 ? wl : ws);
  if (seas_first >= 0 && ((mv >> seas_first) & 1u)) q = seas_var;
  if (hgain) q = hvar;
  return q;
}

// HOLDOUT = false: the in-sample filter (ba_ss_prediction_errors).  HOLDOUT = true: the same steps over the
// caller's h rows behind the series (ba_ss_holdout_prediction_errors; ss_filter_params.h says what the
// parameters mean there): the prologue and the step loop are the in-sample ones on a time base of the series'
// length; what differs is the initial condition -- a = T_{T-1} alpha, P = RQR_{T-1} --, that every step is
// observed and that there is no log likelihood.
template <bool HOLDOUT>
__global__ __launch_bounds__(WAVE) void ss_filter_kernel(SsFilterParams P) {
  extern __shared__ double s_P[];   // m x ld
  __shared__ double s_phi[SSG_MAX_AR * AR_MAX], s_var[SSG_MAX_VAR], s_tc[SSG_MAX_STATE], s_ts[SSG_MAX_STATE];
  const int lane = (int)threadIdx.x, row = (int)blockIdx.x;
  if (row >= P.chain_count) return;
  const int64_t chain = (int64_t)P.chain_first + row;
  const int T = P.T, p = P.p, m = P.m, ld = P.ld;
  const SsgSpec &Q = *P.spec;
  const int time0 = HOLDOUT ? P.time0 : 0;   // the time of row 0
  double *err = P.errors + (size_t)row * T;
  double *var_out = P.variances ? P.variances + (size_t)row * T : nullptr;

  // ---- y* = y - X beta over the included coefficients, a step per lane; the included columns
  // are listed 64 candidates at a time (lane k: the k-th of them and its coefficient)
  {
    const uint8_t *gam = P.src.gamma + chain * P.src.gamma_stride;
    const double *bet = P.src.beta + chain * P.src.beta_stride;
    for (int t0 = 0; t0 < T; t0 += WAVE)
      if (t0 + lane < T) err[t0 + lane] = P.y[(size_t)chain * (size_t)P.y_stride + t0 + lane];
    for (int j0 = 0; j0 < p; j0 += WAVE) {
      const int jl = j0 + lane;
      const bool inc = jl < p && gam[jl] != 0;
      const unsigned long long incmask = __ballot(inc);
      if (!incmask) continue;
      const int cnt = __popcll(incmask);
      // lane k <- the k-th included column of the batch (ascending)
      const int rank = __popcll(incmask & ((1ull << lane) - 1ull));
      __shared__ int s_idx[WAVE];
      __shared__ double s_beta[WAVE];
      if (inc) { s_idx[rank] = jl; s_beta[rank] = bet[jl]; }
      wave_lds_sync();
      for (int t0 = 0; t0 < T; t0 += WAVE) {
        const int t = t0 + lane;
        if (t < T) {
          double ys = err[t];
          for (int k = 0; k < cnt; ++k) ys -= P.X[(size_t)s_idx[k] * T + t] * s_beta[k];
          err[t] = ys;
        }
      }
      wave_lds_sync();
    }
  }

  // ---- the chain's parameters and the block list
  if (lane < P.nvar) s_var[lane] = P.src.var[chain * P.src.var_stride + lane];
  if (P.src.phi && lane < P.nar * AR_MAX) s_phi[lane] = P.src.phi[chain * P.src.phi_stride + lane];
  s_tc[lane] = lane < m ? Q.trig_c[lane] : 0.0;
  s_ts[lane] = lane < m ? Q.trig_s[lane] : 0.0;
  const double sigsq = P.src.sigsq[chain * P.src.sigsq_stride];
  SsfBlocks B;
  B.nb = P.nblocks;
  B.desc = 0;
  int dur = 1, rc = 1;   // lane b, seasonal block b: its duration; (index of the step's transition + 1 - phase) mod duration (0: it moves)
  bool calb = false;     // lane b: block b is a calendar seasonal -- it moves where the calendar's entry t + 1 says so
  if (lane < P.nblocks) {
    const SsgBlock &K = Q.blk[lane];
    B.desc = SsfBlocks::pack(K) | ((unsigned)(K.nvar > 0 ? 1 : 0) << 25);
    calb = ssg_is_calendar(K);
    if (K.kind == SSG_SEASONAL) {
      dur = K.duration;
      rc = (time0 + 1 - K.phase) % dur;
      if (rc < 0) rc += dur;
    }
  }
  const unsigned seasmask = (unsigned)__ballot(SsfBlocks::kind_of(B.desc) == SSG_SEASONAL);
  // blocks whose transition is never the identity
  const unsigned always =(unsigned)__ballot(SsfBlocks::kind_of(B.desc) == SSG_LOCAL_LINEAR_TREND ||
                                            SsfBlocks::kind_of(B.desc) == SSG_AR || SsfBlocks::kind_of(B.desc) == SSG_TRIG ||
                                            SsfBlocks::kind_of(B.desc) == SSG_SEMILOCAL);
  wave_lds_sync();
  // per lane: is the component one Z selects; the variance its diagonal entry gains every step;
  // the seasonal block it is the first component of (-1: none); its part in a Student trend (1 level, 2 slope)
  bool zsel = false;
  double qdiag = 0.0, seas_var = 0.0, a = 0.0, P0l = 0.0;
  int seas_first = -1, stu = 0;
  // a random-walk holiday's lanes: Z_t and the entry that gains the variance move with the calendar
  // (position of the lane's block = byte hsh / 8 of the step's entry; T is the identity)
  bool hol = false;
  int hsh = 0, hfirst = 0;
  double hvar = 0.0;
  // a dynamic regression's lanes (P.dyn): Z_t's entry is the lane's predictor at t -- column dcol of the
  // table's row t --, T is the identity and the lane's own variance is added every step
  bool dr = false;
  int dcol = 0;
  for (int b = 0; b < B.nb; ++b) {
    const unsigned d = B.at(b);
    const int kd = SsfBlocks::kind_of(d), f = SsfBlocks::first_of(d), n = SsfBlocks::dim_of(d), v0 = SsfBlocks::var0_of(d);
    if (lane < f || lane >= f + n) continue;
    const int w = lane - f;
    zsel = kd == SSG_TRIG ? (w & 1) == 0 : w == 0;
    const bool student = b == Q.student_block - 1;
    if (kd == SSG_LOCAL_LEVEL) qdiag = SsfBlocks::has_var(d) ? s_var[v0] : 0.0;
    else if (kd == SSG_LOCAL_LINEAR_TREND) { qdiag = s_var[v0 + w]; if (student) stu = 1 + w; }
    else if (kd == SSG_SEMILOCAL) qdiag = w < 2 ? s_var[v0 + w] : 0.0;
    else if (kd == SSG_TRIG) qdiag = s_var[v0];
    else if (kd == SSG_AR) qdiag = w == 0 ? s_var[v0] : 0.0;
    else if (kd == SSG_SEASONAL) { if (w == 0) { seas_first = b; seas_var = s_var[v0]; } }
    if (kd == SSG_LOCAL_LEVEL && Q.blk[b].holiday) {
      hol = true; hsh = 8 * b; hfirst = f; hvar = s_var[v0];
      zsel = false;
      qdiag = 0.0;
    }
    if (kd == SSG_LOCAL_LEVEL && P.dyn && Q.blk[b].dynreg) {
      dr = true; dcol = Q.blk[b].dynreg - 1 + w;
      zsel = false;
      qdiag = s_var[v0 + w];
    }
    // (one coefficient of an AR dynamic regression: the autoregression's first component reads the block's column)
    if (kd == SSG_AR && P.dyn && Q.blk[b].dynreg && w == 0) {
      dr = true; dcol = Q.blk[b].dynreg - 1;
      zsel = false;
    }
    a = Q.a0[lane];
    // (a semilocal trend's third component IS the slope's long-run mean)
    if (kd == SSG_SEMILOCAL && w == 2) a = s_phi[SsfBlocks::arx_of(d) * AR_MAX + 1];
    P0l = Q.P0[lane];
  }
  const unsigned long long zmask = __ballot(zsel && lane < m);
  const unsigned long long drmask = __ballot(dr && lane < m);
  // (the lane's predictor of the step, and the next step's on its way while this one is worked on)
  double xw = 0.0, xn = 0.0;
  if (dr) xn = P.dyn[(size_t)time0 * P.dyn_cols + dcol];
  const bool act = lane < m;
  for (int e = lane; e < m * ld; e += WAVE) s_P[e] = 0.0;
  wave_lds_sync();
  if (!HOLDOUT) {
    if (act) s_P[lane * ld + lane] = P0l;
  } else {
    // a = T_{T-1} alpha, by one lane on column m; P = RQR_{T-1}: the step T - 1 moves a seasonal where time T
    // starts a season, and a holiday gains its variance at the position of entry T
    const unsigned long long c0 = P.cal ? P.cal[time0] : (unsigned long long)SSG_CAL_NONE;
    const bool calmove0 = calb && ((c0 >> (8 * (lane & 7))) & (unsigned long long)SSG_CAL_SEASON) != 0;
    const unsigned mv0 = (unsigned)__ballot(lane < B.nb && SsfBlocks::kind_of(B.desc) == SSG_SEASONAL &&
                                            (calb ? calmove0 : rc == (dur == 1 ? 0 : 1))) & seasmask;
    if (act) s_P[lane * ld + m] = P.state[chain * P.state_stride + lane];
    wave_lds_sync();
    if (lane == 0) ssf_apply_T(B, mv0, s_phi, s_tc, s_ts, s_P + m, ld);
    wave_lds_sync();
    if (act) {
      a = s_P[lane * ld + m];
      const bool hgain0 = hol && lane == hfirst + (int)((c0 >> hsh) & 0xffu);
      s_P[lane * ld + lane] = ssf_rqr_diag(qdiag, 0, 1.0, 1.0, seas_first, mv0, seas_var, hgain0, hvar);
    }
  }
  wave_lds_sync();

  const double *qw = P.qw ? P.qw + chain * P.qw_stride : nullptr;
  const double nan = __builtin_nan("");
  double ll = 0.0;
  bool dead = false;
  for (int tb = 0; tb < T; tb += WAVE) {
    const int tt = tb + lane;
    const double ys_l = tt < T ? err[tt] : 0.0;
    const unsigned long long obsmask = __ballot(tt < T && (HOLDOUT || P.observed[tt] != 0));
    double wl_l = 1.0, ws_l = 1.0;
    if (qw && tt < T) { wl_l = qw[tt]; ws_l = qw[(size_t)T + tt]; }
    double v_l = 0.0, F_l = 0.0;
    // (the calendar's entries t -- Z_t -- and t + 1 -- RQR_t -- of the block's steps, one per lane)
    unsigned long long cw_l = SSG_CAL_NONE, cn_l = SSG_CAL_NONE;
    // (entry and row time0 + T are never read: the last step's transition feeds nothing)
    if (P.cal) { if (tt < T) cw_l = P.cal[time0 + tt]; if (tt + 1 < T) cn_l = P.cal[time0 + tt + 1]; }
    const int ns = T - tb < WAVE ? T - tb : WAVE;
    for (int s = 0; s < ns; ++s) {
      const bool obs = ((obsmask >> s) & 1ull) != 0;
      double vout = nan, F = nan;
      unsigned long long zmask_t = zmask;
      bool hgain = false;   // this lane's diagonal entry gains the holiday's variance at this step
      bool calmove = false; // lane b: calendar seasonal b steps into a new season
      if (P.cal) {
        const unsigned long long cw = __builtin_bit_cast(unsigned long long, rl(__builtin_bit_cast(double, cw_l), s));
        const unsigned long long cn = __builtin_bit_cast(unsigned long long, rl(__builtin_bit_cast(double, cn_l), s));
        calmove = calb && ((cn >> (8 * (lane & 7))) & (unsigned long long)SSG_CAL_SEASON) != 0;
        zmask_t |= __ballot(hol && lane == hfirst + (int)((cw >> hsh) & 0xffu));
        hgain = hol && lane == hfirst + (int)((cn >> hsh) & 0xffu);
      }
      if (P.dyn) {
        xw = xn;
        if (dr && tb + s + 1 < T) xn = P.dyn[(size_t)(time0 + tb + s + 1) * P.dyn_cols + dcol];
      }
      if (!dead) {
        // PZ, F, v
        double pz = 0.0;
        if (act) {
          const double *prow = s_P + lane * ld;
          for (unsigned long long zm = zmask_t; zm; zm &= zm - 1) pz += prow[__builtin_ctzll(zm)];
        }
        for (unsigned long long zm = drmask; zm; zm &= zm - 1) {   // (Z_t = x_t on these components)
          const int j = __builtin_ctzll(zm);
          const double xj = rl(xw, j);
          if (act) pz += xj * s_P[lane * ld + j];
        }
        double za = 0.0, zpz = 0.0;
        for (unsigned long long zm = zmask_t; zm; zm &= zm - 1) {
          const int j = __builtin_ctzll(zm);
          za += rl(a, j);
          zpz += rl(pz, j);
        }
        for (unsigned long long zm = drmask; zm; zm &= zm - 1) {
          const int j = __builtin_ctzll(zm);
          const double xj = rl(xw, j);
          za += xj * rl(a, j);
          zpz += xj * rl(pz, j);
        }
        F = zpz + sigsq;
        if (!(F > 0.0) || !(F <= 1.79769313486231570815e308)) {
          // "Found a zero (or negative) forecast variance!": the chain's outputs are NaN from here on
          dead = true;
          F = nan;
          if (lane == 0) atomicMin(P.flag, (int)chain);
        } else {
          const double ys = rl(ys_l, s);
          const double v = obs ? ys - za : 0.0;
          const double Finv = 1.0 / F;
          if (obs) {
            if (act) {
              a += pz * (v * Finv);
              double *prow = s_P + lane * ld;
              for (int j = 0; j < m; ++j) prow[j] -= (pz * rl(pz, j)) * Finv;
            }
          }
          vout = v;
          // a <- T a, P <- T P T' + RQR
          const unsigned mv = (unsigned)__ballot(lane < B.nb && SsfBlocks::kind_of(B.desc) == SSG_SEASONAL && (calb ? calmove : rc == 0)) & seasmask;
          if (always | mv) {
            if (act) s_P[lane * ld + m] = a;
            wave_lds_sync();
            for (int c = lane; c <= m; c += WAVE) ssf_apply_T(B, mv, s_phi, s_tc, s_ts, s_P + c, ld);
            wave_lds_sync();
            if (act) {
              ssf_apply_T(B, mv, s_phi, s_tc, s_ts, s_P + lane * ld, 1);
              a = s_P[lane * ld + m];
            }
            wave_lds_sync();
            // (the two passes agree only up to rounding: the upper triangle is the variance)
            if (act)
              for (int j = 0; j < lane; ++j) s_P[lane * ld + j] = s_P[j * ld + lane];
          }
          // (the step's Student-trend weights: every lane reads them, the trend's two lanes use them)
          const double wl = rl(wl_l, s), ws = rl(ws_l, s);
          if (act) {
            const double q = ssf_rqr_diag(qdiag, stu, wl, ws, seas_first, mv, seas_var, hgain, hvar);
            if (q != 0.0) s_P[lane * ld + lane] += q;
          }
          wave_lds_sync();
        }
      }
      if (lane < B.nb) { rc = rc + 1 == dur ? 0 : rc + 1; }
      if (lane == s) { v_l = vout; F_l = F; }
    }
    // the block's log likelihood terms and standardised errors, a step per lane; the terms are
    // summed in step order
    const bool ob_l = ((obsmask >> lane) & 1ull) != 0;
    if (!HOLDOUT) {
      const double term = ob_l ? -0.5 * (1.8378770664093454835606594728112 + log(F_l) + v_l * v_l / F_l) : 0.0;
      for (int s = 0; s < ns; ++s) ll += rl(term, s);
    }
    if (tt < T) {
      err[tt] = (P.standardize && ob_l) ? v_l / sqrt(F_l) : v_l;
      if (var_out) var_out[tt] = F_l;
    }
  }
  if (!HOLDOUT && lane == 0) P.loglik[row] = dead ? nan : ll;
}

}  // namespace

// One instance per translation unit: a second kernel in this one changes the code the compiler makes for the
// first (its register allocation), and the in-sample instance is kept byte-stable.  This file makes the
// in-sample instance; ss_filter_holdout_kernel.hip defines SS_FILTER_HOLDOUT_UNIT, includes this file and makes
// the holdout instance from the same source.
#ifndef SS_FILTER_HOLDOUT_UNIT
size_t ss_filter_lds(int m, int ld) { return (size_t)m * ld * sizeof(double); }

hipError_t launch_ss_filter(hipStream_t stream, const SsFilterParams &P) {
  if (P.chain_count <= 0) return hipSuccess;
  KtScope kt(stream, KT_SS_FILTER);
  hipLaunchKernelGGL(ss_filter_kernel<false>, dim3((unsigned)P.chain_count), dim3(WAVE), ss_filter_lds(P.m, P.ld), stream, P);
  return hipGetLastError();
}
#else
hipError_t launch_ss_filter_holdout(hipStream_t stream, const SsFilterParams &P) {
  if (P.chain_count <= 0) return hipSuccess;
  KtScope kt(stream, KT_SS_FILTER);
  hipLaunchKernelGGL(ss_filter_kernel<true>, dim3((unsigned)P.chain_count), dim3(WAVE), ss_filter_lds(P.m, P.ld), stream, P);
  return hipGetLastError();
}
#endif

}  // namespace boom_amd
