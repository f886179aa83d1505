// Small dense linear algebra of one wavefront, a matrix row per lane, and the three draws built on it:
// a multivariate normal given its precision (RegressionCoefficientSampler::sample_regression_coefficients,
// rmvn_ivar_mt), the Bartlett triangle (WishartTriangle) and rWish_mt -- for d <= MW_MAX.  On top,
// rhh_draw_model: one draw of HierGaussianRegressionAsisSampler for a hierarchical regression holiday
// model (hier_holiday_kernel.hip; tests/cpp/hier_probe.hip runs the same code).
//
// Layout.  A matrix sits in LDS, row-major at leading dimension MW_LD = 17 (a lane per row: rows fall on
// different banks).  Lane r of a group of 16 owns row r; the four groups of a wave work on four matrices
// at once (step 1 of the draw: four holidays in flight), or the wave's first d lanes on one.  A lane
// whose row is >= d takes no part (callers pass r = 64 for a group without work).  Vectors live one
// entry per lane in a register; what a solve hands from lane to lane goes through 16 doubles of LDS.
// Nothing is indexed in registers: no scratch.
//
// Arithmetic.  Every function runs under `fp contract(off)` and every sum has one written order, so the
// results are those of the same loops in IEEE double on any machine (tests/ss_hier_regholiday_oracle.py
// restates them in that order) and do not depend on how many sweeps a call makes:
//   mw_chol      left-looking by column j: s = a_rj - l_r0 l_j0 - l_r1 l_j1 - ... (k ascending);
//                l_jj = sqrt(s), l_rj = s / l_jj
//   mw_forward   x_r = (((b_r - l_r0 x_0) - l_r1 x_1) - ...) / l_rr              (k ascending)
//   mw_backward  x_r = (((b_r - l_{d-1,r} x_{d-1}) - l_{d-2,r} x_{d-2}) - ...) / l_rr   (k descending)
//   mw_inverse   W = L^-1 by columns (lane c: w_ic = ((i == c) - l_ic w_cc - ... - l_{i,i-1} w_{i-1,c}) / l_ii),
//                then A^-1 = W'W: entry (r, c) = w_{k0,r} w_{k0,c} + ... + w_{d-1,r} w_{d-1,c}, k0 = max(r, c)
//   mw_wishart   P = C T: p_rc = c_rc t_cc + ... + c_rr t_rc (k ascending), Omega = P P':
//                entry (r, c) = p_r0 p_c0 + ... + p_rm p_cm, m = min(r, c)
// every sum starting from its first term (the inverse and the products from 0 + the first product).
#pragma once
#include <hip/hip_runtime.h>

#include "device_rng.h"
#include "kalman_params.h"
#include "wave_lanes.h"

namespace boom_amd {

namespace {

enum { MW_MAX = RHH_MAX_WIDTH, MW_LD = MW_MAX + 1, MW_MAT = MW_MAX * MW_LD };

// the LDS of one wavefront's draw
struct MwLds {
  double M[4][MW_MAT];     // a matrix per group of 16 lanes
  double N[MW_MAT], T[MW_MAT];
  double xb[4][MW_MAX];    // the solves' hand-off, per group
  double vec[MW_MAX];
  double z[RH_MAX_COEF];   // step 1's normals, then the centred effects
  double om_in[MW_MAX * MW_MAX], mu_in[MW_MAX];
  // what the chain's draw leaves, written to memory once every model's draw is through
  double beta[RH_MAX_COEF];
  double mu_out[RH_MAX_MODELS][MW_MAX];
  double om_out[RH_MAX_MODELS][MW_MAX * MW_MAX];
};

// M's lower triangle -> its Cholesky factor, in place.  false on the lane whose pivot is not positive
// and finite (the caller votes).
__device__ __forceinline__ bool mw_chol(double *M, int d, int r) {
#pragma clang fp contract(off)
  bool ok = true;
  for (int j = 0; j < d; ++j) {
    double s = 0.0;
    if (r >= j && r < d) {
      s = M[r * MW_LD + j];
      for (int k = 0; k < j; ++k) s = s - M[r * MW_LD + k] * M[j * MW_LD + k];
    }
    if (r == j) {
      ok = s > 0.0 && isfinite(s);
      M[j * MW_LD + j] = sqrt(s);
    }
    wave_lds_sync();
    if (r > j && r < d) M[r * MW_LD + j] = s / M[j * MW_LD + j];
    wave_lds_sync();
  }
  return ok;
}

// L x = v: lane r gives v_r and gets x_r
__device__ __forceinline__ double mw_forward(const double *L, double *xb, int d, int r, double v) {
#pragma clang fp contract(off)
  for (int j = 0; j < d; ++j) {
    if (r == j) {
      v = v / L[j * MW_LD + j];
      xb[j] = v;
    }
    wave_lds_sync();
    if (r > j && r < d) v = v - L[r * MW_LD + j] * xb[j];
  }
  wave_lds_sync();
  return v;
}

// L'x = v
__device__ __forceinline__ double mw_backward(const double *L, double *xb, int d, int r, double v) {
#pragma clang fp contract(off)
  for (int j = d - 1; j >= 0; --j) {
    if (r == j) {
      v = v / L[j * MW_LD + j];
      xb[j] = v;
    }
    wave_lds_sync();
    if (r < j) v = v - L[j * MW_LD + r] * xb[j];
  }
  wave_lds_sync();
  return v;
}

// the factor L in M -> (L L')^-1 in M, whole and symmetric to the bit; N is the workspace (L^-1)
__device__ __forceinline__ void mw_inverse(double *M, double *N, int d, int r) {
#pragma clang fp contract(off)
  if (r < d) {
    // column r of L^-1: the lane reads back what it wrote, no other lane's
    for (int i = r; i < d; ++i) {
      double s = i == r ? 1.0 : 0.0;
      for (int k = r; k < i; ++k) s = s - M[i * MW_LD + k] * N[k * MW_LD + r];
      N[i * MW_LD + r] = s / M[i * MW_LD + i];
    }
  }
  wave_lds_sync();
  if (r < d) {
    for (int c = 0; c < d; ++c) {
      double s = 0.0;
      for (int k = r > c ? r : c; k < d; ++k) s = s + N[k * MW_LD + r] * N[k * MW_LD + c];
      M[r * MW_LD + c] = s;
    }
  }
  wave_lds_sync();
}

// WishartTriangle(rng, d, nu): row by row, sqrt(rchisq(nu - i)) on the diagonal first, then the i normals
// to its left, as the reference draws them.  rchisq(df) = rgamma(df / 2, scale 2) (Bmath/rchisq.cpp).
// Every lane makes every draw; T == nullptr: the numbers are consumed and dropped.
__device__ __forceinline__ void mw_bartlett(SeqRng &rng, int d, double nu, double *T, int lane, int *bad) {
#pragma clang fp contract(off)
  for (int i = 0; i < d; ++i) {
    const double g = d_rgamma_scale(rng, (nu - (double)i) / 2.0, 2.0, bad);
    if (T && lane == 0) T[i * MW_LD + i] = sqrt(g);
    for (int j = 0; j < i; ++j) {
      const double z = d_rnorm(rng, 0.0, 1.0);
      if (T && lane == 0) T[i * MW_LD + j] = z;
    }
  }
  wave_lds_sync();
}

// rWish_mt's product: C (lower, in M) and the triangle T -> (C T)(C T)' at out (leading dimension MW_MAX)
__device__ __forceinline__ void mw_wishart(const double *M, const double *T, double *N, double *out, int d, int r) {
#pragma clang fp contract(off)
  if (r < d) {
    for (int c = 0; c <= r; ++c) {
      double s = 0.0;
      for (int k = c; k <= r; ++k) s = s + M[r * MW_LD + k] * T[k * MW_LD + c];
      N[r * MW_LD + c] = s;
    }
  }
  wave_lds_sync();
  if (r < d) {
    for (int c = 0; c < d; ++c) {
      double s = 0.0;
      const int m = r < c ? r : c;
      for (int k = 0; k <= m; ++k) s = s + N[r * MW_LD + k] * N[c * MW_LD + k];
      out[r * MW_MAX + c] = s;
    }
  }
  wave_lds_sync();
}

// the draw N(A^-1 b, A^-1) of sample_regression_coefficients: A's lower triangle in M (the factor is left
// there), lane r gives b_r and its normal z_r and gets its entry: L'^-1 z + L'^-1 L^-1 b
__device__ __forceinline__ double mw_mvn_draw(double *M, double *xb, int d, int r, double b, double z, bool *ok) {
#pragma clang fp contract(off)
  *ok = mw_chol(M, d, r);
  const double m = mw_backward(M, xb, d, r, mw_forward(M, xb, d, r, b));
  const double e = mw_backward(M, xb, d, r, z);
  return e + m;
}

// d normals in order, every lane drawing every one: lane r keeps the r-th
__device__ __forceinline__ double mw_normals(SeqRng &rng, int d, int r) {
  double mine = 0.0;
  for (int i = 0; i < d; ++i) {
    const double z = d_rnorm(rng, 0.0, 1.0);
    if (i == r) mine = z;
  }
  return mine;
}

// One draw of HierGaussianRegressionAsisSampler::draw for one model (the steps are the reference's, see
// DESIGN 3.26): H holidays of width d at the flat coefficients base .. base + H d - 1 of the list, counts
// and totals there (global memory), mu_g / om_g the chain's current hyper-mean and hyper-precision,
// hyper the model's RHH_HYPER_* block.  Leaves beta at W.beta[base ..], mu at mu_out, Omega at om_out;
// returns false (on every lane) where a factor was not positive definite or a result not finite.
__device__ __forceinline__ bool rhh_draw_model(MwLds &W, SeqRng &rng, int lane, int d, int H, int base, double sigsq,
                                               double nu0, const double *counts, const double *totals,
                                               const double *mu_g, const double *om_g, const double *hyper,
                                               double *mu_out, double *om_out) {
#pragma clang fp contract(off)
  const int g = lane >> 4, r16 = lane & 15;
  int bad = 0;
  bool ok = true, okk;
  for (int i = lane; i < d * d; i += WAVE) W.om_in[(i / d) * MW_MAX + i % d] = om_g[(i / d) * MW_MAX + i % d];
  if (lane < d) W.mu_in[lane] = mu_g[lane];
  // step 1: every holiday's normals in order, then four holidays at a time
  for (int i = 0; i < H * d; ++i) {
    const double z = d_rnorm(rng, 0.0, 1.0);
    if (lane == 0) W.z[i] = z;
  }
  wave_lds_sync();
  double om_mu = 0.0;   // (Omega mu)_r
  if (r16 < d)
    for (int c = 0; c < d; ++c) om_mu = om_mu + W.om_in[r16 * MW_MAX + c] * W.mu_in[c];
  for (int h0 = 0; h0 < H; h0 += 4) {
    const int h = h0 + g;
    const int r = (h < H && r16 < d) ? r16 : WAVE;
    double *M = W.M[g];
    double b = 0.0, z = 0.0;
    if (r < d) {
      const int j = base + h * d + r;
      for (int c = 0; c <= r; ++c) M[r * MW_LD + c] = W.om_in[r * MW_MAX + c];
      M[r * MW_LD + r] = counts[j] / sigsq + W.om_in[r * MW_MAX + r];
      b = totals[j] / sigsq + om_mu;
      z = W.z[h * d + r];
    }
    wave_lds_sync();
    const double v = mw_mvn_draw(M, W.xb[g], d, r, b, z, &okk);
    ok = ok && okk;
    if (r < d) W.beta[base + h * d + r] = v;
  }
  wave_lds_sync();
  // step 2 (a), MvnMeanSampler::draw: the wave's first d lanes on one matrix from here on
  const int r = lane < d ? lane : WAVE;
  double *M = W.M[0], *xb = W.xb[0];
  const double *Sinv0 = hyper + RHH_HYPER_SINV0, *S0 = hyper + RHH_HYPER_S0, *Sinv0mu0 = hyper + RHH_HYPER_SINV0MU0;
  const double n = (double)H;
  if (r < d) {
    double bar = 0.0;   // MvnSuf::update_raw's running mean
    for (int h = 0; h < H; ++h) {
      const double w = (W.beta[base + h * d + r] - bar) / (double)(h + 1);
      bar = bar + w;
    }
    W.vec[r] = bar;
    for (int c = 0; c <= r; ++c) M[r * MW_LD + c] = n * W.om_in[r * MW_MAX + c] + Sinv0[r * MW_MAX + c];
  }
  wave_lds_sync();
  double b = 0.0;
  if (r < d) {
    double s = 0.0;
    for (int c = 0; c < d; ++c) s = s + W.om_in[r * MW_MAX + c] * W.vec[c];
    b = n * s + Sinv0mu0[r];
  }
  double z = mw_normals(rng, d, r);
  const double mu1 = mw_mvn_draw(M, xb, d, r, b, z, &okk);   // mu'
  ok = ok && okk;
  // step 2 (b), MvnVarSampler::draw: its precision is overwritten below without being read; its numbers
  // are consumed (its matrix is the one of step 3: a failure there is found there)
  mw_bartlett(rng, d, nu0 + n, nullptr, lane, &bad);
  // step 3: centred at mu'
  double xtx = 0.0, xty = 0.0;
  if (r < d) {
    for (int h = 0; h < H; ++h) {
      const int j = base + h * d + r;
      const double c = W.beta[j] - mu1;
      W.z[h * d + r] = c;
      xtx = xtx + counts[j];
      xty = xty + (totals[j] - counts[j] * c);
    }
    for (int c = 0; c <= r; ++c) M[r * MW_LD + c] = Sinv0[r * MW_MAX + c];
    M[r * MW_LD + r] = xtx / sigsq + Sinv0[r * MW_MAX + r];
    b = xty / sigsq + Sinv0mu0[r];
  }
  wave_lds_sync();
  z = mw_normals(rng, d, r);
  const double mu2 = mw_mvn_draw(M, xb, d, r, b, z, &okk);
  ok = ok && okk;
  if (r < d) {
    for (int c = 0; c <= r; ++c) {
      double s = 0.0;
      for (int h = 0; h < H; ++h) s = s + W.z[h * d + r] * W.z[h * d + c];
      M[r * MW_LD + c] = s + S0[r * MW_MAX + c];
    }
  }
  wave_lds_sync();
  okk = mw_chol(M, d, r);
  ok = ok && okk;
  mw_inverse(M, W.N, d, r);
  okk = mw_chol(M, d, r);
  ok = ok && okk;
  mw_bartlett(rng, d, nu0 + n, W.T, lane, &bad);
  mw_wishart(M, W.T, W.N, om_out, d, r);
  if (r < d) {
    mu_out[r] = mu2;
    ok = ok && isfinite(mu2);
    for (int c = 0; c < d; ++c) ok = ok && isfinite(om_out[r * MW_MAX + c]);
    for (int h = 0; h < H; ++h) ok = ok && isfinite(W.beta[base + h * d + r]);
  }
  wave_lds_sync();
  return __ballot(!ok) == 0ull && bad == 0;
}

}  // namespace

}  // namespace boom_amd
