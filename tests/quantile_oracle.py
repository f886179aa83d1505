"""A restatement of QuantileRegressionSpikeSlabSampler::draw() on the device's substreams, in
Python over the oracle's primitives (oracle_lib.Oracle): the parity yardstick of
ba_quantile_sweep.

One draw() (Models/Glm/PosteriorSamplers/QuantileRegressionPosteriorSampler.cpp:30-39, :77-91):
  1. for every observation r_i = |y_i - x_i'beta|.  If r_i > 0: lambda_inv = rig_mt(rng,
     1 / r_i, 1.0) (distributions/inverse_gaussian.cpp:59-69: one normal, then one uniform),
     and the weighted suf takes (x_i, y*_i, w_i) with w_i = lambda_inv and
     y*_i = y_i - (2 (1 - q) - 1) / lambda_inv.  If r_i == 0 the observation is left out and
     nothing is read from the RNG.  Observation i of sweep s reads stream 32 from slot
     s n + i of 256 (spill as the oracle's bo_rng_slot does).
  2. SpikeSlabSampler::draw_model_indicators / draw_beta at sigma^2 = 1 on that suf, with a
     fixed-precision slab (the oracle's bo_sss, slab_kind 0).  SpikeSlabSampler keeps no state
     besides gamma, beta and its RNG, so a bo_sss built per sweep with those three carried
     over is the same sampler.  Stream 3.
There is no sigma^2 and no nu.

The one deviation from the reference's arithmetic: rig_mt forms the smaller root of its
quadratic as mu + mu y mu2lam - mu2lam sqrt(mu y (4 lambda + mu y)), which cancels when
t = mu y / (2 lambda) is large -- a small residual.  smaller_root() is the algebraically
identical mu / (1 + t + sqrt(t (2 + t))), as the device kernel has it (tests/test_quantile_cpu.py
holds both forms to a 60-digit evaluation).  reference_root() is the reference's form, kept
for that comparison.
"""
import ctypes as C

import numpy as np

from oracle_lib import BoRng, _dp, _u8, f64, fcol

IMPUTE_STREAM, IMPUTE_STRIDE = 32, 256


def smaller_root(mu, y, lam=1.0):
    """the smaller root of rig_mt's quadratic, without the cancellation"""
    t = mu * y / (2 * lam)
    return mu / (1 + t + np.sqrt(t * (2 + t)))


def reference_root(mu, y, lam=1.0):
    """the same root as inverse_gaussian.cpp:62-65 writes it"""
    muy = mu * y
    mu2lam = .5 * mu / lam
    return mu + muy * mu2lam - mu2lam * np.sqrt(muy * (4 * lam + muy))


def rig(mu, lam, z, u, root=smaller_root):
    """rig_mt given its normal z and its uniform u (scalars or arrays)"""
    x = root(mu, z * z, lam)
    return np.where(u > mu / (mu + x), mu * mu / x, x)


def impute_point(y, eta, shift, norm, unif, rig=rig):
    """(w, z, t) of one observation: w = lambda_inv, z = w y* = w y - shift with
    shift = 1 - 2 q, t the root's argument; norm() / unif() read the observation's slot, and
    are not called when the residual is 0 or 1 / r is not finite.  rig: the inverse-Gaussian draw
    given its normal and uniform (tests/latent_ref.py passes this module's on another math table)"""
    r = abs(y - eta)
    with np.errstate(divide="ignore", over="ignore"):
        mu = np.float64(1.0) / np.float64(r)
    if not (r > 0 and np.isfinite(mu)):
        return 0.0, 0.0, 0.0
    zn = norm()
    u = unif()
    w = float(rig(mu, 1.0, zn, u))
    return w, w * y - shift, float(mu * (zn * zn) / 2)


class QuantileOracle:
    """One chain of QuantileRegressionSpikeSlabSampler on the device's substreams."""

    def __init__(self, o, X, y, quantile, mu, prec, pi, seed, chain, gamma0, beta0=None, max_flips=-1,
                 max_model_size=-1):
        self.o, self.L = o, o.lib
        o._declare_sss()
        L = self.L
        L.bo_rng_slot.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
        L.bo_rng_slot.restype = None
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64)
        self.n, self.p = self.X.shape
        self.q = float(quantile)
        self.shift = 1.0 - 2.0 * self.q
        self.mu, self.prec, self.pi = f64(mu), np.asarray(prec, dtype=np.float64), f64(pi)
        self.seed, self.chain = int(seed), int(chain)
        self.gamma = np.ascontiguousarray(gamma0, dtype=np.uint8).copy()
        self.beta = np.zeros(self.p) if beta0 is None else f64(beta0) * self.gamma
        self.max_flips, self.max_model_size = int(max_flips), int(max_model_size)
        self.sss_rng = BoRng()
        L.bo_rng_seed_philox(C.byref(self.sss_rng), self.seed, self.chain, 3, 0)
        self.sweep = 0
        self.weights = None
        self.residuals = None
        self.max_t = []        # per sweep: the largest t = mu y / (2 lambda)
        self.min_abs_r = []    # per sweep: the smallest non-zero |r|

    def _slot(self, index):
        r = BoRng()
        self.L.bo_rng_seed_philox(C.byref(r), self.seed, self.chain, IMPUTE_STREAM, 0)
        self.L.bo_rng_slot(C.byref(r), int(index), IMPUTE_STRIDE)
        return r

    def impute(self):
        """(w, z) of the sweep about to be drawn; records the residuals, the largest t and the
        smallest non-zero |r|"""
        o, n, s = self.o, self.n, self.sweep
        inc = np.flatnonzero(self.gamma)
        eta = self.X[:, inc] @ self.beta[inc]
        w, z, t = np.zeros(n), np.zeros(n), np.zeros(n)
        for i in range(n):
            rng = self._slot(s * n + i)
            w[i], z[i], t[i] = impute_point(self.y[i], eta[i], self.shift,
                                            lambda: o.norms(rng, 1)[0], lambda: o.uniforms(rng, 1)[0])
        r = np.abs(self.y - eta)
        self.residuals = r
        self.last_max_t = float(t.max())
        self.last_min_abs_r = float(r[r > 0].min()) if np.any(r > 0) else np.inf
        return w, z

    def draw(self):
        L = self.L
        p = self.p
        w, z = self.impute()
        self.weights = w
        self.max_t.append(self.last_max_t)
        self.min_abs_r.append(self.last_min_abs_r)
        xtx = self.X.T @ (self.X * w[:, None])
        xty = self.X.T @ z
        h = L.bo_sss_create(p, _dp(fcol(xtx)), _dp(f64(xty)), 0, _dp(self.mu), _dp(fcol(self.prec)),
                            _dp(self.pi))
        try:
            L.bo_sss_set_options(h, self.max_model_size, self.max_flips)
            L.bo_sss_set_state(h, _u8(self.gamma), _dp(f64(self.beta)))
            C.memmove(L.bo_sss_rng(h), C.byref(self.sss_rng), C.sizeof(BoRng))
            st = L.bo_sss_draw_model_indicators(h, 1.0)
            if st == 0:
                st = L.bo_sss_draw_beta(h, 1.0)
            if st:
                raise RuntimeError("SpikeSlabSampler status %d" % st)
            g = np.zeros(p, dtype=np.uint8)
            b = np.zeros(p)
            L.bo_sss_get_state(h, _u8(g), _dp(b))
            C.memmove(C.byref(self.sss_rng), L.bo_sss_rng(h), C.sizeof(BoRng))
        finally:
            L.bo_sss_destroy(h)
        self.gamma, self.beta = g, b
        self.sweep += 1
        return self.gamma.copy(), self.beta.copy()
