"""A restatement of TRegressionSpikeSlabSampler::draw() on the device's substreams, in Python
over the oracle's primitives (oracle_lib.Oracle): the parity yardstick of ba_student_sweep.

One draw() (Models/Glm/PosteriorSamplers/TRegressionSpikeSlabSampler.cpp:41-47):
  1. impute_latent_data (TRegressionSampler.cpp:124-140, TDataImputer.cpp:26-30): for every
     observation delta_i = (y_i - x_i'beta) / sigma and w_i = rgamma(shape (nu + 1) / 2,
     rate (nu + delta_i^2) / 2); the weighted suf (X'WX, X'Wy, y'Wy) from (x_i, y_i, w_i).
     Observation i of sweep s reads stream 31 from slot s n + i of 256 (spill as the
     oracle's bo_rng_slot does).
  2. SpikeSlabSampler::draw_model_indicators / draw_beta given sigma^2 on that suf, slab
     precision scaling with sigma^2 (the oracle's bo_sss, slab_kind 1).  SpikeSlabSampler
     keeps no state besides gamma, beta and its RNG (SpikeSlabSampler.cpp:40-82), so a
     bo_sss built per sweep with those three carried over is the same sampler.  Stream 3.
  3. sigma^2 (TRegressionSampler.cpp:160-166, GenericGaussianVarianceSampler.cpp:44-63):
     DF = n + prior df, SS = wsse + prior ss with wsse = beta'X'WX beta - 2 beta'X'Wy + y'Wy
     (WeightedRegressionModel.cpp:206-208); 1 / Gamma(DF/2, SS/2), truncated when sigma has
     an upper limit.  Stream 15, slot s of 4096.
  4. nu (TRegressionSampler.cpp:173-176): ScalarSliceSampler (Samplers/ScalarSliceSampler.cpp)
     with lower limit 0, unimodal = false, the sampler's own suggested_dx (initially 1), on
     log prior(nu) + sum_i dstudent(y_i, x_i'beta, sigma, nu, log) at the new beta and
     sigma^2 (TRegression.cpp:74-86, student_fix.cpp:28-42).  The same stream as sigma^2,
     after it.

rng_setup=("mt", seed) swaps only the random-number provider for the reference's layout
(oracle/ref_driver.cpp ref_student_run, the golden fixtures tests/golden/student_*.npz): one
MT19937-64 stream, the sampler's, seeded from GlobalRng(seed) (PosteriorSampler's
seed_rng), read in draw() order -- the n weights, the SpikeSlabSampler draws, sigma^2, then
the slice sampler's exponential and uniforms.  The arithmetic is the same code path in
both modes, so the golden pins the substream mode the device is compared with.

wsse="exact" forms sigma^2's sum of squares as fsum_i w_i r_i^2 over residuals
r_i = fsum(y_i, -x_ij beta_j) instead of the reference's suf form (the yardstick of the
device's direct sum at a large offset in y); "suf" (the default) is the reference's.
"""
import ctypes as C
import math

import numpy as np
from scipy.special import gammaln

from oracle_lib import BoRng, _dp, _u8, f64, fcol

IMPUTE_STREAM, SN_STREAM = 31, 15
IMPUTE_STRIDE, SN_STRIDE = 256, 4096


class SliceError(RuntimeError):
    pass


def nu_log_prior(nu, prior):
    kind, a, b = prior
    if kind == 0:
        return -np.inf if (nu > b or nu < a) else np.log(1.0 / (b - a))
    if not nu > 0:
        return -np.inf
    return a * np.log(b) - gammaln(a) + (a - 1) * np.log(nu) - b * nu


def nu_log_post(nu, u, n_log_sigma, prior):
    """log prior(nu) + sum_i [dt(t_i, nu, log) - log sigma], u_i = t_i^2 (dt in closed form)"""
    lp = nu_log_prior(nu, prior)
    if lp == -np.inf:
        return lp
    n = len(u)
    c = gammaln(0.5 * (nu + 1)) - gammaln(0.5 * nu) - 0.5 * np.log(nu * np.pi)
    return lp + (n * c - n_log_sigma) - 0.5 * (nu + 1) * float(np.sum(np.log1p(u / nu)))


def slice_draw_nu(unif, rexp1, logf, x, dx, stats=None, fused=None):
    """ScalarSliceSampler::draw for a target bounded below at 0 (find_limits ->
    find_upper_limit with its random extra doublings, then shrink).  unif() / rexp1() read
    the sampler's stream.  Returns (new x, new suggested_dx, smallest relative margin of the
    slice comparisons).  stats (a dict): gets the number of doublings and of shrinks, and the
    margin so far where the sampler raises; fused: what a device that rounds the candidate's
    lo + (hi - lo) u once makes of it (tests/latent_ref.py's replays)."""
    margin = [np.inf]
    stats = {} if stats is None else stats
    stats.update(doublings=0, shrinks=0, margin=np.inf)

    def note(a, b):
        if np.isfinite(a) and np.isfinite(b):
            margin[0] = min(margin[0], abs(a - b) / max(abs(a), abs(b), 1e-300))
            stats["margin"] = margin[0]

    logp_slice = logf(x) - rexp1()
    if not np.isfinite(logp_slice):
        raise SliceError("initial value leads to infinite probability")
    lo, hi = 0.0, x + dx
    logphi = logf(hi)
    note(logphi, logp_slice)
    doublings = 0
    while logphi >= logp_slice or unif() > .5:
        hi = x + 2 * (hi - x)
        if not np.isfinite(hi):
            raise SliceError("infinite upper limit")
        logphi = logf(hi)
        note(logphi, logp_slice)
        doublings += 1
        stats["doublings"] = doublings
        if doublings > 100:
            raise SliceError("more than 100 doublings")
    if np.isnan(logphi):
        raise SliceError("upper limit gives NaN probability")
    tries = 0
    while True:
        cand = lo + (hi - lo) * unif()
        if fused is not None and lo != 0.0:
            cand = fused(cand)
        lp = logf(cand)
        note(lp, logp_slice)
        if not lp < logp_slice:
            return cand, dx, margin[0]
        if cand > x:
            hi = cand
        else:
            lo = cand
        dx = hi - lo
        tries += 1
        stats["shrinks"] = tries
        if tries > 100:
            raise SliceError("number of tries exceeded")


class StudentOracle:
    """One chain of TRegressionSpikeSlabSampler on the device's substreams (rng_setup=("mt", seed):
    on the reference's one stream; seed and chain are then not read)."""

    def __init__(self, o, X, y, mu, prec, pi, seed, chain, gamma0, beta0=None, sigsq0=1.0,
                 nu0=30.0, nu_prior=(0, 0.1, 100.0), sigma_prior=(1.0, 1.0),
                 sigma_max=np.inf, max_flips=-1, max_model_size=-1, allow_selection=True,
                 rng_setup=None, wsse="suf"):
        self.o, self.L = o, o.lib
        o._declare_sss()
        L = self.L
        L.bo_rng_slot.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
        L.bo_rng_slot.restype = None
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64)
        self.n, self.p = self.X.shape
        self.mu, self.prec, self.pi = f64(mu), np.asarray(prec, dtype=np.float64), f64(pi)
        self.seed, self.chain = int(seed), int(chain)
        self.gamma = np.ascontiguousarray(gamma0, dtype=np.uint8).copy()
        self.beta = np.zeros(self.p) if beta0 is None else f64(beta0) * self.gamma
        self.sigsq, self.nu, self.dx = float(sigsq0), float(nu0), 1.0
        self.nu_prior = nu_prior
        df, guess = sigma_prior
        alpha, beta = df / 2.0, df * guess * guess / 2.0   # ChisqModel(df, sigma_guess)
        self.prior_df, self.prior_ss = 2 * alpha, 2 * beta
        self.sigma_max = float(sigma_max)
        self.max_flips, self.max_model_size = int(max_flips), int(max_model_size)
        self.allow_selection = bool(allow_selection)   # SpikeSlabSampler::allow_model_selection
        assert wsse in ("suf", "exact")
        self.wsse_form = wsse
        self.mt = rng_setup is not None and rng_setup[0] == "mt"
        self.sss_rng = BoRng()
        if self.mt:
            glob = o.rng_mt(int(rng_setup[1]))
            L.bo_rng_seed_mt(C.byref(self.sss_rng), L.bo_seed_rng(C.byref(glob)))
        else:
            L.bo_rng_seed_philox(C.byref(self.sss_rng), self.seed, self.chain, 3, 0)
        self.sweep = 0
        self.margin = np.inf
        self.weights = None
        self.suf = None

    def _slot(self, stream, index, stride):
        if self.mt:
            return self.sss_rng     # the sampler's one stream, in draw() order
        r = BoRng()
        self.L.bo_rng_seed_philox(C.byref(r), self.seed, self.chain, stream, 0)
        self.L.bo_rng_slot(C.byref(r), int(index), int(stride))
        return r

    def exact_wsse(self, w, gamma, beta):
        """fsum_i w_i r_i^2, r_i = fsum(y_i, -x_ij beta_j) over the included j"""
        inc = np.flatnonzero(gamma)
        r = [math.fsum([float(self.y[i])] + [-float(v) for v in self.X[i, inc] * beta[inc]])
             for i in range(self.n)]
        return math.fsum(float(wi) * ri * ri for wi, ri in zip(w, r))

    def impute(self):
        o, n, s = self.o, self.n, self.sweep
        inc = np.flatnonzero(self.gamma)
        r = self.y - self.X[:, inc] @ self.beta[inc]
        sd = np.sqrt(self.sigsq)
        w = np.empty(n)
        for i in range(n):
            delta = r[i] / sd
            rng = self._slot(IMPUTE_STREAM, s * n + i, IMPUTE_STRIDE)
            w[i] = o.gammas(rng, 0.5 * (self.nu + 1), 0.5 * (self.nu + delta * delta), 1)[0]
        return w

    def draw(self):
        L, o = self.L, self.o
        n, p = self.n, self.p
        w = self.impute()
        self.weights = w
        Xw = self.X * w[:, None]
        xtx = self.X.T @ Xw
        xty = Xw.T @ self.y
        yty = float(np.dot(self.y * w, self.y))
        self.suf = dict(sumw=float(np.sum(w)), yty=yty, xty=xty.copy())
        # SpikeSlabSampler given sigma^2
        h = L.bo_sss_create(p, _dp(fcol(xtx)), _dp(f64(xty)), 1, _dp(self.mu), _dp(fcol(self.prec)),
                            _dp(self.pi))
        try:
            L.bo_sss_set_options(h, self.max_model_size, self.max_flips)
            L.bo_sss_set_state(h, _u8(self.gamma), _dp(f64(self.beta)))
            C.memmove(L.bo_sss_rng(h), C.byref(self.sss_rng), C.sizeof(BoRng))
            st = L.bo_sss_draw_model_indicators(h, float(self.sigsq)) if self.allow_selection else 0
            if st == 0:
                st = L.bo_sss_draw_beta(h, float(self.sigsq))
            if st:
                raise RuntimeError("SpikeSlabSampler status %d" % st)
            g = np.zeros(p, dtype=np.uint8)
            b = np.zeros(p)
            L.bo_sss_get_state(h, _u8(g), _dp(b))
            C.memmove(C.byref(self.sss_rng), L.bo_sss_rng(h), C.sizeof(BoRng))
        finally:
            L.bo_sss_destroy(h)
        self.gamma, self.beta = g, b
        # sigma^2 | beta, w
        wsse = float(b @ xtx @ b - 2 * (b @ xty) + yty)
        self.suf["wsse_suf"] = wsse
        if self.wsse_form == "exact":
            wsse = self.suf["wsse_exact"] = self.exact_wsse(w, g, b)
        DF, SS = n + self.prior_df, wsse + self.prior_ss
        rng = self._slot(SN_STREAM, self.sweep, SN_STRIDE)
        if np.isinf(self.sigma_max):
            self.sigsq = 1.0 / o.gammas(rng, DF / 2, SS / 2, 1)[0]
        else:
            self.sigsq = 1.0 / o.trun_gammas(rng, DF / 2, SS / 2, 1.0 / self.sigma_max ** 2, 1)[0]
        # nu | beta, sigma^2 (observed data)
        inc = np.flatnonzero(g)
        r = self.y - self.X[:, inc] @ b[inc]
        sigma = np.sqrt(self.sigsq)
        u = (r / sigma) ** 2
        n_log_sigma = n * np.log(sigma)
        logf = lambda nu: nu_log_post(nu, u, n_log_sigma, self.nu_prior)  # noqa: E731
        unif = lambda: L.bo_unif(C.byref(rng))                              # noqa: E731
        rexp1 = lambda: 1.0 * L.bo_exp_rand(C.byref(rng))                   # noqa: E731
        self.nu, self.dx, m = slice_draw_nu(unif, rexp1, logf, self.nu, self.dx)
        self.margin = min(self.margin, m)
        self.sweep += 1
        return self.gamma.copy(), self.beta.copy(), self.sigsq, self.nu
