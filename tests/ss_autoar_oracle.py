"""A restatement of ArSpikeSlabSampler::draw() (bsts AddAutoAr: an ArStateModel whose coefficients
have a spike-and-slab prior), one chain, in numpy over the oracle's scalar primitives on a Philox
stream: the parity yardstick of state model kind 9 (ba_ss_add_state_model).

  Models/TimeSeries/PosteriorSamplers/ArSpikeSlabSampler.cpp   draw, draw_phi, shrink_phi,
                                                               draw_phi_univariate, draw_sigma_full_conditional
  Models/Glm/PosteriorSamplers/SpikeSlabSampler.cpp            draw_model_indicators, draw_beta, log_model_prob
  Models/Glm/VariableSelectionPrior.cpp:271-300                logp, make_valid
  LinAlg/SWEEP.cpp                                             SweptVarianceMatrix(precision, true).RSW(i)

draw() reads ONE generator in sequence: the Fisher-Yates shuffle's random_int(0, i), i = L - 1 .. 1;
one uniform per flip; up to 100 proposals of n normals (n the model's size), then
draw_phi_univariate's truncated normals; the sigma draw.

Every comparison that steers the draw records its margin (`margin`: the smallest seen): |log u -
(logp_new - logp_old)| per flip, the distance of every stationarity test from its boundary, the
rejection loops' accept tests.  `dtype=np.longdouble` evaluates all of the linear algebra in
extended precision ON THE SAME RANDOM NUMBERS (the primitives stay double): the difference between
the two evaluations is the gate of the device tests.
"""
import ctypes as C

import numpy as np

from oracle_lib import BoRng

AUTO_AR = 9


def chol(A):
    """lower Cholesky factor in A's dtype (numpy.linalg has no long double); None: not positive definite"""
    n = A.shape[0]
    Lc = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - Lc[j, :j] @ Lc[j, :j]
        if not d > 0:
            return None
        Lc[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            Lc[i, j] = (A[i, j] - Lc[i, :j] @ Lc[j, :j]) / Lc[j, j]
    return Lc


def lsolve(Lc, b):
    x = np.zeros_like(b)
    for i in range(len(b)):
        x[i] = (b[i] - Lc[i, :i] @ x[:i]) / Lc[i, i]
    return x


def ltsolve(Lc, b):
    n = len(b)
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - Lc[i + 1:, i] @ x[i + 1:]) / Lc[i, i]
    return x


def stationarity_margin(phi):
    """distance of ArModel::check_stationary's decision from its boundary: the quick bound sum |phi|
    < 1, else min over the step-down recursion's partial autocorrelations of | |r| - 1 |"""
    a = np.array(phi, dtype=float)
    s = np.sum(np.abs(a))
    m = abs(s - 1.0)
    if s < 1:
        return m
    for k in range(len(a), 0, -1):
        r = a[k - 1]
        m = min(m, abs(abs(r) - 1.0))
        if not abs(r) < 1:
            return m
        a = np.array([(a[j] + r * a[k - 2 - j]) / (1 - r * r) for j in range(k - 1)])
    return m


class AutoArSampler:
    """ArSpikeSlabSampler for one chain.  State: gamma (uint8), phi (L, zeros where excluded), sigsq."""

    def __init__(self, o, lags, mu, siginv, pi, df, sigma_guess, sigma_upper_limit=np.inf, truncate=True,
                 max_flips=-1, select=True, dtype=np.float64):
        self.o, self.lib = o, o.lib
        lib = self.lib
        lib.bo_random_int.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
        lib.bo_rnorm.restype = C.c_double
        lib.bo_rtrun_norm_2.argtypes = [C.c_void_p] + [C.c_double] * 4 + [C.POINTER(C.c_int)]
        lib.bo_rtrun_norm_2.restype = C.c_double
        self.L = int(lags)
        self.ft = dtype
        self.mu = np.array(mu, dtype=float).reshape(self.L)
        self.siginv = np.array(siginv, dtype=float).reshape(self.L, self.L)
        self.pi = np.array(pi, dtype=float).reshape(self.L)
        with np.errstate(divide="ignore"):
            self.logpi = np.log(self.pi)
            self.logcpi = np.log(1 - self.pi)
        # ChisqModel(df, sigma_guess): 2 alpha = df, 2 beta = df sigma_guess^2
        self.prior_df = 2 * (df / 2.0)
        self.prior_ss = 2 * (df * sigma_guess * sigma_guess / 2.0)
        self.sigma_max = float(sigma_upper_limit)
        self.truncate, self.max_flips, self.select = bool(truncate), int(max_flips), bool(select)
        self.margin = np.inf
        self.proposals = 0        # draw_beta calls of the last draw
        self.univariate = False   # the last draw went through draw_phi_univariate
        self.caught = False       # ... and an error inside it restored phi

    # -- decisions ---------------------------------------------------------------------------
    def _note(self, m):
        if np.isfinite(m):
            self.margin = min(self.margin, float(m))

    def stationary(self, phi):
        phi = np.ascontiguousarray(np.asarray(phi, dtype=float))
        self._note(stationarity_margin(phi))
        return bool(self.lib.bo_test_ar_check_stationary(len(phi), phi.ctypes.data_as(C.POINTER(C.c_double))))

    # -- SpikeSlabSampler ----------------------------------------------------------------------
    def spike_logp(self, g):
        ans = 0.0
        for i in range(self.L):
            ans += self.logpi[i] if g[i] else self.logcpi[i]
            if not np.isfinite(ans):
                return -np.inf
        return ans

    def _selected(self, g, xtx, xty, sigsq):
        idx = np.flatnonzero(g)
        ft = self.ft
        prec = self.siginv[np.ix_(idx, idx)].astype(ft)
        mu = self.mu[idx].astype(ft)
        X = np.asarray(xtx, dtype=float)[np.ix_(idx, idx)].astype(ft)
        xy = np.asarray(xty, dtype=float)[idx].astype(ft)
        return idx, prec, mu, X, xy, ft(sigsq)

    def log_model_prob(self, g, xtx, xty, sigsq):
        numerator = self.spike_logp(g)
        if numerator == -np.inf or not np.any(g):
            return numerator
        idx, prec, mu, X, xy, s2 = self._selected(g, xtx, xty, sigsq)
        Lp = chol(prec)
        if Lp is None:
            return -np.inf
        numerator = numerator + .5 * (2 * np.sum(np.log(np.diag(Lp))))
        pmu = prec @ mu
        numerator = numerator - .5 * (mu @ pmu)
        Lc = chol(prec + X / s2)
        if Lc is None:
            return -np.inf
        denominator = np.sum(np.log(np.diag(Lc)))
        S = lsolve(Lc, xy / s2 + pmu)
        denominator = denominator - .5 * (S @ S)
        return numerator - denominator

    def draw_model_indicators(self, rng, g, xtx, xty, sigsq):
        """returns the new indicators"""
        if not self.select:
            return g
        L = self.L
        g = np.array(g, dtype=np.uint8)
        indx = list(range(L))
        for i in range(L - 1, 0, -1):
            j = self.lib.bo_random_int(C.byref(rng), 0, i)
            if j != i:
                indx[i], indx[j] = indx[j], indx[i]
        logp = self.log_model_prob(g, xtx, xty, sigsq)
        if not np.isfinite(logp):
            for i in range(L):
                if self.pi[i] <= 0.0 and g[i]:
                    g[i] = 0
                if self.pi[i] >= 1.0 and not g[i]:
                    g[i] = 1
            logp = self.log_model_prob(g, xtx, xty, sigsq)
        if not np.isfinite(logp):
            raise RuntimeError("SpikeSlabSampler did not start with a legal configuration.")
        n = L
        if self.max_flips > 0:
            n = min(n, self.max_flips)
        for i in range(n):
            which = indx[i]
            g[which] ^= 1
            logp_new = self.log_model_prob(g, xtx, xty, sigsq)
            u = self.lib.bo_unif(C.byref(rng))
            with np.errstate(divide="ignore"):
                logu = np.log(u)
            d = float(logp_new - logp)
            self._note(abs(logu - d))
            if logu > d:
                g[which] ^= 1
            else:
                logp = logp_new
        return g

    def posterior(self, g, xtx, xty, sigsq):
        """(idx, precision, mean) of the included coefficients' conditional"""
        idx, prec, mu, X, xy, s2 = self._selected(g, xtx, xty, sigsq)
        pmu = prec @ mu
        prec = prec + X / s2
        pmu = pmu + xy / s2
        Lc = chol(prec)
        if Lc is None:
            raise RuntimeError("Cholesky decomposition failed in rmvn_ivar_mt.")
        return idx, prec, Lc, ltsolve(Lc, lsolve(Lc, pmu))

    def draw_beta(self, rng, g, xtx, xty, sigsq):
        """full-length coefficients"""
        out = np.zeros(self.L)
        if not np.any(g):
            return out
        idx, _, Lc, mean = self.posterior(g, xtx, xty, sigsq)
        z = np.array([self.lib.bo_rnorm(C.byref(rng), 0.0, 1.0) for _ in idx]).astype(self.ft)
        out[idx] = (ltsolve(Lc, z) + mean).astype(float)
        return out

    # -- ArSpikeSlabSampler --------------------------------------------------------------------
    def shrink_phi(self, phi):
        """on the INCLUDED sub-vector, as written; returns (ok, phi)"""
        attempts, max_attempts = 0, 20
        phi = np.array(phi, dtype=float)
        while True:
            a = attempts
            attempts += 1
            if not (a < max_attempts and not self.stationary(phi)):
                break
            phi = phi * .95
        return attempts < max_attempts, phi

    def univariate_conditional(self, prec, mean, phi, i):
        """(mean, sd) of coefficient i given the others under N(mean, prec^-1), through the swept
        precision: S = -prec, RSW(i)"""
        x = -prec[i, i]
        resid_var = -1.0 / x
        x = x * -1
        others = [j for j in range(len(phi)) if j != i]
        beta = np.array([(-prec[i, j]) / x for j in others], dtype=self.ft)
        cm = beta @ (np.asarray(phi, dtype=self.ft)[others] - mean[others]) + mean[i]
        return float(cm), float(np.sqrt(resid_var))

    def draw_phi_univariate(self, rng, g, phi_full, xtx, xty, sigsq):
        idx, prec, _, mean = self.posterior(g, xtx, xty, sigsq)
        p = len(idx)
        phi = np.array(phi_full, dtype=float)[idx]
        if not self.stationary(phi_full):
            ok, phi = self.shrink_phi(phi)
            if not ok:
                raise RuntimeError("illegal initial value of phi")
        for i in range(p):
            if p == 1:
                continue
            cm, csd = self.univariate_conditional(prec, mean, phi, i)
            initial_phi = phi[i]
            lo, hi = -1.0, 1.0
            attempts = 0
            while True:
                if attempts > 1000:
                    raise RuntimeError("Too many attempts in draw_phi_univariate.")
                attempts += 1
                st = C.c_int(0)
                cand = self.lib.bo_rtrun_norm_2(C.byref(rng), cm, csd, lo, hi, C.byref(st))
                if st.value:
                    raise RuntimeError("rtrun_norm_2")
                phi[i] = cand
                full = np.zeros(self.L)
                full[idx] = phi
                if self.stationary(full):
                    break
                if cand > initial_phi:
                    hi = cand
                else:
                    lo = cand
        full = np.zeros(self.L)
        full[idx] = phi
        return full

    def draw_phi(self, rng, g, phi, xtx, xty, sigsq):
        original = np.array(phi, dtype=float)
        self.proposals, self.univariate, self.caught = 0, False, False
        if not np.any(g):
            self.proposals = 1     # (drop_all: nothing is drawn, and an empty model is stationary)
            return np.zeros(self.L)
        ok, attempts = False, 0
        cur = original
        while not ok and attempts < 100:
            attempts += 1
            cur = self.draw_beta(rng, g, xtx, xty, sigsq)
            ok = self.stationary(cur) if self.truncate else True
        self.proposals = attempts
        if ok:
            return cur
        self.univariate = True
        try:
            return self.draw_phi_univariate(rng, g, original, xtx, xty, sigsq)
        except RuntimeError:
            self.caught = True
            return original

    def draw_sigma(self, rng, g, phi, xtx, yty_xty, n):
        xty, yty = yty_xty
        ft = self.ft
        if not np.any(g):
            ss = ft(yty)
        else:
            idx = np.flatnonzero(g)
            b = np.asarray(phi, dtype=float)[idx].astype(ft)
            X = np.asarray(xtx, dtype=float)[np.ix_(idx, idx)].astype(ft)
            ss = ft(yty) + (b @ (X @ b) - 2 * (b @ np.asarray(xty, dtype=float)[idx].astype(ft)))
        DF, SS = float(n + self.prior_df), float(ss + self.prior_ss)
        if np.isinf(self.sigma_max):
            return 1.0 / self.o.gammas(rng, DF / 2, SS / 2, 1)[0]
        return 1.0 / self.o.trun_gammas(rng, DF / 2, SS / 2, 1.0 / (self.sigma_max * self.sigma_max), 1)[0]

    def draw(self, rng, g, phi, sigsq, suf):
        """one ArSpikeSlabSampler::draw() on suf = dict(xtx, xty, yty, n): (gamma, phi, sigsq)"""
        xtx, xty = np.asarray(suf["xtx"], dtype=float), np.asarray(suf["xty"], dtype=float)
        g = self.draw_model_indicators(rng, np.array(g, dtype=np.uint8), xtx, xty, sigsq)
        phi = np.where(g != 0, np.asarray(phi, dtype=float), 0.0)   # set_inc
        phi = self.draw_phi(rng, g, phi, xtx, xty, sigsq)
        sigsq = self.draw_sigma(rng, g, phi, xtx, (xty, suf["yty"]), suf["n"])
        return g, phi, float(sigsq)


def ar_stream_id(blocks, which):
    """the engine's sampler id of autoregression-family block `which` of a list (kinds 4 and 9)"""
    occ = sum(1 for b in blocks[:which] if b["kind"] in (4, AUTO_AR))
    return 12 + 16 * occ


def fresh_rng(o, seed, chain, stream, pos=0):
    r = BoRng()
    o.lib.bo_rng_seed_philox(C.byref(r), int(seed), int(chain), int(stream), int(pos))
    return r
