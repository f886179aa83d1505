"""A restatement of StateSpacePosteriorSampler::draw() for StateSpaceLogitModel (bsts family =
"logit") on the device's substreams, one chain, in Python over the oracle's primitives: the parity
yardstick of ba_ss_logit_sweep, built as tests/ss_poisson_oracle.py is (whose structure, filter,
state-model statistics, SpikeSlabSampler driver and dense posterior it imports).

Per-step data: an observed step carries successes y_t, trials n_t, a latent value v_t and a
precision q_t (0 and 4 / n_t in a new model, StateSpaceLogitModel.cpp:67-74); the filter sees
v_t - x_t'beta with the observation variance H_t = 1 / q_t; a missing step has no observation and
H_t = pi^2 / 3, and its successes and trials are never read.

One draw() (StateSpacePosteriorSampler.cpp:42-64, StateSpaceLogitPosteriorSampler.cpp:82-123):
  0. the first time: impute_state with the latent data in hand, then one imputation whose values
     are all overwritten in step 3 before anything reads them -- only its slots are used up, so
     round r of a fresh sampler imputes with s = r + 1;
  1. the observation model's sampler with fix_latent_data(true) (BinomialLogitSpikeSlabSampler::
     draw: its own shuffle -- every position swaps with one drawn from the whole range --, then
     indicators and beta at sigma^2 = 1 with a fixed-precision slab) on the complete-data
     statistics the last impute_state left (X'QX, X'Q(v - Z alpha), observed steps), stream 3;
  2. every state model's variance draw (ss_student_oracle's);
  3. impute_nonstate_latent_data: BinomialLogitCltDataImputer::impute(n_t, y_t, eta_t) with
     eta_t = Z_t'alpha_t + x_t'beta (alpha the last state draw, beta the new one) for the observed
     steps, stream 9, slot s T + t of 256 in the sampler's s-th imputation; v_t = sum / info,
     q_t = info;
  4. impute_state: the simulation smoother with H_t, then the statistics over the observed steps.

The imputer (BinomialLogitDataImputer.cpp:119-211):
  n_t <= clt_threshold  per trial a logistic draw on the side of 0 its outcome says (bo_runif on
                        (cutpoint, 1) or (0, cutpoint), the logit) and the component of the
                        nine-normal scale mixture (bo_rmulti on the posterior weights);
  n_t >  clt_threshold  the failures' and the successes' counts per component by two multinomial
                        draws (Rmath::rmultinom_mt restated over bo_test_rbinom), then one normal
                        draw (bo_rnorm) with the truncated-normal moments of the occupied cells
                        (trun_norm_moments, distributions/trun_norm.cpp:243-269, restated here:
                        the oracle's own is static).
A replay of the same uniforms on a copy of the stream restates the component draw's cumulative
comparison and, for a binomial draw with n min(p, 1 - p) < 30, the inversion loop's `u < f`, and
records the smallest margin of any of them -- a draw closer to a branch point than the device's
arithmetic differs from this one's may take the other branch there.  A binomial draw at
n min(p, 1 - p) >= 30 (BTPE) is counted in `btpe`: its comparisons are not under the record.
"""
import ctypes as C
import math

import numpy as np

from oracle_lib import BoRng, _dp, _u8, f64, fcol
from ss_poisson_oracle import (Structure, bonferroni_bound, dense_posterior, impute_state,  # noqa: F401
                               moment_z, state_model_suf, _copy)
from ss_student_oracle import SsStudentOracle

LOGIT_STREAM, LOGIT_STRIDE = 9, 256
MISSING_VARIANCE = 3.289868133696452872944830333292   # Constants::pi_squared_over_3
LOG_SQRT_2PI = 0.918938533204672741780329736406
MIX_SIGMA = np.array([0.88437229872213, 1.16097607474416, 1.28021991084306, 1.3592552924727, 1.67589879794907,
                      2.20287232043947, 2.20507148325819, 2.91944313615144, 3.90807611741308])
MIX_WEIGHT = np.array([0.038483985581272, 0.13389889791451, 0.0657842076622429, 0.105680086433879,
                       0.345939491553619, 0.0442261124345564, 0.193289780660134, 0.068173066865908,
                       0.00452437089387876])
MIX_LOGW = np.array([math.log(w) for w in MIX_WEIGHT])
MIX_LOGSIGMA = np.array([math.log(s) for s in MIX_SIGMA])


def declare(L):
    L.bo_rng_slot.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.bo_rng_slot.restype = None
    L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_rnorm.restype = C.c_double
    L.bo_unif.argtypes = [C.c_void_p]
    L.bo_unif.restype = C.c_double
    L.bo_runif.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_runif.restype = C.c_double
    L.bo_rmulti.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    L.bo_rmulti.restype = C.c_int
    L.bo_test_rbinom.argtypes = [C.c_void_p, C.c_uint, C.c_double]
    L.bo_test_rbinom.restype = C.c_uint
    L.bo_sss_set_shuffle_kind.argtypes = [C.c_void_p, C.c_int]
    L.bo_sss_set_shuffle_kind.restype = None


class Record:
    """the smallest margin of the replayed branch comparisons; how many binomial draws took BTPE"""

    def __init__(self):
        self.margin, self.btpe = np.inf, 0

    def see(self, gap):
        self.margin = min(self.margin, gap)


def _log_pnorm(x, lower):
    z = -x if lower else x
    return math.log(0.5 * math.erfc(z / 1.4142135623730951))


def trun_norm_moments(mu, sigma, cutpoint, positive_support):
    """distributions/trun_norm.cpp:243-269: (mean, variance) of N(mu, sigma^2) above / below the cutpoint"""
    sigsq = sigma * sigma
    a = (cutpoint - mu) / sigma
    log_dnorm = -LOG_SQRT_2PI - 0.5 * a * a
    if positive_support:
        phi_ratio = math.exp(log_dnorm - _log_pnorm(a, False))
        mean = mu + sigma * phi_ratio
        variance = sigsq * (1 - phi_ratio * (phi_ratio - a))
    else:
        phi_ratio = math.exp(log_dnorm - _log_pnorm(a, True))
        mean = mu - sigma * phi_ratio
        variance = sigsq * (1 - a * phi_ratio - phi_ratio * phi_ratio)
    return mean, max(variance, 0.0)


def rbinom(L, rng, n, pp, rec):
    """BOOM::binomial_distribution(n, pp)(rng) by bo_test_rbinom; below n min(p, q) = 30 the
    inversion loop (distributions/BinomialDistribution.cpp) replayed on a copy of the stream"""
    p = pp if pp < 1.0 - pp else 1.0 - pp
    q = 1.0 - p
    replay = _copy(rng)
    ans = int(L.bo_test_rbinom(C.byref(rng), int(n), float(pp)))
    if n * p >= 30:
        rec.btpe += 1
        return ans
    r = p / q
    g = r * (n + 1)
    qn = q ** float(n)
    done = False
    while not done:
        ix, f, u = 0, qn, L.bo_unif(C.byref(replay))
        while True:
            rec.see(abs(u - f))
            if u < f:
                done = True
                break
            if ix > 110:
                break
            u -= f
            ix += 1
            f *= (g / ix - r)
    if pp > 0.5:
        ix = int(n) - ix
    assert ix == ans, (n, pp, ix, ans)
    return ans


def rmultinom(L, rng, n, prob, rec):
    """Rmath::rmultinom_mt (Bmath/rmultinom.cpp:82-136) for probabilities that sum to one"""
    K = len(prob)
    rN = [0] * K
    p_tot = 0.0
    for k in range(K):
        p_tot += prob[k]
    if n == 0:
        return rN
    for k in range(K - 1):
        rN[k] = rbinom(L, rng, n, prob[k] / p_tot, rec)
        n -= rN[k]
        if n <= 0:
            return rN
        p_tot -= prob[k]
    rN[K - 1] = n
    return rN


def impute_small_sample(L, rng, nt, ys, eta, rec):
    """impute_small_sample (BinomialLogitDataImputer.cpp:134-152): (sum, info)"""
    total, info = 0.0, 0.0
    cutpoint_prob = 1 / (1 + math.exp(-(0 - eta)))
    for t in range(nt):
        if t < ys:
            u = L.bo_runif(C.byref(rng), cutpoint_prob, 1.0)
        else:
            u = L.bo_runif(C.byref(rng), 0.0, cutpoint_prob)
        latent = (0.0 + 1.0 * math.log(u / (1. - u))) + eta
        v = latent - eta
        wsp = np.zeros(9)
        for c in range(9):
            xs = (v - 0.0) / MIX_SIGMA[c]
            wsp[c] = MIX_LOGW[c] + -(LOG_SQRT_2PI + 0.5 * xs * xs + MIX_LOGSIGMA[c])
        mx = wsp.max()
        nc = 0.0
        for c in range(9):
            wsp[c] = math.exp(wsp[c] - mx)
            nc += wsp[c]
        wsp = np.ascontiguousarray(wsp / nc)
        replay = _copy(rng)
        st = C.c_int(0)
        ind = L.bo_rmulti(C.byref(rng), _dp(wsp), 9, C.byref(st))
        if st.value:
            raise RuntimeError("rmulti status %d" % st.value)
        # rmulti_mt (distributions/rmulti.cpp:41-78) on the same uniform
        probsum = 0.0
        for c in range(9):
            probsum += wsp[c]
        tmp = L.bo_runif(C.byref(replay), 0.0, probsum)
        psum, got = 0.0, -1
        for c in range(9):
            psum += wsp[c]
            rec.see(abs(tmp - psum))
            if got < 0 and tmp <= psum:
                got = c
        assert got == ind
        w = 1.0 / (MIX_SIGMA[ind] * MIX_SIGMA[ind])
        info += w
        total += latent * w
    return total, info


def impute_large_sample(L, rng, nt, ys, eta, rec):
    """impute_large_sample (BinomialLogitDataImputer.cpp:155-211): (sum, info)"""
    xz = (0 - eta) / 1.0
    neg_support, pos_support = 1 / (1 + math.exp(-xz)), 1 / (1 + math.exp(xz))
    p0, p1 = np.zeros(9), np.zeros(9)
    for m in range(9):
        z = (0 - eta) / MIX_SIGMA[m]
        p0[m] = MIX_WEIGHT[m] / neg_support * (0.5 * math.erfc(-z / 1.4142135623730951))
        p1[m] = MIX_WEIGHT[m] / pos_support * (0.5 * math.erfc(z / 1.4142135623730951))
    s0 = s1 = 0.0
    for m in range(9):
        s0 += p0[m]
        s1 += p1[m]
    p0, p1 = [float(x) / s0 for x in p0], [float(x) / s1 for x in p1]
    N0 = rmultinom(L, rng, nt - ys, p0, rec)
    N1 = rmultinom(L, rng, ys, p1, rec)
    info = mean = variance = 0.0
    for m in range(9):
        total_obs = N0[m] + N1[m]
        if total_obs == 0:
            continue
        sigsq = MIX_SIGMA[m] * MIX_SIGMA[m]
        sig4 = sigsq * sigsq
        info += total_obs / sigsq
        if N0[m] > 0:
            tmean, tvar = trun_norm_moments(eta, MIX_SIGMA[m], 0.0, False)
            mean += N0[m] * tmean / sigsq
            variance += N0[m] * tvar / sig4
        if N1[m] > 0:
            tmean, tvar = trun_norm_moments(eta, MIX_SIGMA[m], 0.0, True)
            mean += N1[m] * tmean / sigsq
            variance += N1[m] * tvar / sig4
    return L.bo_rnorm(C.byref(rng), mean, math.sqrt(variance)), info


def impute_point(L, rng, nt, ys, eta, clt, rec):
    """BinomialLogitCltDataImputer::impute(n, y, eta): (sum, info)"""
    nt, ys = int(round(nt)), int(round(ys))
    if nt > clt:
        return impute_large_sample(L, rng, nt, ys, float(eta), rec)
    return impute_small_sample(L, rng, nt, ys, float(eta), rec)


def impute(o, seed, chain, successes, trials, eta, observed, s, clt, rec):
    """the sampler's s-th imputation of every observed step: (sum, info); 0 where the step is
    missing (nothing of it is read)"""
    L = o.lib
    declare(L)
    T = len(eta)
    total, info = np.zeros(T), np.zeros(T)
    for t in range(T):
        if not observed[t]:
            continue
        rng = BoRng()
        L.bo_rng_seed_philox(C.byref(rng), int(seed), int(chain), LOGIT_STREAM, 0)
        L.bo_rng_slot(C.byref(rng), int(s) * T + t, LOGIT_STRIDE)
        total[t], info[t] = impute_point(L, rng, trials[t], successes[t], eta[t], clt, rec)
    return total, info


def observation_variances(q, observed):
    return np.array([1.0 / q[t] if observed[t] else MISSING_VARIANCE for t in range(len(q))])


def draw_sss(o, rng, xtx, xty, mu, prec, pi, gamma, beta, max_flips=-1):
    """BinomialLogitSpikeSlabSampler::draw_model_indicators / draw_beta with a fixed-precision slab:
    ss_poisson_oracle.draw_sss with the sampler's own shuffle (bo_sss, scales = 0, shuffle kind 1)
    continuing the stream `rng` (updated in place): (gamma, beta)"""
    L, p = o.lib, len(xty)
    o._declare_sss()
    declare(L)
    h = L.bo_sss_create(p, _dp(fcol(xtx)), _dp(f64(xty)), 0, _dp(f64(mu)), _dp(fcol(prec)), _dp(f64(pi)))
    try:
        L.bo_sss_set_shuffle_kind(h, 1)
        L.bo_sss_set_options(h, -1, int(max_flips))
        L.bo_sss_set_state(h, _u8(np.ascontiguousarray(gamma, dtype=np.uint8)), _dp(f64(beta)))
        C.memmove(L.bo_sss_rng(h), C.byref(rng), C.sizeof(BoRng))
        st = L.bo_sss_draw_model_indicators(h, 1.0)
        if st == 0:
            st = L.bo_sss_draw_beta(h, 1.0)
        if st:
            raise RuntimeError("SpikeSlabSampler status %d" % st)
        g, b = np.zeros(p, dtype=np.uint8), np.zeros(p)
        L.bo_sss_get_state(h, _u8(g), _dp(b))
        C.memmove(C.byref(rng), L.bo_sss_rng(h), C.sizeof(BoRng))
    finally:
        L.bo_sss_destroy(h)
    return g, b


class SsLogitOracle:
    """one chain of StateSpaceLogitPosteriorSampler on the device's substreams"""

    def __init__(self, o, successes, trials, X, observed, blocks, mu, prec, pi, seed, chain, gamma0, beta0=None,
                 clt_threshold=5, max_flips=-1):
        self.o, self.L = o, o.lib
        declare(self.L)
        self.X = np.asarray(X, dtype=np.float64)
        self.T, self.p = self.X.shape
        self.obs = (np.ones(self.T, bool) if observed is None else np.asarray(observed).astype(bool))
        self.successes, self.trials = np.asarray(successes, dtype=float), np.asarray(trials, dtype=float)
        self.clt = int(clt_threshold)
        self.S = Structure(blocks)
        self.mu, self.prec, self.pi = f64(mu), np.asarray(prec, dtype=np.float64), f64(pi)
        self.seed, self.chain, self.max_flips = int(seed), int(chain), int(max_flips)
        self.gamma = np.ascontiguousarray(gamma0, dtype=np.uint8).copy()
        self.beta = np.zeros(self.p) if beta0 is None else f64(beta0) * self.gamma
        # the state models' parameters, priors and samplers' streams: the Student restatement's
        # (built on a series that only sizes the handle; its observation model is not used)
        helper = SsStudentOracle(o, np.zeros(self.T), self.X, None if observed is None else observed, blocks,
                                 self.mu, self.prec, self.pi, seed, chain, self.gamma)
        self._sm = helper
        self.var = helper.var
        self.suf_n, self.suf_ss = helper.suf_n, helper.suf_ss
        self.sss_rng = o.rng_philox(self.seed, self.chain, 3, 0)
        self.state_rng = o.rng_philox(self.seed, self.chain, 2, 0)
        # a new model: v = 0, q = 4 / n_t (a missing step's trials are not read)
        self.v = np.zeros(self.T)
        self.q = np.array([4.0 / self.trials[t] if self.obs[t] else 0.0 for t in range(self.T)])
        self.state = None
        self.initialized = False
        self.imputations = 0
        self.rounds = 0
        self.record = Record()

    @property
    def margin(self):
        return self.record.margin

    @property
    def btpe(self):
        return self.record.btpe

    def _rnorm(self, mu, sd):
        return self.L.bo_rnorm(C.byref(self.state_rng), float(mu), float(sd))

    def xbeta(self):
        inc = np.flatnonzero(self.gamma)
        return self.X[:, inc] @ self.beta[inc]

    def offset(self):
        return self.state @ self.S.Z

    def H(self):
        return observation_variances(self.q, self.obs)

    def set_latent(self, v, q):
        self.v = np.where(self.obs, np.asarray(v, dtype=float), 0.0)
        self.q = np.where(self.obs, np.asarray(q, dtype=float), 0.0)

    def impute_latent(self, keep=True):
        """impute_nonstate_latent_data; keep = False: the slots are used up and nothing is stored"""
        s = self.imputations
        self.imputations += 1
        if not keep:
            return s
        total, info = impute(self.o, self.seed, self.chain, self.successes, self.trials, self.offset() + self.xbeta(),
                             self.obs, s, self.clt, self.record)
        ob = self.obs
        self.v, self.q = np.zeros(self.T), np.zeros(self.T)
        self.v[ob], self.q[ob] = total[ob] / info[ob], info[ob]
        return s

    def impute_state(self):
        ystar = self.v - self.xbeta()
        self.state = impute_state(self.S, self.var, ystar, self.obs, self.H(), self._rnorm)
        self.suf_n, self.suf_ss = state_model_suf(self.S, self.state)
        # update_complete_data_sufficient_statistics: observed steps, response v - Z alpha, weight q
        ob = self.obs
        z = ((self.v - self.offset()) * self.q)[ob]
        Xo, qo = self.X[ob], self.q[ob]
        self.xtx, self.xty = Xo.T @ (Xo * qo[:, None]), Xo.T @ z
        return self.state

    def draw_observation_model(self):
        self.gamma, self.beta = draw_sss(self.o, self.sss_rng, self.xtx, self.xty, self.mu, self.prec, self.pi,
                                         self.gamma, self.beta, self.max_flips)

    def draw_state_models(self):
        sm = self._sm
        sm.var, sm.suf_n, sm.suf_ss = self.var, self.suf_n, self.suf_ss
        sm.draw_state_models()
        self.var = sm.var

    def draw(self):
        if not self.initialized:
            self.impute_state()
            self.initialized = True
            self.impute_latent(keep=False)   # (every value is overwritten below before it is read)
        self.draw_observation_model()
        self.draw_state_models()
        self.last_s = self.impute_latent()
        self.impute_state()
        self.rounds += 1
        return self.gamma.copy(), self.beta.copy()


def logit_regression_rounds(o, X, y, ntrials, mu, prec, pi, seed, chain, gamma0, nsweeps, clt_threshold=5,
                            max_flips=-1):
    """BinomialLogitSpikeSlabSampler through the imputer above with offset 0 and every step
    observed, then bo_sss on X'QX and X'(sum): what Oracle.logit_run computes (the two differ in
    the order of the sums only).  Returns per sweep gamma and beta, and the record of margins"""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    gamma, beta = np.ascontiguousarray(gamma0, dtype=np.uint8).copy(), np.zeros(p)
    rng = o.rng_philox(int(seed), int(chain), 3, 0)
    obs = np.ones(n, bool)
    rec = Record()
    G, B = np.zeros((nsweeps, p), np.uint8), np.zeros((nsweeps, p))
    for s in range(nsweeps):
        inc = np.flatnonzero(gamma)
        total, info = impute(o, seed, chain, y, ntrials, X[:, inc] @ beta[inc], obs, s, clt_threshold, rec)
        gamma, beta = draw_sss(o, rng, X.T @ (X * info[:, None]), X.T @ total, mu, prec, pi, gamma, beta, max_flips)
        G[s], B[s] = gamma, beta
    return G, B, rec
