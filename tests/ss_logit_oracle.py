"""A restatement of StateSpacePosteriorSampler::draw() for StateSpaceLogitModel (bsts family =
"logit") on the device's substreams, one chain, in Python over the oracle's primitives: the parity
yardstick of ba_ss_logit_sweep.  The round is tests/ss_family_oracle.py's (StateSpaceLogitPosterior
Sampler.cpp:82-123); this file is what the family adds to it.

Per-step data: an observed step carries successes y_t and trials n_t; a new model has v_t = 0 and
q_t = 4 / n_t (StateSpaceLogitModel.cpp:67-74); a missing step has H_t = pi^2 / 3, and its successes
and trials are never read.

The observation model's sampler is BinomialLogitSpikeSlabSampler::draw with its own shuffle (every
position swaps with one drawn from the whole range).

The imputation: BinomialLogitCltDataImputer::impute(n_t, y_t, eta_t) for the observed steps, stream 9,
slot s T + t of 256 in the sampler's s-th imputation; v_t = sum / info, q_t = info.

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

from oracle_lib import BoRng, _dp
from ss_family_oracle import SsFamilyOracle, draw_sss
from ss_poisson_oracle import _copy

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


class SsLogitOracle(SsFamilyOracle):
    """one chain of StateSpaceLogitPosteriorSampler on the device's substreams"""

    MISSING_VARIANCE = MISSING_VARIANCE
    SHUFFLE_KIND = 1

    def __init__(self, o, successes, trials, X, observed, blocks, mu, prec, pi, seed, chain, gamma0, beta0=None,
                 clt_threshold=5, max_flips=-1):
        declare(o.lib)
        self.successes, self.trials = np.asarray(successes, dtype=float), np.asarray(trials, dtype=float)
        self.clt = int(clt_threshold)
        self.record = Record()
        SsFamilyOracle.__init__(self, o, X, observed, blocks, mu, prec, pi, seed, chain, gamma0, beta0, max_flips)

    @property
    def margin(self):
        return self.record.margin

    @property
    def btpe(self):
        return self.record.btpe

    def initial_precisions(self):
        # (a missing step's trials are not read)
        return np.array([4.0 / self.trials[t] if self.obs[t] else 0.0 for t in range(self.T)])

    def impute(self, s):
        total, info = impute(self.o, self.seed, self.chain, self.successes, self.trials, self.offset() + self.xbeta(),
                             self.obs, s, self.clt, self.record)
        ob = self.obs
        self.v, self.q = np.zeros(self.T), np.zeros(self.T)
        self.v[ob], self.q[ob] = total[ob] / info[ob], info[ob]


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
        gamma, beta = draw_sss(o, rng, X.T @ (X * info[:, None]), X.T @ total, mu, prec, pi, gamma, beta, max_flips,
                               SsLogitOracle.SHUFFLE_KIND)
        G[s], B[s] = gamma, beta
    return G, B, rec
