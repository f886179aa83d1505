"""A restatement of StateSpacePosteriorSampler::draw() for StateSpacePoissonModel (bsts family =
"poisson") on the device's substreams, one chain, in Python over the oracle's primitives: the
parity yardstick of ba_ss_poisson_sweep.  The round is tests/ss_family_oracle.py's (StateSpacePoisson
PosteriorSampler.cpp:79-147); this file is what the family adds to it.

Per-step data: a new model has v_t = 0 and q_t = 1; a missing step has H_t = pi^2 / 6, and its count
and exposure are never read.

The observation model's sampler is PoissonRegressionSpikeSlabSampler (.cpp:55-59) with the plain shuffle.

The imputation: PoissonDataImputer::impute(y_t, exposure_t, eta_t) for the observed steps, stream 11,
slot s T + t of 256 in the sampler's s-th imputation: the last event time by Cheng's BC beta sampler,
the event past the interval (three branches at |eta| >= 600), the two unmixing draws; q_t = q_ext
(+ q_int if y_t > 0), v_t = (q_ext (z_ext - mu_ext) (+ q_int (z_int - mu_int))) / q_t, the external
term first.

The imputer's values come from the oracle's primitives (bo_test_rbeta_a1, bo_exp_rand,
bo_rmulti); a replay of the same uniforms on a copy of the stream (bo_unif, bo_runif) restates
the beta sampler's accept / reject tests and the component draw's cumulative comparison and
records the smallest margin of any of them -- a draw closer to a branch point than the device's
arithmetic differs from this one's may take the other branch there.
"""
import ctypes as C
import math

import numpy as np

from oracle_lib import BoRng, _dp, f64
from ss_family_oracle import SsFamilyOracle, draw_sss

POISSON_STREAM, POISSON_STRIDE = 11, 256
MISSING_VARIANCE = 1.6449340668482264061   # Constants::pi_squared_over_6
LOG_SQRT_2PI = 0.918938533204672741780329736406


def declare(L):
    L.bo_rng_slot.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.bo_rng_slot.restype = None
    L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_rnorm.restype = C.c_double
    L.bo_unif.argtypes = [C.c_void_p]
    L.bo_unif.restype = C.c_double
    L.bo_exp_rand.argtypes = [C.c_void_p]
    L.bo_exp_rand.restype = C.c_double
    L.bo_runif.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_runif.restype = C.c_double
    L.bo_rmulti.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    L.bo_rmulti.restype = C.c_int
    L.bo_test_rbeta_a1.argtypes = [C.c_void_p, C.c_double]
    L.bo_test_rbeta_a1.restype = C.c_double


def _copy(rng):
    r = BoRng()
    C.memmove(C.byref(r), C.byref(rng), C.sizeof(BoRng))
    return r


def _fused(v):
    """an a + b c the device may round once: tests/imputer_ref.py's replays move it by an ulp
    (this module's `math` is then their table); the value itself otherwise"""
    f = getattr(math, "fused", None)
    return v if f is None else f(v)


def _gap(a, b):
    return abs(a - b) / max(1.0, abs(a), abs(b))


def rbeta_a1_margin(L, rng, aa):
    """Rmath::rbeta_mt(rng, aa, 1), aa >= 1 (algorithm BC with a = 1, b = aa) replayed on `rng`:
    (the draw, the smallest gap of a comparison that decided a branch)"""
    expmax = 1024 * 0.693147180559945309417232121458
    a, b = (aa, 1.0) if aa < 1.0 else (1.0, aa)
    alpha, beta, delta = a + b, 1.0 / a, 1.0 + b - a
    k1 = delta * (0.0138889 + 0.0416667 * a) / (b * beta - 0.777778)
    k2 = 0.25 + (0.5 + 0.25 / delta) * a
    margin = np.inf

    def vw(u1):
        v = beta * math.log(u1 / (1.0 - u1))
        return v, (b * math.exp(v) if v <= expmax else np.finfo(float).max)
    while True:
        u1 = L.bo_unif(C.byref(rng))
        u2 = L.bo_unif(C.byref(rng))
        margin = min(margin, _gap(u1, 0.5))
        if u1 < 0.5:
            y = u1 * u2
            z = u1 * y
            margin = min(margin, _gap(0.25 * u2 + z - y, k1))
            if 0.25 * u2 + z - y >= k1:
                continue
        else:
            z = u1 * u1 * u2
            margin = min(margin, _gap(z, 0.25))
            if z <= 0.25:
                v, w = vw(u1)
                break
            margin = min(margin, _gap(z, k2))
            if z >= k2:
                continue
        v, w = vw(u1)
        lhs, rhs = alpha * (math.log(alpha / (a + w)) + v) - 1.3862944, math.log(z)
        margin = min(margin, _gap(lhs, rhs))
        if lhs >= rhs:
            break
    return (a / (a + w) if aa == a else w / (a + w)), margin


class Mixtures:
    """the reference table's mixtures as the engine takes them (dict(counts, ncomp, mu, sigma,
    weight, largest_index))"""

    def __init__(self, mix):
        self.counts = np.asarray(mix["counts"], dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(np.asarray(mix["ncomp"], dtype=np.int64))])
        self.mu, self.sigma = f64(mix["mu"]), f64(mix["sigma"])
        self.logw = np.array([math.log(w) for w in f64(mix["weight"])])
        self.largest = int(mix["largest_index"])

    def of(self, nevents):
        i = int(np.searchsorted(self.counts, nevents))
        assert i < len(self.counts) and self.counts[i] == nevents, "no mixture for count %d" % nevents
        s = slice(self.off[i], self.off[i + 1])
        return self.mu[s], self.sigma[s], self.logw[s]


def unmix(L, rng, M, u, nevents):
    """unmix_poisson_augmented_data (poisson_mixture_approximation_table.cpp:45-62): (mu, sigsq,
    margin of the component draw)"""
    if nevents >= M.largest:
        return -math.log(float(nevents)), 1.0 / float(nevents), np.inf
    mu, sigma, logw = M.of(nevents)
    nc = len(mu)
    wsp = np.zeros(nc)
    for c in range(nc):
        xs = (u - mu[c]) / sigma[c]
        wsp[c] = logw[c] + -(LOG_SQRT_2PI + 0.5 * xs * xs + math.log(sigma[c]))
    mx = wsp.max()
    tot = 0.0
    for c in range(nc):
        wsp[c] = math.exp(wsp[c] - mx)
        tot += wsp[c]
    wsp = np.ascontiguousarray(wsp / tot)
    replay = _copy(rng)
    st = C.c_int(0)
    ind = L.bo_rmulti(C.byref(rng), _dp(wsp), nc, C.byref(st))
    if st.value:
        raise RuntimeError("rmulti status %d" % st.value)
    # rmulti_mt (distributions/rmulti.cpp:41-78) on the same uniform: where tmp fell among the
    # cumulative sums
    probsum = 0.0
    for c in range(nc):
        probsum += wsp[c]
    tmp = L.bo_runif(C.byref(replay), 0.0, probsum)
    psum, margin, got = 0.0, np.inf, -1
    for c in range(nc):
        psum += wsp[c]
        margin = min(margin, abs(tmp - psum))
        if got < 0 and tmp <= psum:
            got = c
    assert got == ind
    return mu[ind], sigma[ind] * sigma[ind], margin


def impute_parts(L, rng, M, y, exposure, eta):
    """PoissonDataImputer::impute (PoissonDataImputer.cpp:36-96): the external point (z_ext, mu_e,
    sigsq_e), the internal one (z_int, mu_i, sigsq_i; None where y = 0) and the smallest margin"""
    y = int(round(y))
    margin = np.inf
    t_final = 0.0
    if y > 0:
        replay = _copy(rng)
        draw = L.bo_test_rbeta_a1(C.byref(rng), float(y))
        again, margin = rbeta_a1_margin(L, replay, float(y))
        assert abs(again - draw) <= 1e-14 * draw
        t_final = exposure * draw
    delta = exposure - t_final
    if abs(eta) < 600:
        z_ext = -math.log(_fused(delta + (1.0 / math.exp(eta)) * L.bo_exp_rand(C.byref(rng))))
    elif delta > 0:
        err = -math.log(L.bo_exp_rand(C.byref(rng)))          # rexv_mt(rng, 0, 1)
        xx, yy = math.log(delta), -err - eta
        hi, lo = max(xx, yy), min(xx, yy)
        z_ext = -(hi + math.log1p(math.exp(lo - hi)))             # -lse2
    else:
        z_ext = eta + -math.log(L.bo_exp_rand(C.byref(rng)))
    mu_e, sig_e, m = unmix(L, rng, M, z_ext - eta, 1)
    margin = min(margin, m)
    internal = None
    if y > 0:
        z_int = -math.log(t_final)
        mu_i, sig_i, m = unmix(L, rng, M, z_int - eta, y)
        margin = min(margin, m)
        internal = (z_int, mu_i, sig_i)
    return (z_ext, mu_e, sig_e), internal, margin


def impute_point(L, rng, M, y, exposure, eta):
    """PoissonDataImputer::impute and the combination of StateSpacePoissonPosteriorSampler.cpp:
    112-123, the external point first: (v, q, margin)"""
    (z_ext, mu_e, sig_e), internal, margin = impute_parts(L, rng, M, y, exposure, eta)
    q = 1.0 / sig_e
    s = (z_ext - mu_e) * q
    if internal is not None:
        z_int, mu_i, sig_i = internal
        s += _fused((z_int - mu_i) * (1.0 / sig_i))   # (sum + weight x residual: fusable on the device)
        q += 1.0 / sig_i
    return s / q, q, margin


def impute(o, seed, chain, M, counts, exposure, eta, observed, s):
    """the sampler's s-th imputation of every observed step: (v, q, margin); v = q = 0 where the
    step is missing (nothing of it is read)"""
    L = o.lib
    declare(L)
    T = len(eta)
    v, q, margin = np.zeros(T), np.zeros(T), np.inf
    for t in range(T):
        if not observed[t]:
            continue
        rng = BoRng()
        L.bo_rng_seed_philox(C.byref(rng), int(seed), int(chain), POISSON_STREAM, 0)
        L.bo_rng_slot(C.byref(rng), int(s) * T + t, POISSON_STRIDE)
        v[t], q[t], m = impute_point(L, rng, M, counts[t], exposure[t], float(eta[t]))
        margin = min(margin, m)
    return v, q, margin


class SsPoissonOracle(SsFamilyOracle):
    """one chain of StateSpacePoissonPosteriorSampler on the device's substreams"""

    MISSING_VARIANCE = MISSING_VARIANCE

    def __init__(self, o, counts, exposure, X, observed, blocks, mix, mu, prec, pi, seed, chain, gamma0,
                 beta0=None, max_flips=-1):
        declare(o.lib)
        self.counts, self.exposure = np.asarray(counts, dtype=float), np.asarray(exposure, dtype=float)
        self.M = Mixtures(mix)
        self.margin = np.inf   # the imputer's branch comparisons'
        SsFamilyOracle.__init__(self, o, X, observed, blocks, mu, prec, pi, seed, chain, gamma0, beta0, max_flips)

    def initial_precisions(self):
        return np.where(self.obs, 1.0, 0.0)

    def impute(self, s):
        self.v, self.q, m = impute(self.o, self.seed, self.chain, self.M, self.counts, self.exposure,
                                   self.offset() + self.xbeta(), self.obs, s)
        self.margin = min(self.margin, m)


def poisson_regression_rounds(o, X, y, exposure, mix, mu, prec, pi, seed, chain, gamma0, nsweeps, max_flips=-1):
    """PoissonRegressionSpikeSlabSampler through the imputer above with offset 0 and every step
    observed, then bo_sss on X'QX and X'Q v: what Oracle.poisson_run computes (the two differ in
    the order of the sums only).  Returns per sweep gamma and beta, and the smallest margin"""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    M = Mixtures(mix)
    gamma, beta = np.ascontiguousarray(gamma0, dtype=np.uint8).copy(), np.zeros(p)
    rng = o.rng_philox(int(seed), int(chain), 3, 0)
    obs = np.ones(n, bool)
    G, B, margin = np.zeros((nsweeps, p), np.uint8), np.zeros((nsweeps, p)), np.inf
    for s in range(nsweeps):
        inc = np.flatnonzero(gamma)
        v, q, m = impute(o, seed, chain, M, y, exposure, X[:, inc] @ beta[inc], obs, s)
        margin = min(margin, m)
        gamma, beta = draw_sss(o, rng, X.T @ (X * q[:, None]), X.T @ (v * q), mu, prec, pi, gamma, beta, max_flips)
        G[s], B[s] = gamma, beta
    return G, B, margin
