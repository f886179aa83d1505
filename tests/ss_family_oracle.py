"""One chain of StateSpacePosteriorSampler::draw() with a latent-data observation model (bsts family =
"poisson", "logit") on the device's substreams, in Python over the oracle's primitives: what the
restatements of tests/ss_poisson_oracle.py and tests/ss_logit_oracle.py share.  A family supplies its
imputer (impute_latent), the precisions of a new model (initial_precisions), the variance of a missing
step (MISSING_VARIANCE) and the shuffle of its SpikeSlabSampler (SHUFFLE_KIND).

Per-step data: an observed step carries a latent value v_t and a precision q_t; the filter sees
v_t - x_t'beta with the observation variance H_t = 1 / q_t; a missing step has no observation, the
family's MISSING_VARIANCE as H_t, and its data are never read.

One draw() (StateSpacePosteriorSampler.cpp:42-64):
  0. the first time: impute_state with the latent data in hand, then one imputation whose values are
     all overwritten in step 3 before anything reads them -- only its slots are used up, so round r
     of a fresh sampler imputes with s = r + 1;
  1. the observation model's sampler with fix_latent_data(true): inclusion indicators and beta at
     sigma^2 = 1 with a fixed-precision slab on the complete-data statistics the last impute_state
     left (X'QX, X'Q(v - Z alpha), observed steps), stream 3;
  2. every state model's variance draw (ss_student_oracle.StateModelSamplers);
  3. impute_nonstate_latent_data: the family's imputer at eta_t = Z_t'alpha_t + x_t'beta (alpha the
     last state draw, beta the new one) for the observed steps, in the sampler's s-th imputation;
  4. impute_state: the simulation smoother with H_t, then the statistics over the observed steps.
"""
import ctypes as C

import numpy as np

from oracle_lib import BoRng, _dp, _u8, f64, fcol
from ss_student_oracle import StateModelSamplers, Structure, impute_state, oracle_stream_ids, state_model_suf


def observation_variances(q, observed, missing_variance):
    return np.array([1.0 / q[t] if observed[t] else missing_variance for t in range(len(q))])


def draw_sss(o, rng, xtx, xty, mu, prec, pi, gamma, beta, max_flips=-1, shuffle_kind=0):
    """SpikeSlabSampler::draw_model_indicators / draw_beta at sigma^2 = 1 with a fixed-precision
    slab (bo_sss, scales = 0; shuffle_kind 1: BinomialLogitSpikeSlabSampler's own shuffle)
    continuing the stream `rng` (updated in place): (gamma, beta)"""
    L, p = o.lib, len(xty)
    o._declare_sss()
    h = L.bo_sss_create(p, _dp(fcol(xtx)), _dp(f64(xty)), 0, _dp(f64(mu)), _dp(fcol(prec)), _dp(f64(pi)))
    try:
        if shuffle_kind:
            L.bo_sss_set_shuffle_kind.argtypes = [C.c_void_p, C.c_int]
            L.bo_sss_set_shuffle_kind.restype = None
            L.bo_sss_set_shuffle_kind(h, int(shuffle_kind))
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


class SsFamilyOracle(StateModelSamplers):
    """one chain of a latent-data family's StateSpacePosteriorSampler on the device's substreams"""

    MISSING_VARIANCE = None   # the family's
    SHUFFLE_KIND = 0

    def __init__(self, o, X, observed, blocks, mu, prec, pi, seed, chain, gamma0, beta0, max_flips):
        self.X = np.asarray(X, dtype=np.float64)
        self.T, self.p = self.X.shape
        self.obs = (np.ones(self.T, bool) if observed is None else np.asarray(observed).astype(bool))
        self.S = Structure(blocks)
        self.mu, self.prec, self.pi = f64(mu), np.asarray(prec, dtype=np.float64), f64(pi)
        self.max_flips = int(max_flips)
        self.gamma = np.ascontiguousarray(gamma0, dtype=np.uint8).copy()
        self.beta = np.zeros(self.p) if beta0 is None else f64(beta0) * self.gamma
        StateModelSamplers.__init__(self, o, blocks, seed, chain, oracle_stream_ids(o, self.T, blocks))
        self.sss_rng = o.rng_philox(self.seed, self.chain, 3, 0)
        self.v = np.zeros(self.T)
        self.q = self.initial_precisions()
        self.state = None
        self.initialized = False
        self.imputations = 0
        self.rounds = 0

    def initial_precisions(self):
        """q_t of a new model (0 at a missing step)"""
        raise NotImplementedError

    def impute(self, s):
        """the sampler's s-th imputation at eta = offset() + xbeta(): sets v and q (0 at a missing
        step) and takes note of the margins"""
        raise NotImplementedError

    def xbeta(self):
        inc = np.flatnonzero(self.gamma)
        return self.X[:, inc] @ self.beta[inc]

    def offset(self):
        return self.state @ self.S.Z

    def H(self):
        return observation_variances(self.q, self.obs, self.MISSING_VARIANCE)

    def set_latent(self, v, q):
        self.v = np.where(self.obs, np.asarray(v, dtype=float), 0.0)
        self.q = np.where(self.obs, np.asarray(q, dtype=float), 0.0)

    def impute_latent(self, keep=True):
        """impute_nonstate_latent_data; keep = False: the slots are used up and nothing is stored"""
        s = self.imputations
        self.imputations += 1
        if keep:
            self.impute(s)
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
                                         self.gamma, self.beta, self.max_flips, self.SHUFFLE_KIND)

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


def fixed_case():
    """T = 12, a local linear trend, latent values around a random walk, precisions over four
    decades and one missing step"""
    T = 12
    rs = np.random.Generator(np.random.PCG64(6))
    v = np.cumsum(rs.standard_normal(T)) + 1.0
    from cases import general_spec
    blocks = general_spec(v, [("trend",)])
    blocks[0]["initial_sigma"] = np.array([0.55, 0.22])
    S = Structure(blocks)
    var = [blocks[0]["initial_sigma"] ** 2]
    obs = np.ones(T, bool)
    obs[7] = False
    q = np.exp(rs.uniform(np.log(1e-2), np.log(1e2), T))
    return blocks, S, var, v, obs, q
