"""A restatement of StateSpacePosteriorSampler::draw() for StateSpaceStudentRegressionModel
(bsts family = "student") on the device's substreams, one chain, in Python over the oracle's
primitives: the parity yardstick of ba_ss_student_sweep, built as tests/student_oracle.py is.

One draw() (StateSpacePosteriorSampler.cpp:41-63, StateSpaceStudentPosteriorSampler.cpp:56-126):
  0. the first time: impute_state with the weights in hand (all 1), then the weights once;
  1. the observation model's sampler with fix_latent_data(true) (TRegressionSpikeSlabSampler.cpp:
     41-47): inclusion indicators and beta given sigma^2 on the complete-data statistics the
     last impute_state left (X'WX, X'W(y - Z alpha), (y - Z alpha)'W(y - Z alpha), observed
     steps), stream 3; sigma^2 (DF = observed steps + prior df) and nu (the slice sampler on
     the observed steps' y_t - Z_t'alpha_t - x_t'beta), stream 15, slot r of 4096 in round r;
  2. every state model's variance draw from the statistics of the last state draw, on the
     stream bo_ssm_block_stream_id reports, read sequentially (level, trend, seasonal: one
     gamma draw each);
  3. impute_nonstate_latent_data: w_t = rgamma((nu + 1) / 2, rate (nu + delta_t^2) / 2) with
     delta_t = (y_t - x_t'beta - Z_t'alpha_t) / sigma for the observed steps, stream 31, slot
     s T + t of 256 in the sampler's s-th imputation (the first draw() makes two);
  4. impute_state: the Durbin-Koopman simulation smoother with the per-step observation variance
     H_t = sigma^2 / w_t -- the model's student_marginal_variance() (sigma^2 nu / (nu - 2), or
     1e8 sigma^2 for nu <= 2) where the step is missing or w_t = 0 -- dense, in numpy: the
     normals from the chain's stream 2 through bo_rnorm in the order of bo_ssm_impute_state
     (t = 0: every state model's initial state, then the observation; t >= 1: the state errors
     model by model, then the observation).

dense_posterior() is the same model's joint Gaussian posterior of the whole state path by one
linear solve, written independently of the filter (the yardstick of the yardstick).
"""
import ctypes as C

import numpy as np
from scipy.stats import norm

from oracle_lib import BoRng, _dp, _u8, f64, fcol
from student_oracle import (IMPUTE_STREAM, IMPUTE_STRIDE, SN_STREAM, SN_STRIDE, nu_log_post,
                            slice_draw_nu)

LEVEL, TREND, SEASONAL = 1, 2, 3


def new_season(blk, t):
    """SeasonalStateModel::new_season (SeasonalStateModel.cpp:248-258)"""
    t -= blk["t0"]
    if t < 0:
        t -= blk["duration"] * t
    return t % blk["duration"] == 0


class Structure:
    """the dense matrices of a list of level / trend / seasonal blocks"""

    def __init__(self, blocks):
        for b in blocks:
            assert b["kind"] in (LEVEL, TREND, SEASONAL), "parity cases: level, trend, seasonal"
        self.blocks = blocks
        self.first = np.cumsum([0] + [b["dim"] for b in blocks])[:-1]
        self.m = int(sum(b["dim"] for b in blocks))
        assert self.m <= 20
        self.Z = np.zeros(self.m)
        self.Z[self.first] = 1.0
        self.a0 = np.concatenate([f64(b["a0"]) for b in blocks])
        self.P0 = np.concatenate([f64(b["P0"]) for b in blocks])
        self._T = {}

    def moves(self, b, t):
        return b["kind"] != SEASONAL or new_season(b, t + 1)

    def Tmat(self, t):
        """the transition of the step from t to t + 1"""
        key = tuple(self.moves(b, t) for b in self.blocks)
        if key not in self._T:
            self._T[key] = self._Tmat(t)
        return self._T[key]

    def _Tmat(self, t):
        M = np.eye(self.m)
        for b, f in zip(self.blocks, self.first):
            if b["kind"] == TREND:
                M[f, f + 1] = 1.0
            elif b["kind"] == SEASONAL and self.moves(b, t):
                n = b["dim"]
                S = np.zeros((n, n))
                S[0, :] = -1.0
                S[np.arange(1, n), np.arange(n - 1)] = 1.0
                M[f:f + n, f:f + n] = S
        return M

    def rqr(self, t, sigsq):
        d = np.zeros(self.m)
        for b, f, s in zip(self.blocks, self.first, sigsq):
            if b["kind"] == SEASONAL and not self.moves(b, t):
                continue
            d[f] = s[0]
            if b["kind"] == TREND:
                d[f + 1] = s[1]
        return d


def marginal_variance(sigsq, nu):
    """StateSpaceStudentRegressionModel::student_marginal_variance"""
    return sigsq * nu / (nu - 2) if nu > 2 else sigsq * 1e8


def observation_variances(w, observed, sigsq, nu):
    return np.array([sigsq / w[t] if (observed[t] and w[t] > 0) else marginal_variance(sigsq, nu)
                     for t in range(len(w))])


def gains(S, sigsq, observed, H):
    """the part of ScalarMarginalDistribution::update that does not look at the data
    (ScalarKalmanFilter.cpp:41-83): F_t and K_t (K in the next step's coordinates, 0 where the
    step is missing)"""
    T, m, Z = len(H), S.m, S.Z
    P = np.diag(S.P0)
    F, K = np.zeros(T), np.zeros((T, m))
    for t in range(T):
        Tm = S.Tmat(t)
        PZ = P @ Z
        F[t] = Z @ PZ + H[t]
        assert F[t] > 0
        TPZ = Tm @ PZ
        if observed[t]:
            K[t] = TPZ / F[t]
        P = Tm @ P @ Tm.T - np.outer(TPZ, K[t]) + np.diag(S.rqr(t, sigsq))
        P = .5 * (P + P.T)
    return F, K


def innovations(S, K, y, observed):
    """... and the part that does: v_t = y_t - Z'a_t, a_{t+1} = T a_t + K_t v_t"""
    a = S.a0.copy()
    v = np.zeros(len(y))
    for t in range(len(y)):
        if observed[t]:
            v[t] = y[t] - S.Z @ a
        a = S.Tmat(t) @ a + K[t] * v[t]
    return v


def disturbance_smooth(S, v, F, K):
    """fast_disturbance_smooth (ScalarKalmanFilter.cpp:168-196): r_t (row t), r_{-1}"""
    T, m = len(v), S.m
    r = np.zeros(m)
    out = np.zeros((T, m))
    for t in range(T - 1, -1, -1):
        out[t] = r
        coef = v[t] / F[t] - K[t] @ r
        r = S.Tmat(t).T @ r + S.Z * coef
    return out, r


def simulate_forward(S, sigsq, H, rnorm):
    """simulate_forward (StateSpaceModelBase.cpp:771-790) in the order of bo_ssm_impute_state;
    rnorm(mu, sd) reads the state stream (no draw when sd == 0)"""
    T, m = len(H), S.m
    st = np.zeros((T, m))
    ys = np.zeros(T)
    for t in range(T):
        if t == 0:
            for b, f in zip(S.blocks, S.first):
                if b["kind"] == LEVEL:
                    st[0, f] = rnorm(S.a0[f], np.sqrt(S.P0[f]))
                else:
                    z = [rnorm(0.0, 1.0) for _ in range(b["dim"])]
                    for i in range(b["dim"]):
                        st[0, f + i] = np.sqrt(S.P0[f + i]) * z[i] + S.a0[f + i]
        else:
            eta = np.zeros(m)
            for b, f, s in zip(S.blocks, S.first, sigsq):
                if b["kind"] == LEVEL:
                    eta[f] = rnorm(0.0, np.sqrt(s[0]))
                elif b["kind"] == TREND:
                    z0, z1 = rnorm(0.0, 1.0), rnorm(0.0, 1.0)
                    eta[f], eta[f + 1] = np.sqrt(s[0]) * z0 + 0.0, np.sqrt(s[1]) * z1 + 0.0
                elif new_season(b, t):
                    eta[f] = rnorm(0.0, np.sqrt(s[0]))
            st[t] = S.Tmat(t - 1) @ st[t - 1] + eta
        ys[t] = rnorm(S.Z @ st[t], np.sqrt(H[t]))
    return st, ys


def impute_state(S, sigsq, ystar, observed, H, rnorm, FK=None, simulate=simulate_forward):
    """Base::impute_state (StateSpaceModelBase.cpp:278-291): the state draw, T x m.  The data
    filter and the simulation filter share F_t and K_t (FK: computed already); simulate: the
    simulation of a Structure whose state errors are not the ones above"""
    T = len(ystar)
    F, K = FK if FK is not None else gains(S, sigsq, observed, H)
    v = innovations(S, K, ystar, observed)
    st, ys = simulate(S, sigsq, H, rnorm)
    vs = innovations(S, K, ys, observed)
    r, r0 = disturbance_smooth(S, v, F, K)
    rs, r0s = disturbance_smooth(S, vs, F, K)
    mean_obs = S.a0 + S.P0 * r0
    mean_sim = S.a0 + S.P0 * r0s
    out = st.copy()
    for t in range(T):
        if t > 0:
            Tm, q = S.Tmat(t - 1), S.rqr(t - 1, sigsq)
            mean_obs = Tm @ mean_obs + q * r[t - 1]
            mean_sim = Tm @ mean_sim + q * rs[t - 1]
        out[t] += mean_obs - mean_sim
    return out


def state_model_suf(S, st):
    """observe_state of every state model over the draw: (n, sum of squares) per variance"""
    T = st.shape[0]
    n = [np.zeros(2) for _ in S.blocks]
    ss = [np.zeros(2) for _ in S.blocks]
    for k, (b, f) in enumerate(zip(S.blocks, S.first)):
        if b["kind"] == LEVEL:
            d = np.diff(st[:, f])
            n[k][0], ss[k][0] = T - 1, float(np.sum(d * d))
        elif b["kind"] == TREND:
            # MvnSuf::update_raw, then center_sumsq(0)(i, i) = sumsq_ii + n ybar_i^2
            err = np.stack([st[1:, f] - (st[:-1, f] + st[:-1, f + 1]), st[1:, f + 1] - st[:-1, f + 1]], 1)
            nn, ybar, sumsq = 0.0, np.zeros(2), np.zeros(2)
            for e in err:
                nn += 1.0
                w = (e - ybar) / nn
                ybar = ybar + w
                sumsq = sumsq + w * w * (nn - 1)
                w2 = e - ybar
                sumsq = sumsq + w2 * w2
            n[k][:] = nn
            ss[k][:] = sumsq + ybar * ybar * nn
        else:
            for t in range(1, T):
                if new_season(b, t):
                    delta = st[t, f] + np.sum(st[t - 1, f:f + b["dim"]])
                    n[k][0] += 1
                    ss[k][0] += delta * delta
    return n, ss


def dense_posterior(S, sigsq, ystar, observed, H):
    """the joint Gaussian posterior of (alpha_0, ..., alpha_{T-1}) given the observed y*: the
    prior's mean and covariance built from the recursion alpha_t = T alpha_{t-1} + eta_t, then
    one conditioning solve.  Returns mean (T m) and covariance (T m x T m)."""
    T, m = len(ystar), S.m
    mean = np.zeros((T, m))
    cov = np.zeros((T, m, T, m))
    mean[0] = S.a0
    cov[0, :, 0, :] = np.diag(S.P0)
    for t in range(1, T):
        Tm = S.Tmat(t - 1)
        mean[t] = Tm @ mean[t - 1]
        for s in range(t):
            cov[t, :, s, :] = Tm @ cov[t - 1, :, s, :]
            cov[s, :, t, :] = cov[t, :, s, :].T
        cov[t, :, t, :] = Tm @ cov[t - 1, :, t - 1, :] @ Tm.T + np.diag(S.rqr(t - 1, sigsq))
    mu, Sig = mean.reshape(T * m), cov.reshape(T * m, T * m)
    obs = np.flatnonzero(observed)
    A = np.zeros((len(obs), T * m))
    for i, t in enumerate(obs):
        A[i, t * m:(t + 1) * m] = S.Z
    G = A @ Sig @ A.T + np.diag(np.asarray(H)[obs])
    W = np.linalg.solve(G, A @ Sig).T
    return mu + W @ (np.asarray(ystar)[obs] - A @ mu), Sig - W @ A @ Sig


def bonferroni_bound(count, level=1e-3):
    """two-sided z bound with family-wise level `level` over `count` statistics"""
    return float(norm.isf(level / (2.0 * count)))


def moment_z(draws, mean, cov):
    """z-statistics of the sample mean (d of them) and of the sample covariance's upper
    triangle (d (d + 1) / 2) of n Gaussian draws against (mean, cov); var(S_ij) = (cov_ii
    cov_jj + cov_ij^2) / (n - 1)"""
    n, d = draws.shape
    zm = (draws.mean(0) - mean) / np.sqrt(np.diag(cov) / n)
    S = np.cov(draws, rowvar=False)
    iu = np.triu_indices(d)
    dg = np.diag(cov)
    zc = (S - cov)[iu] / np.sqrt((np.outer(dg, dg) + cov * cov)[iu] / (n - 1))
    return zm, zc


def fixed_case():
    """T = 12, a local linear trend, weights over four decades, a weight of exactly 0 on an
    observed step and one missing step"""
    T = 12
    rs = np.random.Generator(np.random.PCG64(5))
    y = np.cumsum(rs.standard_normal(T)) + 3.0
    from cases import general_spec
    blocks = general_spec(y, [("trend",)])
    blocks[0]["initial_sigma"] = np.array([0.55, 0.22])
    S = Structure(blocks)
    var = [blocks[0]["initial_sigma"] ** 2]
    obs = np.ones(T, bool)
    obs[7] = False
    w = np.exp(rs.uniform(np.log(1e-2), np.log(1e2), T))
    w[3] = 0.0
    sigsq, nu = 0.6, 5.0
    H = observation_variances(w, obs, sigsq, nu)
    return blocks, S, var, y, obs, w, sigsq, nu, H


def oracle_stream_ids(o, T, blocks):
    """the stream of every variance sampler of a level / trend / seasonal list, per block, as
    bo_ssm_block_stream_id reports it (a handle on a series of zeros: the ids depend on the list alone)"""
    L = o.lib
    dummy = dict(b=np.zeros(1), ominv=np.eye(1), pi=np.full(1, 0.5), df=1.0, sigma_guess=1.0)
    h = o._ssg_build(np.zeros(T), np.zeros((T, 1)), None, dummy, blocks)
    ids = [[L.bo_ssm_block_stream_id(h, k, v) for v in range(len(b["initial_sigma"]))] for k, b in enumerate(blocks)]
    L.bo_ssm_destroy.argtypes = [C.c_void_p]
    L.bo_ssm_destroy(h)
    return ids


class StateModelSamplers:
    """the state models' half of one chain, whatever the observation model: every model's variances,
    their priors, statistics and samplers' streams (stream_ids: per block, one id per variance), and the
    state stream"""

    def __init__(self, o, blocks, seed, chain, stream_ids):
        self.o, self.L = o, o.lib
        self.L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
        self.L.bo_rnorm.restype = C.c_double
        self.blocks = blocks
        self.seed, self.chain = int(seed), int(chain)
        self.var = [f64(b["initial_sigma"]) ** 2 for b in blocks]
        self.var_prior = [(2 * (f64(b["df"]) / 2.0), 2 * (f64(b["df"]) * f64(b["sigma_guess"]) ** 2 / 2.0),
                           f64(b["sigma_upper_limit"])) for b in blocks]
        self.var_rng = [[o.rng_philox(self.seed, self.chain, sid, 0) for sid in row] for row in stream_ids]
        self.suf_n = [np.zeros(2) for _ in blocks]
        self.suf_ss = [np.zeros(2) for _ in blocks]
        self.state_rng = o.rng_philox(self.seed, self.chain, 2, 0)

    def _rnorm(self, mu, sd):
        return self.L.bo_rnorm(C.byref(self.state_rng), float(mu), float(sd))

    def _draw_variance(self, rng, DF, SS, smax):
        if np.isinf(smax):
            return 1.0 / self.o.gammas(rng, DF / 2, SS / 2, 1)[0]
        return 1.0 / self.o.trun_gammas(rng, DF / 2, SS / 2, 1.0 / (smax * smax), 1)[0]

    def draw_block_variances(self, k):
        pdf, pss, smax = self.var_prior[k]
        for v in range(len(self.var[k])):
            d = self._draw_variance(self.var_rng[k][v], self.suf_n[k][v] + pdf[v], self.suf_ss[k][v] + pss[v], smax[v])
            if self.blocks[k]["kind"] == TREND:
                d = 1.0 / (1.0 / d)   # ZeroMeanMvnIndependenceSampler: siginv = 1 / draw, Sigma its inverse
            self.var[k][v] = d

    def draw_state_models(self):
        """every state model's sampler, in model order"""
        for k in range(len(self.blocks)):
            self.draw_block_variances(k)


class SsStudentOracle(StateModelSamplers):
    """one chain of StateSpaceStudentPosteriorSampler on the device's substreams"""

    def __init__(self, o, y, X, observed, blocks, mu, prec, pi, seed, chain, gamma0, beta0=None,
                 sigsq0=1.0, nu0=30.0, nu_prior=(0, 0.1, 100.0), sigma_prior=(1.0, 1.0),
                 sigma_max=np.inf, max_flips=-1):
        o._declare_sss()
        o.lib.bo_rng_slot.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
        o.lib.bo_rng_slot.restype = None
        self.y, self.X = f64(y), np.asarray(X, dtype=np.float64)
        self.T, self.p = self.X.shape
        self.obs = (np.ones(self.T, bool) if observed is None else np.asarray(observed).astype(bool))
        self.S = Structure(blocks)
        self.mu, self.prec, self.pi = f64(mu), np.asarray(prec, dtype=np.float64), f64(pi)
        self.gamma = np.ascontiguousarray(gamma0, dtype=np.uint8).copy()
        self.beta = np.zeros(self.p) if beta0 is None else f64(beta0) * self.gamma
        self.sigsq, self.nu, self.dx = float(sigsq0), float(nu0), 1.0
        self.nu_prior = nu_prior
        df, guess = sigma_prior
        self.prior_df, self.prior_ss = 2 * (df / 2.0), 2 * (df * guess * guess / 2.0)
        self.sigma_max, self.max_flips = float(sigma_max), int(max_flips)
        StateModelSamplers.__init__(self, o, blocks, seed, chain, oracle_stream_ids(o, self.T, blocks))
        self.sss_rng = o.rng_philox(self.seed, self.chain, 3, 0)
        self.w = np.where(self.obs, 1.0, 0.0)
        self.state = None
        self.initialized = False
        self.imputations = 0
        self.rounds = 0
        self.margin = np.inf        # the slice comparisons'
        self.flip_margin = np.inf   # (filled by callers that look at the indicator draws' margins)

    # ---- pieces -------------------------------------------------------------------
    def _slot(self, stream, index, stride):
        r = BoRng()
        self.L.bo_rng_seed_philox(C.byref(r), self.seed, self.chain, stream, 0)
        self.L.bo_rng_slot(C.byref(r), int(index), int(stride))
        return r

    def xbeta(self):
        inc = np.flatnonzero(self.gamma)
        return self.X[:, inc] @ self.beta[inc]

    def offset(self):
        return self.state @ self.S.Z

    def H(self):
        return observation_variances(self.w, self.obs, self.sigsq, self.nu)

    def impute_weights(self):
        o, T, s = self.o, self.T, self.imputations
        r = self.y - self.xbeta() - self.offset()
        sd = np.sqrt(self.sigsq)
        w = np.zeros(T)
        for t in range(T):
            if not self.obs[t]:
                continue
            delta = r[t] / sd
            rng = self._slot(IMPUTE_STREAM, s * T + t, IMPUTE_STRIDE)
            w[t] = o.gammas(rng, 0.5 * (self.nu + 1), 0.5 * (self.nu + delta * delta), 1)[0]
        self.imputations += 1
        self.w = w
        return w

    def impute_state(self):
        ystar = self.y - self.xbeta()
        self.state = impute_state(self.S, self.var, ystar, self.obs, self.H(), self._rnorm)
        self.suf_n, self.suf_ss = state_model_suf(self.S, self.state)
        # update_complete_data_sufficient_statistics: observed steps, response y - Z alpha
        ob = self.obs
        z = (self.y - self.offset())[ob]
        Xo, wo = self.X[ob], self.w[ob]
        Xw = Xo * wo[:, None]
        self.xtx, self.xty, self.yty = Xo.T @ Xw, Xw.T @ z, float(np.dot(z * wo, z))
        self.nobs = int(ob.sum())
        return self.state

    def draw_observation_model(self):
        L, o, p = self.L, self.o, self.p
        h = L.bo_sss_create(p, _dp(fcol(self.xtx)), _dp(f64(self.xty)), 1, _dp(self.mu), _dp(fcol(self.prec)),
                            _dp(self.pi))
        try:
            L.bo_sss_set_options(h, -1, self.max_flips)
            L.bo_sss_set_state(h, _u8(self.gamma), _dp(f64(self.beta)))
            C.memmove(L.bo_sss_rng(h), C.byref(self.sss_rng), C.sizeof(BoRng))
            st = L.bo_sss_draw_model_indicators(h, float(self.sigsq))
            if st == 0:
                st = L.bo_sss_draw_beta(h, float(self.sigsq))
            if st:
                raise RuntimeError("SpikeSlabSampler status %d" % st)
            g, b = np.zeros(p, dtype=np.uint8), np.zeros(p)
            L.bo_sss_get_state(h, _u8(g), _dp(b))
            C.memmove(C.byref(self.sss_rng), L.bo_sss_rng(h), C.sizeof(BoRng))
        finally:
            L.bo_sss_destroy(h)
        self.gamma, self.beta = g, b
        wsse = float(b @ self.xtx @ b - 2 * (b @ self.xty) + self.yty)
        DF, SS = self.nobs + self.prior_df, wsse + self.prior_ss
        rng = self._slot(SN_STREAM, self.rounds, SN_STRIDE)
        if np.isinf(self.sigma_max):
            self.sigsq = 1.0 / o.gammas(rng, DF / 2, SS / 2, 1)[0]
        else:
            self.sigsq = 1.0 / o.trun_gammas(rng, DF / 2, SS / 2, 1.0 / self.sigma_max ** 2, 1)[0]
        r = (self.y - self.offset() - self.xbeta())[self.obs]
        sigma = np.sqrt(self.sigsq)
        u = (r / sigma) ** 2
        n_log_sigma = self.nobs * np.log(sigma)
        logf = lambda nu: nu_log_post(nu, u, n_log_sigma, self.nu_prior)   # noqa: E731
        unif = lambda: L.bo_unif(C.byref(rng))                               # noqa: E731
        rexp1 = lambda: 1.0 * L.bo_exp_rand(C.byref(rng))                    # noqa: E731
        self.nu, self.dx, m = slice_draw_nu(unif, rexp1, logf, self.nu, self.dx)
        self.margin = min(self.margin, m)

    def draw(self):
        if not self.initialized:
            self.impute_state()
            self.initialized = True
            # (these weights are replaced below before any statistic reads them: the statistics
            # in hand stay those of the weights the state was drawn with)
            keep = self.w
            self.impute_weights()
            self.w = keep
        self.draw_observation_model()
        self.draw_state_models()
        self.impute_weights()
        self.impute_state()
        self.rounds += 1
        return self.gamma.copy(), self.beta.copy(), self.sigsq, self.nu
