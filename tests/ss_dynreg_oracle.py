"""A restatement of the state half of StateSpacePosteriorSampler::draw() for a list of state models that
holds DynamicRegressionStateModel blocks with the independent random-walk sampler (StateModels/
DynamicRegressionStateModel.cpp, bsts AddDynamicRegression with DynamicRegressionRandomWalkOptions;
ba_ss_add_dynamic_regression), on the device's substreams, one chain: the parity yardstick of the general
structural kernel's DR instances.  Built on tests/ss_holiday_oracle.py's per-step forms -- Z(t), Tmat(t),
rqr(t, .) -- whose gains, innovations, disturbance smoother, dense posterior and long-double filter serve
unchanged; what names the kinds of blocks (the simulation, the statistics, the forecast, the sampler ids) is
restated here.

The dynamic regression block (d coefficients, predictors x_t for every time t):
  T_t = I;  Z_t = x_t on the block's components;  RQR_t = diag(sigma_1^2 .. sigma_d^2), every step;
  observe_state(then, now, t), t = 1 .. T - 1: (now[i] - then[i])^2 into coefficient i's sum, n = T - 1 each;
  initial state rmvn_mt(mean, diagonal variance): d standard normals, sqrt(P0) z + a0;
  one GenericGaussianVarianceSampler(ChisqModel(df_i, guess_i)) with a sigma upper limit per coefficient.

CONVENTIONS (the device's; BOOM draws the d variances from one generator): variance i of the block reads
sampler id 10 + 16 x (the dynamic coefficients ahead of it in the list); the block reads d standard normals
of stream 2 per step t >= 1, scaled by sigma_i, whatever the sigmas.

forecast(): forecast step i advances the block with d errors (rnorm(0, sigma_i), in order) and observes
the new state with row T + i of the predictors.
"""
import ctypes as C

import numpy as np

import ss_holiday_oracle as sho
from ss_holiday_oracle import LEVEL, TREND, SEASONAL, TRIG, f64, new_season

DYNREG = "dynamic_regression"


def dynreg_block(predictors, sdy, initial_sigma=None, a0=None):
    """a dynamic regression block dict with bsts-style defaults per coefficient: sd prior guess 0.01 sd(y),
    df 0.01, upper limit sd(y); initial state N(a0 or 0, sd(y)^2)"""
    x = f64(predictors)
    d = x.shape[1]
    sig = np.full(d, 0.3) if initial_sigma is None else f64(initial_sigma)
    return dict(kind=DYNREG, dim=d, predictors=x, nseasons=0, duration=1, t0=0, lags=0, df=np.full(d, 0.01),
                sigma_guess=np.full(d, 0.01 * sdy), sigma_upper_limit=np.full(d, sdy), initial_sigma=sig,
                initial_phi=np.zeros(0), a0=np.zeros(d) if a0 is None else f64(a0), P0=np.full(d, sdy * sdy))


class Structure(sho.Structure):
    """the dense matrices of a list of level / trend / seasonal / trig / dynamic regression blocks"""

    def __init__(self, blocks):
        for b in blocks:
            assert b["kind"] in (LEVEL, TREND, SEASONAL, TRIG, DYNREG)
        self.blocks = blocks
        self.first = np.cumsum([0] + [b["dim"] for b in blocks])[:-1]
        self.m = int(sum(b["dim"] for b in blocks))
        self.a0 = np.concatenate([f64(b["a0"]) for b in blocks])
        self.P0 = np.concatenate([f64(b["P0"]) for b in blocks])
        self._T = {}
        self._plain = [dict(b, kind=LEVEL) if b["kind"] == DYNREG else b for b in blocks]

    def moves(self, b, t):
        return False if b["kind"] == DYNREG else super().moves(b, t)

    def Z(self, t):
        z = np.zeros(self.m)
        for b, f in zip(self.blocks, self.first):
            if b["kind"] == DYNREG:
                z[f:f + b["dim"]] = b["predictors"][t]
            elif b["kind"] == TRIG:
                z[f:f + b["dim"]:2] = 1.0
            else:
                z[f] = 1.0
        return z

    def rqr(self, t, sigsq):
        d = np.zeros(self.m)
        for b, f, s in zip(self.blocks, self.first, sigsq):
            if b["kind"] == DYNREG:
                d[f:f + b["dim"]] = np.asarray(s)[:b["dim"]]
            elif b["kind"] == TRIG:
                d[f:f + b["dim"]] = s[0]
            elif b["kind"] == SEASONAL:
                if self.moves(b, t):
                    d[f] = s[0]
            else:
                d[f] = s[0]
                if b["kind"] == TREND:
                    d[f + 1] = s[1]
        return d


def simulate_forward(S, sigsq, H, rnorm):
    """simulate_forward in the device's order; rnorm(mu, sd) reads the state stream (no draw when sd == 0)"""
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
                if b["kind"] == DYNREG:
                    for i in range(b["dim"]):   # (one per coefficient, whatever sigma_i: the convention above)
                        eta[f + i] = np.sqrt(s[i]) * rnorm(0.0, 1.0)
                elif b["kind"] == LEVEL:
                    eta[f] = rnorm(0.0, np.sqrt(s[0]))
                elif b["kind"] == TREND:
                    z0, z1 = rnorm(0.0, 1.0), rnorm(0.0, 1.0)
                    eta[f], eta[f + 1] = np.sqrt(s[0]) * z0 + 0.0, np.sqrt(s[1]) * z1 + 0.0
                elif b["kind"] == TRIG:
                    for i in range(b["dim"]):
                        eta[f + i] = rnorm(0.0, np.sqrt(s[0]))
                elif new_season(b, t):
                    eta[f] = rnorm(0.0, np.sqrt(s[0]))
            st[t] = S.Tmat(t - 1) @ st[t - 1] + eta
        ys[t] = rnorm(S.Z(t) @ st[t], np.sqrt(H[t]))
    return st, ys


def impute_state(S, sigsq, ystar, observed, H, rnorm, FK=None):
    """Base::impute_state: ss_holiday_oracle's, with this module's simulation"""
    T = len(ystar)
    F, K = FK if FK is not None else sho.gains(S, sigsq, observed, H)
    v = sho.innovations(S, K, ystar, observed)
    st, ys = simulate_forward(S, sigsq, H, rnorm)
    vs = sho.innovations(S, K, ys, observed)
    r, r0 = sho.disturbance_smooth(S, v, F, K)
    rs, r0s = sho.disturbance_smooth(S, vs, F, K)
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


def nslots(b):
    return b["dim"] if b["kind"] == DYNREG else 2


def state_model_suf(S, st):
    """observe_state of every state model over the draw: (n, sum of squares) per variance; a dynamic
    regression has one of each per coefficient, summed in time order"""
    T = st.shape[0]
    n, ss = sho.state_model_suf(sho.Structure(S._plain), st)   # (the other kinds; a stand-in level per dynamic block)
    for k, (b, f) in enumerate(zip(S.blocks, S.first)):
        if b["kind"] != DYNREG:
            continue
        d = b["dim"]
        n[k], ss[k] = np.full(d, float(T - 1)), np.zeros(d)
        for t in range(1, T):
            delta = st[t, f:f + d] - st[t - 1, f:f + d]
            ss[k] += delta * delta
    return n, ss


def forecast(S, T, last_state, sigsq, sigsq_obs, xbeta, rnorm):
    state = np.array(last_state, dtype=float)
    out = np.zeros(len(xbeta))
    for i in range(len(xbeta)):
        tm = T - 2 + i
        eta = np.zeros(S.m)
        for b, f, s in zip(S.blocks, S.first, sigsq):
            if b["kind"] == DYNREG:
                for q in range(b["dim"]):
                    eta[f + q] = rnorm(0.0, np.sqrt(s[q]))
            elif b["kind"] == LEVEL:
                eta[f] = rnorm(0.0, np.sqrt(s[0]))
            elif b["kind"] == TREND:
                z0, z1 = rnorm(0.0, 1.0), rnorm(0.0, 1.0)
                eta[f], eta[f + 1] = np.sqrt(s[0]) * z0 + 0.0, np.sqrt(s[1]) * z1 + 0.0
            elif b["kind"] == TRIG:
                for q in range(b["dim"]):
                    eta[f + q] = rnorm(0.0, np.sqrt(s[0]))
            elif new_season(b, tm + 1):
                eta[f] = rnorm(0.0, np.sqrt(s[0]))
        state = S.Tmat(tm) @ state + eta
        out[i] = rnorm(S.Z(tm + 2) @ state, np.sqrt(sigsq_obs)) + xbeta[i]
    return out


def block_stream_ids(blocks):
    """the engine's sampler ids: ss_holiday_oracle's for the other kinds; coefficient i of a dynamic
    regression reads 10 + 16 x (the dynamic coefficients ahead of it in the list)"""
    plain = iter(sho.block_stream_ids([b for b in blocks if b["kind"] != DYNREG]))
    out, ahead = [], 0
    for b in blocks:
        if b["kind"] == DYNREG:
            out.append([10 + 16 * (ahead + i) for i in range(b["dim"])])
            ahead += b["dim"]
        else:
            out.append(next(plain))
    return out


class DynRegOracle(sho.HolidayOracle):
    """the state half of one chain's StateSpacePosteriorSampler::draw for a list that holds dynamic
    regressions, on the device's substreams (margin: as HolidayOracle's)"""

    def __init__(self, o, T, observed, blocks, seed, chain):
        self.o, self.L = o, o.lib
        self.L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
        self.L.bo_rnorm.restype = C.c_double
        self.T = int(T)
        self.obs = np.ones(self.T, bool) if observed is None else np.asarray(observed).astype(bool)
        self.seed, self.chain = int(seed), int(chain)
        self.state_rng = o.rng_philox(self.seed, self.chain, 2, 0)
        self.forecast_rng = o.rng_philox(self.seed, self.chain, 5, 0)
        self.state = None
        self.margin = np.inf
        self.blocks = blocks
        self.S = Structure(blocks)
        self.var = [np.array(b["initial_sigma"], dtype=float) ** 2 for b in blocks]
        self.var_prior = [(2 * (f64(b["df"]) / 2.0), 2 * (f64(b["df"]) * f64(b["sigma_guess"]) ** 2 / 2.0),
                           f64(b["sigma_upper_limit"])) for b in blocks]
        self.var_rng = [[o.rng_philox(self.seed, self.chain, sid, 0) for sid in row]
                        for row in block_stream_ids(blocks)]
        self.suf_n = [np.zeros(nslots(b)) for b in blocks]
        self.suf_ss = [np.zeros(nslots(b)) for b in blocks]

    def impute_state(self, ystar, sigsq_obs):
        H = np.full(self.T, float(sigsq_obs))
        self.state = impute_state(self.S, self.var, f64(ystar), self.obs, H, self._rnorm)
        self.suf_n, self.suf_ss = state_model_suf(self.S, self.state)
        return self.state

    def forecast(self, last_state, sigsq_obs, xbeta):
        return forecast(self.S, self.T, last_state, self.var, sigsq_obs, xbeta, self._rnorm_forecast)
