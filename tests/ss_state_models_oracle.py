"""The one recursion of the restatements whose observation row Z_t, transition T_t and state-error variance
RQR_t change from step to step: the state half of StateSpacePosteriorSampler::draw() for a list of state
models, on the device's substreams, one chain, in Python over the oracle's primitives.  The parity yardstick
of the general structural kernel's holiday, calendar seasonal and dynamic regression instances.

A list is a list of block dicts (cases.general_spec's; holiday_block, calendar_block and dynreg_block of
tests/ss_holiday_oracle.py, tests/ss_calendar_seasonal_oracle.py and tests/ss_dynreg_oracle.py, whose
docstrings state each model and its conventions).  Every kind of block is a class below that states what is
its own -- its row of Z_t, its transition and whether it moves at t, its part of RQR_t, its initial-state and
state-error draws, its observe_state and its sampler ids -- and nothing else: Structure assembles the
matrices from the blocks, and simulate_forward, impute_state, state_model_suf, forecast and
block_stream_ids are loops over them.

The normals of simulate_forward come from the chain's stream 2 in the order of the device: t = 0: the
initial state of every model, then the observation; t >= 1: the state errors model by model, then the
observation.  forecast() restates simulate_multiplex_forecast (StateSpaceRegressionModel.cpp:257-278) on
the chain's forecast stream (id 5): forecast step i advances the state with the transition and state errors
of time T - 2 + i (advance_to_timestamp, StateSpaceModelBase.cpp:455-459) and observes it with Z of time
T + i.  dense_posterior() is the joint Gaussian posterior of the whole state path by one linear solve,
written independently of the filter.

tests/ss_student_oracle.py is the independent twin of this file (a fixed Z, level / trend / seasonal only):
the CPU tests compare the two where they must agree, so neither is built on the other.
"""
import ctypes as C

import numpy as np

LEVEL, TREND, SEASONAL, TRIG, HOLIDAY, CALENDAR_SEASONAL = 1, 2, 3, 6, 10, 11
DYNREG = "dynamic_regression"
LOG_2PI = 1.8378770664093454835606594728112


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def new_season(blk, t):
    """SeasonalStateModel::new_season (SeasonalStateModel.cpp:248-258)"""
    t -= blk["t0"]
    if t < 0:
        t -= blk["duration"] * t
    return t % blk["duration"] == 0


# ---- the kinds of blocks ---------------------------------------------------------------------------------
class Block:
    """what the kinds share, and the defaults most of them keep.  `s` is the block's variances; error(t, ..)
    and forecast_error(t, ..) are the error of the step into time t; rqr(t, ..) is the variance of the
    error of the step from t to t + 1; suf(x) is observe_state over the block's columns x of a draw, (n, sum
    of squares) per variance slot; sampler_ids(ahead) counts the earlier members of the block's family"""

    members, nslots = 1, 2

    def __init__(self, b):
        self.b, self.dim = b, int(b["dim"])
        self.a0, self.P0 = f64(b["a0"]), f64(b["P0"])

    def unit(self, k=0, value=1.0):
        e = np.zeros(self.dim)
        if k >= 0:
            e[k] = value
        return e

    def z(self, t):
        return self.unit()

    def moves(self, t):
        return False

    def transition(self, t):
        return np.eye(self.dim)

    def rqr(self, t, s):
        return self.unit(0, s[0])

    def initial_state(self, rnorm):
        """rmvn_mt(mean, diagonal variance): dim standard normals, then sqrt(P0) z + a0"""
        z = [rnorm(0.0, 1.0) for _ in range(self.dim)]
        return [np.sqrt(self.P0[i]) * z[i] + self.a0[i] for i in range(self.dim)]

    def forecast_error(self, t, s, rnorm):
        return self.error(t, s, rnorm)

    def variance(self, draw):
        return draw

    @staticmethod
    def one_slot(n, ss):
        """the statistics of a block with one variance"""
        return np.array([n, 0.0]), np.array([ss, 0.0])


class Level(Block):
    """local level: its initial state is one rnorm(a0, sqrt(P0)), not a scaled standard normal"""

    family = "level"

    def initial_state(self, rnorm):
        return [rnorm(self.a0[0], np.sqrt(self.P0[0]))]

    def error(self, t, s, rnorm):
        return [rnorm(0.0, np.sqrt(s[0]))]

    def suf(self, x):
        d = np.diff(x[:, 0])
        return self.one_slot(x.shape[0] - 1, float(np.sum(d * d)))

    def sampler_ids(self, ahead):
        return [1 + 16 * ahead]


class Trend(Block):
    """local linear trend: two variances, of one family with the level"""

    family = "level"

    def moves(self, t):
        return True

    def transition(self, t):
        return np.array([[1.0, 1.0], [0.0, 1.0]])

    def rqr(self, t, s):
        return np.array([s[0], s[1]], dtype=np.float64)

    def error(self, t, s, rnorm):
        z0, z1 = rnorm(0.0, 1.0), rnorm(0.0, 1.0)
        return [np.sqrt(s[0]) * z0 + 0.0, np.sqrt(s[1]) * z1 + 0.0]

    def suf(self, x):
        # MvnSuf::update_raw, then center_sumsq(0)(i, i) = sumsq_ii + n ybar_i^2
        err = np.stack([x[1:, 0] - (x[:-1, 0] + x[:-1, 1]), x[1:, 1] - x[:-1, 1]], 1)
        nn, ybar, sumsq = 0.0, np.zeros(2), np.zeros(2)
        for e in err:
            nn += 1.0
            w = (e - ybar) / nn
            ybar = ybar + w
            sumsq = sumsq + w * w * (nn - 1)
            w2 = e - ybar
            sumsq = sumsq + w2 * w2
        return np.full(2, nn), sumsq + ybar * ybar * nn

    def sampler_ids(self, ahead):
        return [1 + 16 * ahead, 6 + 16 * ahead]

    def variance(self, draw):
        return 1.0 / (1.0 / draw)   # ZeroMeanMvnIndependenceSampler: siginv = 1 / draw, Sigma its inverse


class Seasonal(Block):
    """seasonal (kind 3: a season starts by the duration rule) and calendar seasonal (kind 11: by the block's
    flags; a time past the calendar's end starts none): it moves, and has an error, only into a new season"""

    family = "seasonal"

    def __init__(self, b):
        super().__init__(b)
        self.calendar = np.asarray(b["calendar"], np.uint8) if b["kind"] == CALENDAR_SEASONAL else None
        n = self.dim
        self.T = np.zeros((n, n))
        self.T[0, :] = -1.0
        self.T[np.arange(1, n), np.arange(n - 1)] = 1.0

    def starts(self, t):
        if self.calendar is None:
            return new_season(self.b, t)
        return bool(self.calendar[t]) if t < len(self.calendar) else False

    def moves(self, t):
        return self.starts(t + 1)

    def transition(self, t):
        return self.T if self.moves(t) else np.eye(self.dim)

    def rqr(self, t, s):
        return self.unit(0, s[0]) if self.moves(t) else np.zeros(self.dim)

    def error(self, t, s, rnorm):
        return self.unit(0, rnorm(0.0, np.sqrt(s[0]))) if self.starts(t) else np.zeros(self.dim)

    def suf(self, x):
        n, ss = np.zeros(2), np.zeros(2)
        for t in range(1, x.shape[0]):
            if self.starts(t):
                delta = x[t, 0] + np.sum(x[t - 1])
                n[0] += 1
                ss[0] += delta * delta
        return n, ss

    def sampler_ids(self, ahead):
        return [7 + 16 * ahead]


class Trig(Block):
    """trigonometric seasonal: a rotation per frequency, one variance for every component"""

    family = "trig"

    def __init__(self, b):
        super().__init__(b)
        rot = f64(b["rotations"])
        self.T = np.eye(self.dim)
        for q in range(0, self.dim, 2):
            c, s = rot[q], rot[q + 1]
            self.T[q:q + 2, q:q + 2] = [[c, s], [-s, c]]

    def z(self, t):
        z = np.zeros(self.dim)
        z[::2] = 1.0
        return z

    def moves(self, t):
        return True

    def transition(self, t):
        return self.T

    def rqr(self, t, s):
        return np.full(self.dim, s[0], dtype=np.float64)

    def error(self, t, s, rnorm):
        return [rnorm(0.0, np.sqrt(s[0])) for _ in range(self.dim)]

    def suf(self, x):
        e = x[1:] - x[:-1] @ self.T.T
        return self.one_slot(self.dim * (x.shape[0] - 1), float(np.sum(e * e)))

    def sampler_ids(self, ahead):
        return [13 + 16 * ahead]


class Holiday(Block):
    """random-walk holiday: position(t) in {-1, 0 .. width - 1} is the component active at time t (times
    past the calendar: an error)"""

    family = "holiday"

    def position(self, t):
        return int(self.b["calendar"][t])

    def z(self, t):
        return self.unit(self.position(t))

    def rqr(self, t, s):
        return self.unit(self.position(t + 1), s[0])

    def error(self, t, s, rnorm):
        z = rnorm(0.0, 1.0)   # (one per step, active or not: the position of a step's normals is a closed form of t)
        return self.unit(self.position(t), np.sqrt(s[0]) * z)

    def forecast_error(self, t, s, rnorm):
        """drawn only where time t is active, as the reference does"""
        k = self.position(t)
        return self.unit(k, rnorm(0.0, np.sqrt(s[0]))) if k >= 0 else np.zeros(self.dim)

    def suf(self, x):
        n, ss = np.zeros(2), np.zeros(2)
        for t in range(1, x.shape[0]):
            p = self.position(t)
            if p >= 0:
                delta = x[t, p] - x[t - 1, p]
                n[0] += 1
                ss[0] += delta * delta
        return n, ss

    def sampler_ids(self, ahead):
        return [8 + 16 * ahead]


class DynamicRegression(Block):
    """dynamic regression: predictors[t] is the block's row of Z_t; a variance, and a sampler, per coefficient"""

    family = "dynamic coefficient"

    def __init__(self, b):
        super().__init__(b)
        self.members = self.nslots = self.dim

    def z(self, t):
        return self.b["predictors"][t]

    def rqr(self, t, s):
        return np.asarray(s)[:self.dim]

    def error(self, t, s, rnorm):
        return [np.sqrt(s[i]) * rnorm(0.0, 1.0) for i in range(self.dim)]   # (one per coefficient, whatever sigma_i)

    def forecast_error(self, t, s, rnorm):
        return [rnorm(0.0, np.sqrt(s[i])) for i in range(self.dim)]

    def suf(self, x):
        ss = np.zeros(self.dim)
        for t in range(1, x.shape[0]):
            delta = x[t] - x[t - 1]
            ss += delta * delta
        return np.full(self.dim, float(x.shape[0] - 1)), ss

    def sampler_ids(self, ahead):
        return [10 + 16 * (ahead + i) for i in range(self.dim)]


KINDS = {LEVEL: Level, TREND: Trend, SEASONAL: Seasonal, CALENDAR_SEASONAL: Seasonal, TRIG: Trig, HOLIDAY: Holiday,
         DYNREG: DynamicRegression}


class Structure:
    """the dense matrices of a list of blocks, assembled from the blocks; Z, T and RQR by step"""

    def __init__(self, blocks):
        self.blocks = blocks
        self.parts = [KINDS[b["kind"]](b) for b in blocks]
        self.first = np.cumsum([0] + [b["dim"] for b in blocks])[:-1]
        self.span = [slice(int(f), int(f) + k.dim) for f, k in zip(self.first, self.parts)]
        self.m = int(sum(b["dim"] for b in blocks))
        self.a0 = np.concatenate([k.a0 for k in self.parts])
        self.P0 = np.concatenate([k.P0 for k in self.parts])
        self._T = {}

    def Z(self, t):
        z = np.zeros(self.m)
        for k, sl in zip(self.parts, self.span):
            z[sl] = k.z(t)
        return z

    def Tmat(self, t):
        """the transition of the step from t to t + 1"""
        key = tuple(k.moves(t) for k in self.parts)
        if key not in self._T:
            M = np.zeros((self.m, self.m))
            for k, sl in zip(self.parts, self.span):
                M[sl, sl] = k.transition(t)
            self._T[key] = M
        return self._T[key]

    def rqr(self, t, sigsq):
        """the diagonal of RQR_t, the variance of the state error of the step from t to t + 1"""
        d = np.zeros(self.m)
        for k, sl, s in zip(self.parts, self.span, sigsq):
            d[sl] = k.rqr(t, s)
        return d


# ---- the filter and the smoother: they ask the Structure alone -------------------------------------------
def gains(S, sigsq, observed, H):
    """the part of ScalarMarginalDistribution::update that does not look at the data
    (ScalarKalmanFilter.cpp:41-83): F_t and K_t (K in the next step's coordinates, 0 where the
    step is missing)"""
    T, m = len(H), S.m
    P = np.diag(S.P0)
    F, K = np.zeros(T), np.zeros((T, m))
    for t in range(T):
        Tm, Z = S.Tmat(t), S.Z(t)
        PZ = P @ Z
        F[t] = Z @ PZ + H[t]
        assert F[t] > 0
        TPZ = Tm @ PZ
        if observed[t]:
            K[t] = TPZ / F[t]
        q = S.rqr(t, sigsq) if t + 1 < T else np.zeros(m)   # (P_T is not used; the calendar may end at T)
        P = Tm @ P @ Tm.T - np.outer(TPZ, K[t]) + np.diag(q)
        P = .5 * (P + P.T)
    return F, K


def innovations(S, K, y, observed):
    """... and the part that does: v_t = y_t - Z_t'a_t, a_{t+1} = T a_t + K_t v_t"""
    a = S.a0.copy()
    v = np.zeros(len(y))
    for t in range(len(y)):
        if observed[t]:
            v[t] = y[t] - S.Z(t) @ a
        a = S.Tmat(t) @ a + K[t] * v[t]
    return v


def log_likelihood(v, F, observed):
    ob = np.asarray(observed).astype(bool)
    return float(np.sum(-0.5 * (LOG_2PI + np.log(F[ob]) + v[ob] ** 2 / F[ob])))


def kalman(S, sigsq, sigsq_obs, ystar, observed, dtype=np.longdouble, form="update"):
    """the forward filter in one floating-point type and one of two algebraic forms of the variance
    update -- "update": T P T' - (T PZ) K' + RQR (the reference's); "filtered": T (P - PZ PZ' / F) T' +
    RQR (the device's) --: dict of v, F, std (v / sqrt F, 0 at a missing step) and loglik.  The gate of
    a device comparison comes from the float64 runs' deviations from the long-double run
    (reference_and_gate), as in tests/prediction_errors_ref.py."""
    dt = dtype
    T, m = len(ystar), S.m
    ys = np.asarray(ystar, dt)
    P = np.diag(np.asarray(S.P0, dt))
    a = np.asarray(S.a0, dt)
    v, F = np.zeros(T, dt), np.zeros(T, dt)
    var = [np.asarray(x, dt) for x in sigsq]
    for t in range(T):
        Tm, Z = np.asarray(S.Tmat(t), dt), np.asarray(S.Z(t), dt)
        PZ = P @ Z
        F[t] = Z @ PZ + dt(sigsq_obs)
        q = np.asarray(S.rqr(t, var), dt) if t + 1 < T else np.zeros(m, dt)
        if observed[t]:
            v[t] = ys[t] - Z @ a
            if form == "update":
                K = (Tm @ PZ) / F[t]
                a = Tm @ a + K * v[t]
                P = Tm @ P @ Tm.T - np.outer(Tm @ PZ, K) + np.diag(q)
            else:
                a = Tm @ (a + PZ * (v[t] / F[t]))
                P = Tm @ (P - np.outer(PZ, PZ) / F[t]) @ Tm.T + np.diag(q)
        else:
            a = Tm @ a
            P = Tm @ P @ Tm.T + np.diag(q)
        P = (P + P.T) / dt(2)
    ob = np.asarray(observed).astype(bool)
    std = np.where(ob, v / np.sqrt(F), dt(0))
    ll = np.sum(-(dt(LOG_2PI) + np.log(F[ob]) + v[ob] ** 2 / F[ob]) / dt(2))
    return dict(v=v, F=F, std=std, loglik=ll)


def reference_and_gate(S, sigsq, sigsq_obs, y, X, gamma, beta, observed):
    """the long-double result and the gates of tests/prediction_errors_ref.py's reference_and_gate:
    the larger deviation of the two float64 forms from it (v scaled by sqrt F, F and the log likelihood
    relative) times 8, at least 64 u"""
    U = float(np.finfo(np.float64).eps) / 2
    inc = np.flatnonzero(gamma)

    def ystar(dt):
        return np.asarray(y, dt) - np.asarray(X, dt)[:, inc] @ np.asarray(beta, dt)[inc]

    ref = kalman(S, sigsq, sigsq_obs, ystar(np.longdouble), observed)
    sF = np.sqrt(ref["F"])
    dev = dict(v=0.0, F=0.0, loglik=0.0)
    for form in ("update", "filtered"):
        r = kalman(S, sigsq, sigsq_obs, ystar(np.float64), observed, np.float64, form)
        dev["v"] = max(dev["v"], float(np.max(np.abs(r["v"] - ref["v"]) / sF)))
        dev["F"] = max(dev["F"], float(np.max(np.abs(r["F"] - ref["F"]) / ref["F"])))
        dev["loglik"] = max(dev["loglik"], float(abs(r["loglik"] - ref["loglik"]) / abs(ref["loglik"])))
    return ref, {k: max(8.0 * d, 64.0 * U) for k, d in dev.items()}


def disturbance_smooth(S, v, F, K):
    """fast_disturbance_smooth (ScalarKalmanFilter.cpp:168-196): r_t (row t), r_{-1}"""
    T, m = len(v), S.m
    r = np.zeros(m)
    out = np.zeros((T, m))
    for t in range(T - 1, -1, -1):
        out[t] = r
        coef = v[t] / F[t] - K[t] @ r
        r = S.Tmat(t).T @ r + S.Z(t) * coef
    return out, r


# ---- the draws: loops over the blocks ---------------------------------------------------------------------
def simulate_forward(S, sigsq, H, rnorm):
    """simulate_forward (StateSpaceModelBase.cpp:771-790) in the device's order; rnorm(mu, sd) reads
    the state stream (no draw when sd == 0)"""
    T, m = len(H), S.m
    st = np.zeros((T, m))
    ys = np.zeros(T)
    for t in range(T):
        if t == 0:
            for k, sl in zip(S.parts, S.span):
                st[0, sl] = k.initial_state(rnorm)
        else:
            eta = np.zeros(m)
            for k, sl, s in zip(S.parts, S.span, sigsq):
                eta[sl] = k.error(t, s, rnorm)
            st[t] = S.Tmat(t - 1) @ st[t - 1] + eta
        ys[t] = rnorm(S.Z(t) @ st[t], np.sqrt(H[t]))
    return st, ys


def impute_state(S, sigsq, ystar, observed, H, rnorm, FK=None):
    """Base::impute_state (StateSpaceModelBase.cpp:278-291): the state draw, T x m.  The data
    filter and the simulation filter share F_t and K_t (FK: computed already)"""
    T = len(ystar)
    F, K = FK if FK is not None else gains(S, sigsq, observed, H)
    v = innovations(S, K, ystar, observed)
    st, ys = simulate_forward(S, sigsq, H, rnorm)
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
    suf = [k.suf(st[:, sl]) for k, sl in zip(S.parts, S.span)]
    return [n for n, _ in suf], [ss for _, ss in suf]


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
        A[i, t * m:(t + 1) * m] = S.Z(t)
    G = A @ Sig @ A.T + np.diag(np.asarray(H)[obs])
    W = np.linalg.solve(G, A @ Sig).T
    return mu + W @ (np.asarray(ystar)[obs] - A @ mu), Sig - W @ A @ Sig


def forecast(S, T, last_state, sigsq, sigsq_obs, xbeta, rnorm):
    """simulate_multiplex_forecast from the state of time T - 1; xbeta: the regression's part of the
    len(xbeta) forecast steps; rnorm(mu, sd) reads the chain's forecast stream"""
    state = np.array(last_state, dtype=float)
    out = np.zeros(len(xbeta))
    for i in range(len(xbeta)):
        tm = T - 2 + i
        eta = np.zeros(S.m)
        for k, sl, s in zip(S.parts, S.span, sigsq):
            eta[sl] = k.forecast_error(tm + 1, s, rnorm)
        state = S.Tmat(tm) @ state + eta
        out[i] = rnorm(S.Z(tm + 2) @ state, np.sqrt(sigsq_obs)) + xbeta[i]
    return out


def block_stream_ids(blocks):
    """the engine's sampler ids of the blocks' variance samplers: level 1, slope 6, seasonal 7, holiday 8,
    dynamic coefficient 10, trig 13 for the first of its family (level and trend are one, so are the two
    seasonals), + 16 per earlier member"""
    ahead, out = {}, []
    for k in Structure(blocks).parts:
        out.append(k.sampler_ids(ahead.get(k.family, 0)))
        ahead[k.family] = ahead.get(k.family, 0) + k.members
    return out


class StateOracle:
    """the state half of one chain's StateSpacePosteriorSampler::draw for a list of the blocks above, on
    the device's substreams; the regression half (the adjusted series y - X beta, the observation
    variance) is given by the caller.

    margin: every variance draw is repeated, from a copy of its generator, with its sum of squares
    moved by the relative amount MARGIN_PROBE up and down.  A rejection sampler's decision that sits
    within that distance of its threshold shows as a different number of uniforms read or a draw that
    jumps; `margin` stays inf while none does and drops to 0 when one did."""

    MARGIN_PROBE = 1e-9

    def __init__(self, o, T, observed, blocks, seed, chain):
        self.o, self.L = o, o.lib
        L = self.L
        L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.bo_rnorm.restype = C.c_double
        self.T = int(T)
        self.obs = np.ones(self.T, bool) if observed is None else np.asarray(observed).astype(bool)
        self.blocks = blocks
        self.S = Structure(blocks)
        self.seed, self.chain = int(seed), int(chain)
        self.var = [np.array(b["initial_sigma"], dtype=float) ** 2 for b in blocks]
        self.var_prior = [(2 * (f64(b["df"]) / 2.0), 2 * (f64(b["df"]) * f64(b["sigma_guess"]) ** 2 / 2.0),
                           f64(b["sigma_upper_limit"])) for b in blocks]
        self.var_rng = [[o.rng_philox(self.seed, self.chain, sid, 0) for sid in row]
                        for row in block_stream_ids(blocks)]
        self.state_rng = o.rng_philox(self.seed, self.chain, 2, 0)
        self.forecast_rng = o.rng_philox(self.seed, self.chain, 5, 0)
        self.suf_n = [np.zeros(k.nslots) for k in self.S.parts]
        self.suf_ss = [np.zeros(k.nslots) for k in self.S.parts]
        self.state = None
        self.margin = np.inf

    def _rnorm(self, mu, sd):
        return self.L.bo_rnorm(C.byref(self.state_rng), float(mu), float(sd))

    def _rnorm_forecast(self, mu, sd):
        return self.L.bo_rnorm(C.byref(self.forecast_rng), float(mu), float(sd))

    def impute_state(self, ystar, sigsq_obs):
        H = np.full(self.T, float(sigsq_obs))
        self.state = impute_state(self.S, self.var, f64(ystar), self.obs, H, self._rnorm)
        self.suf_n, self.suf_ss = state_model_suf(self.S, self.state)
        return self.state

    def _variance(self, rng, DF, SS, smax):
        if np.isinf(smax):
            return 1.0 / self.o.gammas(rng, DF / 2, SS / 2, 1)[0]
        return 1.0 / self.o.trun_gammas(rng, DF / 2, SS / 2, 1.0 / (smax * smax), 1)[0]

    def _draw_variance(self, rng, DF, SS, smax):
        copies = []
        for scale in (1 - self.MARGIN_PROBE, 1 + self.MARGIN_PROBE):
            r = type(rng)()
            C.memmove(C.byref(r), C.byref(rng), C.sizeof(rng))
            copies.append((self._variance(r, DF, SS * scale, smax), bytes(r)))
        d = self._variance(rng, DF, SS, smax)
        for dc, pos in copies:
            if pos != bytes(rng) or not abs(dc - d) <= 1e-6 * abs(d):
                self.margin = 0.0
        return d

    def draw_state_models(self):
        """every state model's sampler, in model order; a block whose statistics are empty (a holiday
        without an active step after t = 0: n = 0 and ss = 0) draws from its prior"""
        for k, model in enumerate(self.S.parts):
            pdf, pss, smax = self.var_prior[k]
            for v in range(len(self.var[k])):
                d = self._draw_variance(self.var_rng[k][v], self.suf_n[k][v] + pdf[v], self.suf_ss[k][v] + pss[v],
                                        smax[v])
                self.var[k][v] = model.variance(d)

    def prediction_errors(self, ystar, sigsq_obs):
        """one_step_prediction_errors at the parameters in hand: v_t, F_t, the log likelihood"""
        H = np.full(self.T, float(sigsq_obs))
        F, K = gains(self.S, self.var, self.obs, H)
        v = innovations(self.S, K, f64(ystar), self.obs)
        return v, F, log_likelihood(v, F, self.obs)

    def forecast(self, last_state, sigsq_obs, xbeta):
        return forecast(self.S, self.T, last_state, self.var, sigsq_obs, xbeta, self._rnorm_forecast)

    def positions(self):
        """where the chain's state, forecast and variance streams stand (the generators' raw bytes)"""
        return (bytes(self.state_rng), bytes(self.forecast_rng),
                [[bytes(r) for r in row] for row in self.var_rng])
