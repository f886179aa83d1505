"""A restatement of the state half of StateSpacePosteriorSampler::draw() for a list of state models
that holds RandomWalkHolidayStateModel blocks (StateModels/RandomWalkHolidayStateModel.cpp, bsts
AddRandomWalkHoliday; ba_ss_add_state_model kind 10), on the device's substreams, one chain, in
Python over the oracle's primitives: the parity yardstick of the general structural kernel's
holiday instances.  Built as tests/ss_student_oracle.py is, but with an observation row Z_t and a
state-error variance RQR_t that change from step to step -- every function below is written for a
time-varying Z (ss_student_oracle's fix Z as one vector; tests/test_ss_holiday_cpu.py compares the two
where they must agree).

The holiday block (width w, a calendar k(t) in {-1, 0 .. w - 1} for every time t):
  T_t = I;  Z_t = e_k(t) where t is active, 0 elsewhere;
  the step into t adds N(0, sigma^2) to component k(t) where t is active, nothing elsewhere:
  RQR_{t-1} = sigma^2 e_k(t) e_k(t)';
  observe_state(then, now, t), t = 1 .. T - 1, active t only: the GaussianSuf of now[k(t)] - then[k(t)];
  initial state rmvn_mt(mean, diagonal variance): w standard normals, sqrt(P0) z + a0;
  ZeroMeanGaussianConjSampler(df, sigma_guess) with a sigma upper limit, on sampler id 8 + 16 per
  earlier holiday block.

The normals of simulate_forward come from the chain's stream 2 in the order of the device: t = 0: the
initial state of every model, then the observation; t >= 1: the state errors model by model, then the
observation.  CONVENTION: a holiday block reads ONE standard normal per step t >= 1, whether the step
is active or not (an inactive step's is read and dropped), so that the position of a step's normals in
the stream is a closed form of t.  (The reference, on its own generator, draws on the active steps
only; the parity yardstick is this restatement on the device's substreams.)

The other blocks -- local level, local linear trend, seasonal, trig -- are those of the GPU cases.

forecast() restates simulate_multiplex_forecast (StateSpaceRegressionModel.cpp:257-278) on the chain's
forecast stream (id 5): forecast step i advances the state with the transition and state errors of
time T - 2 + i (advance_to_timestamp, StateSpaceModelBase.cpp:455-459: the error lands on the calendar's
position at T - 1 + i, drawn only where that time is active, as the reference does) and observes it
with Z of time T + i.

dense_posterior() is the joint Gaussian posterior of the whole state path by one linear solve, written
independently of the filter.
"""
import ctypes as C

import numpy as np

LEVEL, TREND, SEASONAL, TRIG, HOLIDAY = 1, 2, 3, 6, 10
LOG_2PI = 1.8378770664093454835606594728112


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def new_season(blk, t):
    """SeasonalStateModel::new_season (SeasonalStateModel.cpp:248-258)"""
    t -= blk["t0"]
    if t < 0:
        t -= blk["duration"] * t
    return t % blk["duration"] == 0


def holiday_block(width, calendar, sdy, initial_sigma=0.6, a0=None):
    """a kind 10 block dict with bsts-style defaults (as cases.general_spec's): sd prior guess
    0.01 sd(y), df 0.01, upper limit sd(y); initial state N(a0 or 0, sd(y)^2)"""
    return dict(kind=HOLIDAY, width=int(width), dim=int(width), calendar=np.asarray(calendar, dtype=np.int32),
                nseasons=0, duration=1, t0=0, lags=0, df=np.array([0.01]), sigma_guess=np.array([0.01 * sdy]),
                sigma_upper_limit=np.array([sdy]), initial_sigma=np.array([float(initial_sigma)]),
                initial_phi=np.zeros(0), a0=np.zeros(width) if a0 is None else f64(a0),
                P0=np.full(width, sdy * sdy))


class Structure:
    """the dense matrices of a list of level / trend / seasonal / trig / holiday blocks; Z and RQR by step"""

    def __init__(self, blocks):
        for b in blocks:
            assert b["kind"] in (LEVEL, TREND, SEASONAL, TRIG, HOLIDAY)
        self.blocks = blocks
        self.first = np.cumsum([0] + [b["dim"] for b in blocks])[:-1]
        self.m = int(sum(b["dim"] for b in blocks))
        self.a0 = np.concatenate([f64(b["a0"]) for b in blocks])
        self.P0 = np.concatenate([f64(b["P0"]) for b in blocks])
        self._T = {}

    def position(self, b, t):
        """a holiday block's position at time t, -1: inactive (times past the calendar: an error)"""
        return int(b["calendar"][t])

    def moves(self, b, t):
        if b["kind"] == HOLIDAY or b["kind"] == LEVEL:
            return False
        return b["kind"] != SEASONAL or new_season(b, t + 1)

    def Z(self, t):
        z = np.zeros(self.m)
        for b, f in zip(self.blocks, self.first):
            if b["kind"] == HOLIDAY:
                k = self.position(b, t)
                if k >= 0:
                    z[f + k] = 1.0
            elif b["kind"] == TRIG:
                z[f:f + b["dim"]:2] = 1.0
            else:
                z[f] = 1.0
        return z

    def Tmat(self, t):
        """the transition of the step from t to t + 1"""
        key = tuple(self.moves(b, t) for b in self.blocks)
        if key not in self._T:
            M = np.eye(self.m)
            for b, f in zip(self.blocks, self.first):
                if b["kind"] == TREND:
                    M[f, f + 1] = 1.0
                elif b["kind"] == TRIG:
                    rot = f64(b["rotations"])
                    for q in range(0, b["dim"], 2):
                        c, s = rot[q], rot[q + 1]
                        M[f + q:f + q + 2, f + q:f + q + 2] = [[c, s], [-s, c]]
                elif b["kind"] == SEASONAL and self.moves(b, t):
                    n = b["dim"]
                    S = np.zeros((n, n))
                    S[0, :] = -1.0
                    S[np.arange(1, n), np.arange(n - 1)] = 1.0
                    M[f:f + n, f:f + n] = S
            self._T[key] = M
        return self._T[key]

    def rqr(self, t, sigsq):
        """the diagonal of RQR_t, the variance of the state error of the step from t to t + 1"""
        d = np.zeros(self.m)
        for b, f, s in zip(self.blocks, self.first, sigsq):
            if b["kind"] == HOLIDAY:
                k = self.position(b, t + 1)
                if k >= 0:
                    d[f + k] = s[0]
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


def simulate_forward(S, sigsq, H, rnorm):
    """simulate_forward (StateSpaceModelBase.cpp:771-790) in the device's order; rnorm(mu, sd) reads
    the state stream (no draw when sd == 0)"""
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
                if b["kind"] == HOLIDAY:
                    z = rnorm(0.0, 1.0)   # (one per step, active or not: the convention above)
                    k = S.position(b, t)
                    if k >= 0:
                        eta[f + k] = np.sqrt(s[0]) * z
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
    T = st.shape[0]
    n = [np.zeros(2) for _ in S.blocks]
    ss = [np.zeros(2) for _ in S.blocks]
    for k, (b, f) in enumerate(zip(S.blocks, S.first)):
        if b["kind"] == HOLIDAY:
            for t in range(1, T):
                p = S.position(b, t)
                if p >= 0:
                    delta = st[t, f + p] - st[t - 1, f + p]
                    n[k][0] += 1
                    ss[k][0] += delta * delta
        elif b["kind"] == LEVEL:
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
        elif b["kind"] == TRIG:
            d = b["dim"]
            R = S.Tmat(0)[f:f + d, f:f + d]
            e = st[1:, f:f + d] - st[:-1, f:f + d] @ R.T
            n[k][0], ss[k][0] = d * (T - 1), float(np.sum(e * e))
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
        for b, f, s in zip(S.blocks, S.first, sigsq):
            if b["kind"] == HOLIDAY:
                k = S.position(b, tm + 1)
                if k >= 0:
                    eta[f + k] = rnorm(0.0, np.sqrt(s[0]))
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
    """the engine's sampler ids of the blocks' variance samplers: level 1, slope 6, seasonal 7, holiday
    8, trig 13 for the first block of its family (level and trend are one), + 16 per earlier member"""
    fam = {LEVEL: 0, SEASONAL: 0, TRIG: 0, HOLIDAY: 0}
    base = {SEASONAL: 7, TRIG: 13, HOLIDAY: 8}
    out = []
    for b in blocks:
        k = b["kind"]
        if k in base:
            out.append([base[k] + 16 * fam[k]])
            fam[k] += 1
        elif k == LEVEL:
            out.append([1 + 16 * fam[LEVEL]])
            fam[LEVEL] += 1
        else:
            out.append([1 + 16 * fam[LEVEL], 6 + 16 * fam[LEVEL]])
            fam[LEVEL] += 1
    return out


class HolidayOracle:
    """the state half of one chain's StateSpacePosteriorSampler::draw for a list that holds
    random-walk holidays, on the device's substreams; the regression half (the adjusted series
    y - X beta, the observation variance) is given by the caller.

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
        self.suf_n = [np.zeros(2) for _ in blocks]
        self.suf_ss = [np.zeros(2) for _ in blocks]
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
        """every state model's sampler, in model order; a holiday block without an active step after
        t = 0 has n = 0 and ss = 0: its draw is the prior's"""
        for k, b in enumerate(self.blocks):
            pdf, pss, smax = self.var_prior[k]
            for v in range(len(self.var[k])):
                d = self._draw_variance(self.var_rng[k][v], self.suf_n[k][v] + pdf[v], self.suf_ss[k][v] + pss[v],
                                        smax[v])
                if b["kind"] == TREND:
                    d = 1.0 / (1.0 / d)   # ZeroMeanMvnIndependenceSampler: siginv = 1 / draw, Sigma its inverse
                self.var[k][v] = d

    def prediction_errors(self, ystar, sigsq_obs):
        """one_step_prediction_errors at the parameters in hand: v_t, F_t, the log likelihood"""
        H = np.full(self.T, float(sigsq_obs))
        F, K = gains(self.S, self.var, self.obs, H)
        v = innovations(self.S, K, f64(ystar), self.obs)
        return v, F, log_likelihood(v, F, self.obs)

    def forecast(self, last_state, sigsq_obs, xbeta):
        return forecast(self.S, self.T, last_state, self.var, sigsq_obs, xbeta, self._rnorm_forecast)
