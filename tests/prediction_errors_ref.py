"""The yardstick of ba_ss_prediction_errors: a dense scalar Kalman filter over explicit T_t, Z and
RQR_t matrices, written from the formulas (ScalarMarginalDistribution::update) for the eight state
model kinds the engine takes, in numpy.longdouble by default.

    F_t = Z'P Z + sigma^2,  v_t = y*_t - Z'a  (0 at a missing step)
    update form (with symmetrisation):  a <- T a + (T PZ / F) v,  P <- T P T' - (T PZ)(T PZ)'/F + RQR
    filtered form:                      a <- T (a + PZ v / F),    P <- T (P - PZ PZ'/F) T' + RQR
    missing step:                       a <- T a,                 P <- T P T' + RQR
    loglik = sum over the observed steps of log N(v_t; 0, F_t)

The blocks are the dicts capi.ss_set_state_models and tests/cases.py use.  The parameters of a
chain are a list with one dict per block: var (its variance parameters: two for kinds 2, 7 and 8,
none for kind 5, one otherwise), phi (kind 4: the coefficients; kind 7: (phi, mu)), and for kind 8
weights = (level, slope), T each -- entry t divides the variances of the step t -> t + 1.

joint_gaussian() is the same model's joint normal distribution of the observed series, by
unrolling the state equation into a mean vector and a covariance matrix: not a filter.
"""
import numpy as np

LEVEL, TREND, SEASONAL, AR, INTERCEPT, TRIG, SEMILOCAL, STUDENT_TREND = 1, 2, 3, 4, 5, 6, 7, 8
LOG_2PI = np.longdouble("1.8378770664093454835606594728112353")


def block_dim(b):
    k = int(b["kind"])
    if k in (LEVEL, INTERCEPT):
        return 1
    if k in (TREND, STUDENT_TREND):
        return 2
    if k == SEASONAL:
        return int(b["nseasons"]) - 1
    if k == AR:
        return int(b["lags"])
    if k == TRIG:
        return len(b["rotations"])
    if k == SEMILOCAL:
        return 3
    raise ValueError("state model kind %r" % k)


def initial_params(blocks):
    """the parameters a new engine starts from"""
    out = []
    for b in blocks:
        k = int(b["kind"])
        d = dict(var=np.asarray(b["initial_sigma"], float) ** 2 if k != INTERCEPT else np.zeros(0), phi=None)
        if k == AR:
            phi = np.zeros(int(b["lags"]))
            given = np.asarray(b.get("initial_phi", np.zeros(0)), float)
            phi[:len(given)] = given
            d["phi"] = phi
        elif k == SEMILOCAL:
            d["phi"] = np.array([b["slope_priors"][5], b["slope_priors"][4]])   # (phi, mu)
        out.append(d)
    return out


def new_season(b, t):
    """does time t start a new season?  (t - time of the first observation) is a multiple of the duration"""
    return (t - int(b.get("t0", 0))) % int(b["duration"]) == 0


class Model:
    def __init__(self, blocks, params, dtype=np.longdouble):
        self.blocks, self.params, self.dt = blocks, params, dtype
        self.dims = [block_dim(b) for b in blocks]
        self.first = [int(x) for x in np.cumsum([0] + self.dims)[:-1]]
        self.m = int(sum(self.dims))
        dt = dtype
        self.Z = np.zeros(self.m, dt)
        self.a0 = np.zeros(self.m, dt)
        self.P0 = np.zeros(self.m, dt)
        for b, q, f, n in zip(blocks, params, self.first, self.dims):
            k = int(b["kind"])
            if k == TRIG:
                self.Z[f:f + n:2] = 1
            else:
                self.Z[f] = 1
            self.a0[f:f + n] = np.asarray(b["a0"], dt)[:n]
            self.P0[f:f + n] = np.asarray(b["P0"], dt)[:n]
            if k == SEMILOCAL:
                self.a0[f + 2] = dt(q["phi"][1])   # the component IS the slope's long-run mean
                self.P0[f + 2] = 0

    def Tmat(self, t):
        """the transition of the step t -> t + 1"""
        dt = self.dt
        M = np.eye(self.m, dtype=dt)
        for b, q, f, n in zip(self.blocks, self.params, self.first, self.dims):
            k = int(b["kind"])
            if k in (TREND, STUDENT_TREND):
                M[f, f + 1] = 1
            elif k == SEASONAL:
                if new_season(b, t + 1):
                    S = np.zeros((n, n), dt)
                    S[0, :] = -1
                    for i in range(1, n):
                        S[i, i - 1] = 1
                    M[f:f + n, f:f + n] = S
            elif k == AR:
                S = np.zeros((n, n), dt)
                S[0, :] = np.asarray(q["phi"], dt)
                for i in range(1, n):
                    S[i, i - 1] = 1
                M[f:f + n, f:f + n] = S
            elif k == TRIG:
                rot = np.asarray(b["rotations"], dt)
                for j in range(n // 2):
                    c, s = rot[2 * j], rot[2 * j + 1]
                    M[f + 2 * j:f + 2 * j + 2, f + 2 * j:f + 2 * j + 2] = np.array([[c, s], [-s, c]], dt)
            elif k == SEMILOCAL:
                phi = dt(q["phi"][0])
                M[f:f + 3, f:f + 3] = np.array([[1, 1, 0], [0, phi, 1 - phi], [0, 0, 1]], dt)
        return M

    def rqr(self, t):
        """the diagonal of the state error variance of the step t -> t + 1"""
        dt = self.dt
        d = np.zeros(self.m, dt)
        for b, q, f, n in zip(self.blocks, self.params, self.first, self.dims):
            k = int(b["kind"])
            var = np.asarray(q["var"], dt)
            if k == LEVEL:
                d[f] = var[0]
            elif k == TREND:
                d[f], d[f + 1] = var[0], var[1]
            elif k == STUDENT_TREND:
                lw, sw = q["weights"]
                d[f], d[f + 1] = var[0] / dt(lw[t]), var[1] / dt(sw[t])
            elif k == SEASONAL:
                if new_season(b, t + 1):
                    d[f] = var[0]
            elif k == AR:
                d[f] = var[0]
            elif k == TRIG:
                d[f:f + n] = var[0]
            elif k == SEMILOCAL:
                d[f], d[f + 1] = var[0], var[1]
        return d


def ystar(y, X, gamma, beta, dtype=np.longdouble):
    """y - X beta over the included coefficients"""
    inc = np.flatnonzero(np.asarray(gamma))
    out = np.asarray(y, dtype).copy()
    if len(inc):
        out = out - np.asarray(X, dtype)[:, inc] @ np.asarray(beta, dtype)[inc]
    return out


def kalman(blocks, params, sigsq, ys, observed, dtype=np.longdouble, form="update"):
    """the filter: dict of v (prediction errors), F (forecast variances), std (v / sqrt F, 0 at a
    missing step) and loglik"""
    dt = dtype
    S = Model(blocks, params, dt)
    T = len(ys)
    obs = np.ones(T, bool) if observed is None else np.asarray(observed).astype(bool)
    ys = np.asarray(ys, dt)
    a, P, Z = S.a0.copy(), np.diag(S.P0), S.Z
    v, F = np.zeros(T, dt), np.zeros(T, dt)
    ll = dt(0)
    half = dt(1) / dt(2)
    for t in range(T):
        Tm = S.Tmat(t)
        PZ = P @ Z
        F[t] = Z @ PZ + dt(sigsq)
        if not F[t] > 0:
            raise FloatingPointError("Found a zero (or negative) forecast variance!")
        Q = np.diag(S.rqr(t))
        if obs[t]:
            v[t] = ys[t] - Z @ a
            ll = ll - half * (dt(LOG_2PI) + np.log(F[t]) + v[t] * v[t] / F[t])
            if form == "update":
                TPZ = Tm @ PZ
                a = Tm @ a + (TPZ / F[t]) * v[t]
                P = Tm @ P @ Tm.T - np.outer(TPZ, TPZ) / F[t] + Q
                P = half * (P + P.T)
            else:
                a = Tm @ (a + PZ * (v[t] / F[t]))
                P = Tm @ (P - np.outer(PZ, PZ) / F[t]) @ Tm.T + Q
        else:
            a = Tm @ a
            P = Tm @ P @ Tm.T + Q
            if form == "update":
                P = half * (P + P.T)
    std = np.where(obs, v / np.sqrt(F), 0)
    return dict(v=v, F=F, std=std, loglik=ll)


def _cholesky(A):
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def joint_gaussian(blocks, params, sigsq, ys, observed, dtype=np.longdouble):
    """the observed series as ONE multivariate normal: dict of loglik (its log density) and
    white (the Cholesky-whitened residuals L^{-1}(y - mu), one per observed step, in order)"""
    dt = dtype
    S = Model(blocks, params, dt)
    T, m = len(ys), S.m
    obs = np.ones(T, bool) if observed is None else np.asarray(observed).astype(bool)
    # the state path: means and the covariance of every pair of times, from the state equation
    mean = np.zeros((T, m), dt)
    cov = np.zeros((T, m, T, m), dt)
    mean[0] = S.a0
    cov[0, :, 0, :] = np.diag(S.P0)
    for t in range(T - 1):
        Tm = S.Tmat(t)
        mean[t + 1] = Tm @ mean[t]
        for s in range(t + 1):
            cov[t + 1, :, s, :] = Tm @ cov[t, :, s, :]
            cov[s, :, t + 1, :] = cov[t + 1, :, s, :].T
        cov[t + 1, :, t + 1, :] = Tm @ cov[t, :, t, :] @ Tm.T + np.diag(S.rqr(t))
    idx = np.flatnonzero(obs)
    mu = np.array([S.Z @ mean[t] for t in idx], dt)
    V = np.array([[S.Z @ cov[s, :, t, :] @ S.Z for t in idx] for s in idx], dt)
    V = V + dt(sigsq) * np.eye(len(idx), dtype=dt)
    L = _cholesky(V)
    r = np.asarray(ys, dt)[idx] - mu
    w = np.zeros(len(idx), dt)
    for i in range(len(idx)):
        w[i] = (r[i] - L[i, :i] @ w[:i]) / L[i, i]
    ll = -(dt(len(idx)) * dt(LOG_2PI)) / 2 - np.sum(np.log(np.diag(L))) - (w @ w) / 2
    return dict(loglik=ll, white=w)


U = float(np.finfo(np.float64).eps) / 2


def reference_and_gate(blocks, params, sigsq, y, X, gamma, beta, observed):
    """The long-double result and the gates of a device comparison, from the reference alone: the
    recursion is run in float64 in both algebraic forms (y* in float64 too); the larger of their
    deviations from the long-double result -- v and v / sqrt F scaled by sqrt F, F and the log
    likelihood relative -- times 8, at least 64 u."""
    ref = kalman(blocks, params, sigsq, ystar(y, X, gamma, beta), observed)
    sF = np.sqrt(ref["F"])
    dev = dict(v=0.0, F=0.0, loglik=0.0)
    for form in ("update", "filtered"):
        f64 = kalman(blocks, params, sigsq, ystar(y, X, gamma, beta, np.float64), observed, np.float64, form)
        dev["v"] = max(dev["v"], float(np.max(np.abs(f64["v"] - ref["v"]) / sF)))
        dev["F"] = max(dev["F"], float(np.max(np.abs(f64["F"] - ref["F"]) / ref["F"])))
        dev["loglik"] = max(dev["loglik"], float(abs(f64["loglik"] - ref["loglik"]) / abs(ref["loglik"])))
    gate = {k: max(8.0 * d, 64.0 * U) for k, d in dev.items()}
    return ref, gate


def device_deviation(ref, errors, variances, std, loglik):
    """the device's deviations in the gates' units"""
    sF = np.sqrt(ref["F"])
    L = np.longdouble
    return dict(v=float(np.max(np.abs(np.asarray(errors, L) - ref["v"]) / sF)),
                std=float(np.max(np.abs(np.asarray(std, L) - ref["std"]))),
                F=float(np.max(np.abs(np.asarray(variances, L) - ref["F"]) / ref["F"])),
                loglik=float(abs(L(loglik) - ref["loglik"]) / abs(ref["loglik"])))
