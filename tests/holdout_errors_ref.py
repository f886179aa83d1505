"""The yardstick of ba_ss_holdout_prediction_errors (bsts.prediction.errors' holdout part,
StateSpaceRegressionModel::one_step_holdout_prediction_errors): a dense scalar Kalman filter over the h rows
that follow a series of T steps, started from a drawn final state alpha (time T - 1), in numpy.longdouble by
default.

    a <- T_{T-1} alpha,  P <- RQR_{T-1}  (a diagonal)
    for i = 0 .. h - 1, t = T + i, every step observed:
        F_i = Z_t'P Z_t + sigma^2,  v_i = y*_i - Z_t'a,  y*_i = newY_i - newX_i'beta (included coefficients)
        update form (with symmetrisation):  a <- T_t a + (T_t PZ / F) v,  P <- T_t P T_t' - (T_t PZ)(T_t PZ)'/F + RQR_t
        filtered form:                      a <- T_t (a + PZ v / F),      P <- T_t (P - PZ PZ'/F) T_t' + RQR_t
    the transition after the last step feeds nothing and is not formed: nothing of time T + h is asked for.

The recursion asks a *view* for Z(t), Tmat(t) and rqr(t) in one floating-point type; a view is made by a
function of the type, so that one model serves the long-double run and the float64 runs of the gate:

    model_view(blocks, params)      prediction_errors_ref.Model: kinds 1-7 (a fixed Z)
    structure_view(S, variances)    ss_state_models_oracle.Structure: the random-walk holiday, the calendar
                                    seasonal and the dynamic regressions (Z_t, T_t and RQR_t by step)

Neither of those two files is edited; what they compute in float64 is converted.
"""
import numpy as np

import prediction_errors_ref as per

U = per.U


class _ModelView:
    def __init__(self, blocks, params, dt):
        self.S = per.Model(blocks, params, dt)
        self.m = self.S.m

    def Z(self, t):
        return self.S.Z

    def Tmat(self, t):
        return self.S.Tmat(t)

    def rqr(self, t):
        return self.S.rqr(t)


class _StructureView:
    def __init__(self, S, variances, dt):
        self.S, self.var, self.dt, self.m = S, variances, dt, S.m

    def Z(self, t):
        return np.asarray(self.S.Z(t), self.dt)

    def Tmat(self, t):
        return np.asarray(self.S.Tmat(t), self.dt)

    def rqr(self, t):
        return np.asarray(self.S.rqr(t, self.var), self.dt)


def model_view(blocks, params):
    """blocks and one chain's parameters as prediction_errors_ref.kalman takes them"""
    return lambda dt: _ModelView(blocks, params, dt)


def structure_view(S, variances):
    """S: a ss_state_models_oracle.Structure; variances: one array per block (its variance parameters)"""
    return lambda dt: _StructureView(S, variances, dt)


def ystar(newY, newX, gamma, beta, dtype=np.longdouble):
    """newY - newX beta over the included coefficients (newX None or without columns: newY)"""
    out = np.asarray(newY, dtype).copy()
    inc = np.flatnonzero(np.asarray(gamma)) if newX is not None else []
    if len(inc):
        out = out - np.asarray(newX, dtype)[:, inc] @ np.asarray(beta, dtype)[inc]
    return out


def initial_condition(V, alpha, T, dtype=np.longdouble):
    """(a, P) the holdout filter starts from: T_{T-1} alpha and diag RQR_{T-1}"""
    return V.Tmat(T - 1) @ np.asarray(alpha, dtype), np.diag(V.rqr(T - 1))


def holdout_filter(view, alpha, T, sigsq, ys, dtype=np.longdouble, form="update"):
    """the filter over ys (= y*, h rows) from the final state alpha of a series of T steps: dict of v, F and std
    (v / sqrt F)"""
    dt = dtype
    V = view(dt)
    h = len(ys)
    ys = np.asarray(ys, dt)
    a, P = initial_condition(V, alpha, T, dt)
    v, F = np.zeros(h, dt), np.zeros(h, dt)
    half = dt(1) / dt(2)
    for i in range(h):
        t = T + i
        Z = V.Z(t)
        PZ = P @ Z
        F[i] = Z @ PZ + dt(sigsq)
        if not F[i] > 0:
            raise FloatingPointError("Found a zero (or negative) forecast variance!")
        v[i] = ys[i] - Z @ a
        if i + 1 == h:
            break
        Tm, Q = V.Tmat(t), np.diag(V.rqr(t))
        if form == "update":
            TPZ = Tm @ PZ
            a = Tm @ a + (TPZ / F[i]) * v[i]
            P = Tm @ P @ Tm.T - np.outer(TPZ, TPZ) / F[i] + Q
            P = half * (P + P.T)
        else:
            a = Tm @ (a + PZ * (v[i] / F[i]))
            P = Tm @ (P - np.outer(PZ, PZ) / F[i]) @ Tm.T + Q
    return dict(v=v, F=F, std=v / np.sqrt(F))


def reference_and_gate(view, alpha, T, sigsq, newY, newX, gamma, beta):
    """The long-double result and the gates of a device comparison, from the reference alone, built as
    prediction_errors_ref.reference_and_gate: the recursion is run in float64 in both algebraic forms (y* in
    float64 too); the larger of their deviations from the long-double result -- v and v / sqrt F scaled by
    sqrt F, F relative -- times 8, at least 64 u.  alpha: the device's final state, an input."""
    return gate_of(reference_runs(view, alpha, T, sigsq, newY, newX, gamma, beta))


def reference_runs(view, alpha, T, sigsq, newY, newX, gamma, beta):
    """the three runs reference_and_gate is made of: (long double, float64 "update", float64 "filtered")"""
    ref = holdout_filter(view, alpha, T, sigsq, ystar(newY, newX, gamma, beta))
    ys64 = ystar(newY, newX, gamma, beta, np.float64)
    return (ref,) + tuple(holdout_filter(view, alpha, T, sigsq, ys64, np.float64, form) for form in ("update", "filtered"))


def gate_of(runs, k=None):
    """(reference, gate) of the first k rows (None: all) from reference_runs of at least k rows: no step of the
    filter looks ahead, so the first k outputs of a longer run ARE the run of horizon k and the runs are shared by
    the horizons of a test"""
    ref = {key: val[:k] for key, val in runs[0].items()}
    sF = np.sqrt(ref["F"])
    dev = dict(v=0.0, F=0.0)
    for f64 in runs[1:]:
        dev["v"] = max(dev["v"], float(np.max(np.abs(f64["v"][:k] - ref["v"]) / sF)))
        dev["F"] = max(dev["F"], float(np.max(np.abs(f64["F"][:k] - ref["F"]) / ref["F"])))
    return ref, {key: max(8.0 * d, 64.0 * U) for key, d in dev.items()}


def device_deviation(ref, errors, variances, std):
    """the device's deviations in the gates' units (std is held to the gate of v)"""
    sF = np.sqrt(ref["F"])
    L = np.longdouble
    return dict(v=float(np.max(np.abs(np.asarray(errors, L) - ref["v"]) / sF)),
                std=float(np.max(np.abs(np.asarray(std, L) - ref["std"]))),
                F=float(np.max(np.abs(np.asarray(variances, L) - ref["F"]) / ref["F"])))


def shifted_blocks(blocks, params, alpha, T):
    """kinds 1-7: the same blocks as a model of its own whose time 0 is the series' time T -- a0 := T_{T-1} alpha,
    P0 := diag RQR_{T-1}, every seasonal's t0 moved by -T -- for prediction_errors_ref.kalman and joint_gaussian.
    (A semilocal trend's third initial component is its parameter mu there: alpha must carry mu in that place.)"""
    V = model_view(blocks, params)(np.longdouble)
    a, P = initial_condition(V, alpha, T)
    out = []
    for b, f, n in zip(blocks, V.S.first, V.S.dims):
        out.append(dict(b, a0=a[f:f + n], P0=np.diag(P)[f:f + n], t0=int(b.get("t0", 0)) - T))
    return out
