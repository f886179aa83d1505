"""A restatement of RegressionHolidayStateModel (StateModels/RegressionHolidayStateModel.cpp, bsts
AddRegressionHoliday; ba_ss_add_regression_holiday) in numpy, one chain: observe_state, sample_posterior,
the forecast's offset and a whole round of StateSpacePosteriorSampler::draw in the reference's order.

The model: H holidays, holiday h with a window of w_h days and w_h coefficients; state dimension 1 with
T = 1, RQR = 0, a0 = 1, P0 = 0; Z_t = coefficient[h(t)][d(t)] where a holiday is active, else 0.  Here a
model is a dict (reg_holiday_model) whose calendar holds one flat index offset_h + day per time, or -1.

Because the state is deterministic, the state draw of a list with such models is the state draw of the list
without them on the series y_t - (the models' effects at t): the state half below is
ss_state_models_oracle's StateOracle, fed that series.  augmented_structure() builds the model the
long way -- a constant component per model with Z_t = its coefficient -- for the test that the two agree.

CONVENTIONS (the device's; the reference draws from the model's own generator): the coefficients of all
models of a chain are drawn in (model, coefficient) order from Philox sampler id 162 at one position per
chain; the effects come off the series in model order, (..((y - e_0) - e_1) ..); a coefficient's total is
summed in time order.

The order of a round (StateSpacePosteriorSampler::draw): the observation model's draw, every state model's
draw -- the coefficients with the sigma^2 just drawn and the totals of the last impute_state, formed with
the beta of before that draw --, then impute_state with its observe_state calls.
"""
import ctypes as C

import numpy as np

from ss_state_models_oracle import LEVEL, Structure, f64

REGHOLIDAY = "regression_holiday"
STREAM = 162


def reg_holiday_model(widths, prior, calendar, coefficients=None):
    n = int(np.sum(widths))
    cal = np.asarray(calendar, dtype=np.int32)
    assert cal.min() >= -1 and cal.max() < n
    return dict(kind=REGHOLIDAY, widths=[int(w) for w in widths], prior=(float(prior[0]), float(prior[1])),
                calendar=cal, coefficients=np.zeros(n) if coefficients is None else f64(coefficients))


def split(blocks):
    """(the state models, the regression holiday models) of a list"""
    return [b for b in blocks if b["kind"] != REGHOLIDAY], [b for b in blocks if b["kind"] == REGHOLIDAY]


def ncoef(model):
    return int(np.sum(model["widths"]))


def effects(models, coefs, t):
    """every model's Z_t: its coefficient active at t, or None"""
    return [float(c[m["calendar"][t]]) if m["calendar"][t] >= 0 else None for m, c in zip(models, coefs)]


def offset_series(y, models, coefs):
    """the series less the models' effects, model by model"""
    out = f64(y).copy()
    for t in range(len(out)):
        for e in effects(models, coefs, t):
            if e is not None:
                out[t] = out[t] - e
    return out


def forecast_offset(base, models, coefs, T):
    """forecast step i of the list without the models + the effects of time T + i, model by model"""
    out = f64(base).copy()
    for i in range(len(out)):
        for e in effects(models, coefs, T + i):
            if e is not None:
                out[i] = out[i] + e
    return out


def counts(models, observed, T):
    out = [np.zeros(ncoef(m)) for m in models]
    for m, n in zip(models, out):
        for t in range(T):
            if m["calendar"][t] >= 0 and observed[t]:
                n[m["calendar"][t]] += 1.0
    return out


def observe(models, coefs, y, xbeta, zalpha, observed, dtype=np.float64):
    """observe_state over the series: total[h][d] += (y_t - x_t'beta) - Z_t^all alpha_t + coefficient at every
    observed active step, where Z^all alpha holds every model's effect: in the device's arrangement
    ((y_c[t] - Z_t'alpha_t) - x_t'beta) + coefficient, with y_c the series less the effects"""
    T = len(y)
    yc = offset_series(y, models, coefs).astype(dtype) if dtype == np.float64 else None
    out = [np.zeros(ncoef(m), dtype=dtype) for m in models]
    for t in range(T):
        if not observed[t]:
            continue
        es = effects(models, coefs, t)
        if all(e is None for e in es):
            continue
        if yc is not None:
            base = (yc[t] - zalpha[t]) - xbeta[t]
        else:
            base = dtype(y[t])
            for e in es:
                if e is not None:
                    base = base - dtype(e)
            base = (base - dtype(zalpha[t])) - dtype(xbeta[t])
        for m, tot, e in zip(models, out, es):
            if e is not None:
                tot[m["calendar"][t]] += base + dtype(e)
    return out


def posterior(total, count, sigsq, mu, tau):
    """sample_posterior's moments of one coefficient"""
    precision = count / sigsq + 1.0 / (tau * tau)
    mean = total / sigsq + mu / (tau * tau)
    mean /= precision
    return mean, np.sqrt(1.0 / precision)


def draw(models, totals, cnts, sigsq, rnorm):
    """sample_posterior of every model: (model, coefficient) order, one rnorm(mean, sd) each"""
    out = []
    for m, tot, n in zip(models, totals, cnts):
        mu, tau = m["prior"]
        c = np.zeros(ncoef(m))
        for j in range(len(c)):
            mean, sd = posterior(tot[j], n[j], sigsq, mu, tau)
            c[j] = rnorm(mean, sd)
        out.append(c)
    return out


def dummies_posterior_mean(model, response, observed, T, sigsq):
    """the conjugate posterior mean of a regression of `response` on the model's dummies (one column per
    coefficient, a 1 where it is active and observed) under N(mu, tau^2) and residual variance sigsq, by a
    dense solve"""
    n = ncoef(model)
    rows = [t for t in range(T) if model["calendar"][t] >= 0 and observed[t]]
    D = np.zeros((len(rows), n))
    for i, t in enumerate(rows):
        D[i, model["calendar"][t]] = 1.0
    mu, tau = model["prior"]
    A = D.T @ D / sigsq + np.eye(n) / (tau * tau)
    b = D.T @ f64(response)[rows] / sigsq + mu / (tau * tau)
    return np.linalg.solve(A, b)


class AugmentedStructure(Structure):
    """the list with every regression holiday model as the reference has it: one more state component per
    model, the constant 1 (a0 = 1, P0 = 0, no error), observed through Z_t = the model's coefficient"""

    def __init__(self, blocks, models, coefs):
        const = [dict(kind=LEVEL, dim=1, nseasons=0, duration=1, t0=0, lags=0, a0=np.array([1.0]), P0=np.array([0.0]),
                      initial_sigma=np.array([0.0])) for _ in models]
        super().__init__(list(blocks) + const)
        self.nbase = len(blocks)
        self.models, self.coefs = models, coefs

    def Z(self, t):
        z = super().Z(t)
        for k, e in enumerate(effects(self.models, self.coefs, t)):
            z[self.first[self.nbase + k]] = 0.0 if e is None else e
        return z


class RegHolidayOracle:
    """one chain: `base` restates the state half of the list without the models (a StateOracle of
    ss_state_models_oracle); this class adds the models' coefficients, totals and stream"""

    def __init__(self, o, base, models, y, X, seed, chain):
        self.o, self.L, self.base, self.models = o, o.lib, base, models
        self.L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
        self.L.bo_rnorm.restype = C.c_double
        self.y, self.X = f64(y), f64(X)
        self.T = len(self.y)
        self.obs = base.obs
        self.rng = o.rng_philox(int(seed), int(chain), STREAM, 0)
        self.coefs = [f64(m["coefficients"]).copy() for m in models]
        self.totals = [np.zeros(ncoef(m)) for m in models]   # (before the first state draw: empty)
        self.counts = counts(models, self.obs, self.T)

    def _rnorm(self, mu, sd):
        return self.L.bo_rnorm(C.byref(self.rng), float(mu), float(sd))

    def draw_coefficients(self, sigsq):
        self.coefs = draw(self.models, self.totals, self.counts, sigsq, self._rnorm)
        return self.coefs

    def impute_state(self, beta, sigsq):
        """impute_state and its observe_state calls at the regression parameters given (beta: zero where
        excluded)"""
        xbeta = self.X @ f64(beta)
        yc = offset_series(self.y, self.models, self.coefs)
        st = self.base.impute_state(yc - xbeta, sigsq)
        zalpha = np.array([self.base.S.Z(t) @ st[t] for t in range(self.T)])
        self.totals = observe(self.models, self.coefs, self.y, xbeta, zalpha, self.obs)
        return st

    def round(self, beta, sigsq):
        """what follows the observation model's draw (beta, sigsq) in a round"""
        self.draw_coefficients(sigsq)
        self.base.draw_state_models()
        return self.impute_state(beta, sigsq)
