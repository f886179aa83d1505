"""A restatement of the state half of StateSpacePosteriorSampler::draw() for a list of state models
that holds calendar seasonals (ba_ss_add_state_model kind 11; bsts AddMonthlyAnnualCycle is the one
of 12 seasons that start on the first day of a month), on the device's substreams, one chain, in
Python over the oracle's primitives.  It stands on tests/ss_holiday_oracle.py: the filter, the
smoother, the dense posterior and the long-double gate there are written against a Structure whose
transition and state-error variance change from step to step, and only ask the Structure which blocks
move at a step.  What is restated here is everything that asks "does time t start a new season" by
itself: the Structure's answer, simulate_forward, the sufficient statistics and the forecast.

The calendar seasonal (nseasons - 1 components, flags s(t) in {0, 1} for every time t):
  Z = e_0;
  the step t -> t + 1 where s(t + 1) = 1: the seasonal transition (first row -1, ones below the
  diagonal), RQR = sigma^2 e_0 e_0'; every other step: the identity, no error;
  observe_state at the t >= 1 with s(t) = 1: the GaussianSuf of now[0] + sum(then);
  initial state, prior, sigma upper limit: the seasonal's.
  s(0) is never read.  A step whose next entry lies past the calendar's end does not move (only the
  last step of a series whose calendar has exactly T entries can ask: its result is not used).

CONVENTIONS (the seasonal's, kind 3, exactly): one stream-2 normal per step into a new season -- none
elsewhere, none at all when sigma = 0 (rnorm does not draw at sd 0) --; the variance draw on sampler
id 7 + 16 per earlier seasonal block of either kind.  A calendar with s(t) = (t % d == ph) is
therefore the kind 3 block of duration d and time_of_first_observation ph, draw for draw.
"""
import ctypes as C
import datetime

import numpy as np

import ss_holiday_oracle as sho
from ss_holiday_oracle import HOLIDAY, LEVEL, SEASONAL, TREND, TRIG, f64

CALENDAR_SEASONAL = 11


def calendar_block(nseasons, calendar, sdy, initial_sigma=0.7):
    """a kind 11 block dict with bsts-style defaults (as cases.general_spec's seasonal): sd prior guess
    0.01 sd(y), df 0.01, upper limit sd(y); initial state N(0, sd(y)^2)"""
    n = int(nseasons) - 1
    return dict(kind=CALENDAR_SEASONAL, nseasons=int(nseasons), dim=n,
                calendar=None if calendar is None else np.asarray(calendar, dtype=np.uint8),
                duration=1, t0=0, lags=0, df=np.array([0.01]), sigma_guess=np.array([0.01 * sdy]),
                sigma_upper_limit=np.array([sdy]), initial_sigma=np.array([float(initial_sigma)]),
                initial_phi=np.zeros(0), a0=np.zeros(n), P0=np.full(n, sdy * sdy))


def regular_calendar(count, duration, phase):
    t = np.arange(count)
    return (t % duration == phase).astype(np.uint8)


def starts_calendar(count, starts):
    cal = np.zeros(count, np.uint8)
    cal[[t for t in starts if t < count]] = 1
    return cal


def month_starts(first_date, count):
    """Python's own calendar: flags of day-of-month == 1 for `count` days from first_date = (y, m, d)"""
    d0 = datetime.date(*first_date)
    return np.array([(d0 + datetime.timedelta(days=int(t))).day == 1 for t in range(count)], np.uint8)


def starts(b, t):
    """does time t start a new season of block b (a seasonal of either kind)?"""
    if "season_calendar" in b:
        cal = b["season_calendar"]
        return bool(cal[t]) if t < len(cal) else False
    return sho.new_season(b, t)


class Structure(sho.Structure):
    """ss_holiday_oracle's Structure with the calendar seasonals seen as seasonal blocks that carry
    their flags (season_calendar): Z, Tmat and rqr there ask moves() alone"""

    def __init__(self, blocks):
        view = []
        for b in blocks:
            if b["kind"] == CALENDAR_SEASONAL:
                b = dict(b, kind=SEASONAL, season_calendar=np.asarray(b["calendar"], np.uint8))
            view.append(b)
        super().__init__(view)

    def moves(self, b, t):
        if b["kind"] == SEASONAL:
            return starts(b, t + 1)
        return super().moves(b, t)


def simulate_forward(S, sigsq, H, rnorm):
    """simulate_forward in the device's order: t = 0 the initial state of every model, then the
    observation; t >= 1 the state errors model by model, then the observation"""
    T, m = len(H), S.m
    st, ys = np.zeros((T, m)), np.zeros(T)
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
                sd = np.sqrt(s[0])
                if b["kind"] == SEASONAL:
                    if starts(b, t):
                        eta[f] = rnorm(0.0, sd)
                elif b["kind"] == HOLIDAY:
                    z = rnorm(0.0, 1.0)   # (one per step, active or not: the holiday's convention)
                    k = S.position(b, t)
                    if k >= 0:
                        eta[f + k] = sd * z
                elif b["kind"] == LEVEL:
                    eta[f] = rnorm(0.0, sd)
                elif b["kind"] == TREND:
                    z0, z1 = rnorm(0.0, 1.0), rnorm(0.0, 1.0)
                    eta[f], eta[f + 1] = sd * z0 + 0.0, np.sqrt(s[1]) * z1 + 0.0
                else:
                    assert b["kind"] == TRIG
                    for i in range(b["dim"]):
                        eta[f + i] = rnorm(0.0, sd)
            st[t] = S.Tmat(t - 1) @ st[t - 1] + eta
        ys[t] = rnorm(S.Z(t) @ st[t], np.sqrt(H[t]))
    return st, ys


def impute_state(S, sigsq, ystar, observed, H, rnorm, FK=None):
    """Base::impute_state: the simulated path corrected by the difference of the two smoothed means
    (FK: F_t and K_t computed already -- they do not depend on the draw)"""
    T = len(ystar)
    F, K = FK if FK is not None else sho.gains(S, sigsq, observed, H)
    st, ys = simulate_forward(S, sigsq, H, rnorm)
    r, r0 = sho.disturbance_smooth(S, sho.innovations(S, K, ystar, observed), F, K)
    rs, r0s = sho.disturbance_smooth(S, sho.innovations(S, K, ys, observed), F, K)
    mean_obs, mean_sim = S.a0 + S.P0 * r0, S.a0 + S.P0 * r0s
    out = st.copy()
    out[0] += mean_obs - mean_sim
    for t in range(1, T):
        Tm, q = S.Tmat(t - 1), S.rqr(t - 1, sigsq)
        mean_obs = Tm @ mean_obs + q * r[t - 1]
        mean_sim = Tm @ mean_sim + q * rs[t - 1]
        out[t] += mean_obs - mean_sim
    return out


def state_model_suf(S, st):
    """observe_state of every model over the draw: the seasonals of either kind here, the others as
    ss_holiday_oracle has them"""
    n, ss = sho.state_model_suf(S, st)
    for k, (b, f) in enumerate(zip(S.blocks, S.first)):
        if b["kind"] != SEASONAL:
            continue
        n[k][:], ss[k][:] = 0.0, 0.0
        for t in range(1, st.shape[0]):
            if starts(b, t):
                delta = st[t, f] + np.sum(st[t - 1, f:f + b["dim"]])
                n[k][0] += 1
                ss[k][0] += delta * delta
    return n, ss


def forecast(S, T, last_state, sigsq, sigsq_obs, xbeta, rnorm):
    """simulate_multiplex_forecast from the state of time T - 1: step i advances with the transition and
    state errors of time T - 2 + i -- a seasonal of either kind asks new_season(T - 1 + i) -- and
    observes with Z of time T + i"""
    state = np.array(last_state, dtype=float)
    out = np.zeros(len(xbeta))
    for i in range(len(xbeta)):
        tm = T - 2 + i
        eta = np.zeros(S.m)
        for b, f, s in zip(S.blocks, S.first, sigsq):
            sd = np.sqrt(s[0])
            if b["kind"] == SEASONAL:
                if starts(b, tm + 1):
                    eta[f] = rnorm(0.0, sd)
            elif b["kind"] == HOLIDAY:
                k = S.position(b, tm + 1)
                if k >= 0:
                    eta[f + k] = rnorm(0.0, sd)
            elif b["kind"] == LEVEL:
                eta[f] = rnorm(0.0, sd)
            elif b["kind"] == TREND:
                z0, z1 = rnorm(0.0, 1.0), rnorm(0.0, 1.0)
                eta[f], eta[f + 1] = sd * z0 + 0.0, np.sqrt(s[1]) * z1 + 0.0
            else:
                for q in range(b["dim"]):
                    eta[f + q] = rnorm(0.0, sd)
        state = S.Tmat(tm) @ state + eta
        out[i] = rnorm(S.Z(tm + 2) @ state, np.sqrt(sigsq_obs)) + xbeta[i]
    return out


class CalendarOracle(sho.HolidayOracle):
    """ss_holiday_oracle.HolidayOracle (the variance draws, their decision margins, the prediction
    errors) over this module's Structure and its own impute_state, statistics and forecast"""

    def __init__(self, o, T, observed, blocks, seed, chain):
        S = Structure(blocks)
        super().__init__(o, T, observed, S.blocks, seed, chain)   # (sampler ids: kinds 3 and 11 are one family)
        self.S = S

    def impute_state(self, ystar, sigsq_obs):
        H = np.full(self.T, float(sigsq_obs))
        self.state = impute_state(self.S, self.var, f64(ystar), self.obs, H, self._rnorm)
        self.suf_n, self.suf_ss = state_model_suf(self.S, self.state)
        return self.state

    def forecast(self, last_state, sigsq_obs, xbeta):
        return forecast(self.S, self.T, last_state, self.var, sigsq_obs, xbeta, self._rnorm_forecast)

    def positions(self):
        """where the chain's state, forecast and variance streams stand (the generators' raw bytes)"""
        return (bytes(self.state_rng), bytes(self.forecast_rng),
                [[bytes(r) for r in row] for row in self.var_rng])
