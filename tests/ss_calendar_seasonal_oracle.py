"""A restatement of the state half of StateSpacePosteriorSampler::draw() for a list of state models
that holds calendar seasonals (ba_ss_add_state_model kind 11; bsts AddMonthlyAnnualCycle is the one
of 12 seasons that start on the first day of a month), on the device's substreams, one chain, in
Python over the oracle's primitives.  The recursion is tests/ss_state_models_oracle.py's, where the
seasonal of either kind is the one class Seasonal with two answers to "does time t start a new season":
the duration rule (kind 3) and the block's flags (kind 11).  This file states the model, builds its
block and its calendars and passes that file's names on.

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
import datetime

import numpy as np

from ss_state_models_oracle import (CALENDAR_SEASONAL, Structure, forecast, impute_state,  # noqa: F401
                                    simulate_forward, state_model_suf)
from ss_state_models_oracle import StateOracle as CalendarOracle  # noqa: F401


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
