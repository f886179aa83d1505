"""A restatement of the state half of StateSpacePosteriorSampler::draw() for a list of state models
that holds RandomWalkHolidayStateModel blocks (StateModels/RandomWalkHolidayStateModel.cpp, bsts
AddRandomWalkHoliday; ba_ss_add_state_model kind 10), on the device's substreams, one chain, in
Python over the oracle's primitives: the parity yardstick of the general structural kernel's
holiday instances.  The recursion -- the filter, the smoother, the simulation, the statistics, the
forecast, each written for an observation row Z_t and a state-error variance RQR_t that change from step
to step -- is tests/ss_state_models_oracle.py's, where the holiday is the class Holiday; this file states
the model, builds its block and passes that file's names on (tests/ss_student_oracle.py fixes Z as one
vector; tests/test_ss_holiday_cpu.py compares the two where they must agree).

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
import numpy as np

from ss_state_models_oracle import (HOLIDAY, LEVEL, LOG_2PI, SEASONAL, TREND, TRIG, Structure,  # noqa: F401
                                    block_stream_ids, dense_posterior, disturbance_smooth, f64, forecast, gains,
                                    impute_state, innovations, kalman, log_likelihood, new_season,
                                    reference_and_gate, simulate_forward, state_model_suf)
from ss_state_models_oracle import StateOracle as HolidayOracle  # noqa: F401


def holiday_block(width, calendar, sdy, initial_sigma=0.6, a0=None):
    """a kind 10 block dict with bsts-style defaults (as cases.general_spec's): sd prior guess
    0.01 sd(y), df 0.01, upper limit sd(y); initial state N(a0 or 0, sd(y)^2)"""
    return dict(kind=HOLIDAY, width=int(width), dim=int(width), calendar=np.asarray(calendar, dtype=np.int32),
                nseasons=0, duration=1, t0=0, lags=0, df=np.array([0.01]), sigma_guess=np.array([0.01 * sdy]),
                sigma_upper_limit=np.array([sdy]), initial_sigma=np.array([float(initial_sigma)]),
                initial_phi=np.zeros(0), a0=np.zeros(width) if a0 is None else f64(a0),
                P0=np.full(width, sdy * sdy))
