#!/usr/bin/env python3
"""Diagnostic timing of ba_ss_holdout_prediction_errors: device time of the filter kernel's holdout instance
per call of all chains, beside ba_ss_prediction_errors of the same engine in the same run, both PER STEP (the
holdout call filters `horizon` rows, the in-sample call the series' T).  The two instances run the same step code,
so the per-step costs should be equal; the ratio printed is holdout / in-sample.  Both calls book their kernel
under the timing class ss_filter_kernel, so each is timed in a window of its own.  Two lists: trend + 12 seasons
(m = 13) and bsts's daily model, trend + day of week + 52 weeks of 7 days (m = 59).  Every figure is the mean of
`rounds` calls; the run is repeated `repeats` times on the same engine to show the run-to-run spread.  Not a
bench line.
usage: ss_holdout_errors_bench.py [T p chains horizon [rounds [repeats]]]   (default: T = 2000, p = 100, 1024
chains, horizon 200, 5 rounds, 3 repeats)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import boom_amd  # noqa: E402
from cases import bsts_priors, general_spec  # noqa: E402

T, p, chains, horizon = (int(v) for v in (sys.argv[1:5] or (2000, 100, 1024, 200)))
nsw = int(sys.argv[5]) if len(sys.argv) > 5 else 5
repeats = int(sys.argv[6]) if len(sys.argv) > 6 else 3
rng = np.random.default_rng(8675309)
N = T + horizon
X = rng.standard_normal((N, p))
beta = np.zeros(p)
beta[:5] = rng.choice([-2.0, -1.0, 1.0, 1.5], 5)
level = np.cumsum(0.1 * rng.standard_normal(N))
y = level + np.tile(rng.standard_normal(12), N // 12 + 1)[:N] + np.tile(rng.standard_normal(7), N // 7 + 1)[:N] \
    + X @ beta + 0.5 * rng.standard_normal(N)
g0 = np.zeros(p, np.uint8)
g0[0] = 1
prior, ss, sig_up = bsts_priors(X[:T], y[:T], 5)
FILTER = "ss_filter_kernel"
LISTS = [("trend + 12 seasons, m = 13", [("trend",), ("seasonal", 12, 1)]),
         ("trend + 7 days + 52 weeks of 7 days, m = 59", [("trend",), ("seasonal", 7, 1), ("seasonal", 52, 7)])]


def window(eng, call):
    """(device ms per call, wall ms per call) of nsw calls"""
    eng.kernel_times(reset=True)
    t0 = time.perf_counter()
    for _ in range(nsw):
        call()
    wall = (time.perf_counter() - t0) / nsw * 1e3
    kf = eng.kernel_times(reset=True)
    assert kf[FILTER][1] == nsw, kf[FILTER]
    return kf[FILTER][0] / kf[FILTER][1], wall


def timed(desc):
    eng = boom_amd.Engine(chains, seed=4)
    eng.ss_set_data(y[:T], X[:T], None)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"], sigma_upper_limit=sig_up)
    eng.ss_set_state_models(general_spec(y[:T], desc))
    eng.set_state(g0)
    eng.ss_sweep(3)   # burn-in: the models grow to their size
    newX, newY = np.ascontiguousarray(X[T:]), np.ascontiguousarray(y[T:])
    eng.ss_prediction_errors()   # (buffers)
    eng.ss_holdout_prediction_errors(newX, newY)
    eng.set_kernel_timing(True)
    runs = []
    for _ in range(repeats):
        h_ms, h_wall = window(eng, lambda: eng.ss_holdout_prediction_errors(newX, newY, variances=True))
        f_ms, f_wall = window(eng, lambda: eng.ss_prediction_errors(variances=True))
        hs, fs = h_ms / horizon * 1e3, f_ms / T * 1e3
        runs.append(dict(holdout_ms_per_call=round(h_ms, 4), holdout_call_wall_ms=round(h_wall, 4),
                         in_sample_ms_per_call=round(f_ms, 4), in_sample_call_wall_ms=round(f_wall, 4),
                         holdout_us_per_step=round(hs, 4), in_sample_us_per_step=round(fs, 4),
                         holdout_over_in_sample_per_step=round(hs / fs, 4)))
    eng.set_kernel_timing(False)
    return dict(runs=runs, kbar=float(eng.get_states()[0].sum(1).mean()))


print(json.dumps(dict(T=T, p=p, chains=chains, horizon=horizon, rounds=nsw, repeats=repeats,
                      lists={name: timed(desc) for name, desc in LISTS})))
