#!/usr/bin/env python3
"""Diagnostic timing of ba_ss_prediction_errors: device time of the filter kernel per call of all
chains, beside the same list's state-draw kernel time per round from the timing classes of the same
run -- the state draw does the filter's work plus a simulation and a backward pass, and it is code
the filter does not share, so it is the yardstick.  Three lists: the local level (the path of
ba_ss_set_local_level, its rounds as separate launches so that the state draw has a class of its
own), trend + 12 seasons (m = 13) and bsts's daily model, trend + day of week + 52 weeks of 7 days
(m = 59).  Not a bench line.
usage: ss_prediction_errors_bench.py [T p chains [timed rounds]]   (default: T = 2000, p = 100, 1024
chains, 5 rounds)"""
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

T, p, chains = (int(v) for v in (sys.argv[1:4] or (2000, 100, 1024)))
nsw = int(sys.argv[4]) if len(sys.argv) > 4 else 5
rng = np.random.default_rng(8675309)
X = rng.standard_normal((T, p))
beta = np.zeros(p)
beta[:5] = rng.choice([-2.0, -1.0, 1.0, 1.5], 5)
level = np.cumsum(0.1 * rng.standard_normal(T))
y = level + np.tile(rng.standard_normal(12), T // 12 + 1)[:T] + np.tile(rng.standard_normal(7), T // 7 + 1)[:T] \
    + X @ beta + 0.5 * rng.standard_normal(T)
g0 = np.zeros(p, np.uint8)
g0[0] = 1
prior, ss, sig_up = bsts_priors(X, y, 5)
FILTER = "ss_filter_kernel"
LISTS = [("local level (ba_ss_set_local_level)", None, "kalman_simsmooth_kernel"),
         ("trend + 12 seasons, m = 13", [("trend",), ("seasonal", 12, 1)], "ssm_simsmooth_kernel"),
         ("trend + 7 days + 52 weeks of 7 days, m = 59", [("trend",), ("seasonal", 7, 1), ("seasonal", 52, 7)],
          "ssm_simsmooth_kernel")]


def timed(desc, state_class):
    eng = boom_amd.Engine(chains, seed=4)
    eng.ss_set_data(y, X, None)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"], sigma_upper_limit=sig_up)
    if desc is None:
        eng.ss_set_local_level(ss["level_df"], ss["level_sigma_guess"], ss["level_sigma_upper_limit"],
                               ss["initial_state_mean"], ss["initial_state_variance"], ss["initial_level_sigma"])
        eng.ss_set_tuning(kernel=4)
    else:
        eng.ss_set_state_models(general_spec(y, desc))
    eng.set_state(g0)
    eng.ss_sweep(3)   # burn-in: the models grow to their size
    eng.ss_prediction_errors()   # (buffers)
    eng.set_kernel_timing(True)
    eng.kernel_times(reset=True)
    eng.ss_sweep(nsw)
    kt = eng.kernel_times(reset=True)
    t0 = time.perf_counter()
    for _ in range(nsw):
        eng.ss_prediction_errors(log_likelihood=True)
    wall = (time.perf_counter() - t0) / nsw * 1e3
    kf = eng.kernel_times(reset=True)
    eng.set_kernel_timing(False)
    f, s = kf[FILTER][0] / kf[FILTER][1], kt[state_class][0] / nsw
    return dict(filter_ms_per_call=round(f, 4), call_wall_ms=round(wall, 4), state_draw_ms_per_round=round(s, 4),
                filter_over_state_draw=round(f / s, 4), state_draw_class=state_class,
                kbar=float(eng.get_states()[0].sum(1).mean()))


print(json.dumps(dict(T=T, p=p, chains=chains, rounds=nsw, lists={name: timed(desc, cls) for name, desc, cls in LISTS})))
