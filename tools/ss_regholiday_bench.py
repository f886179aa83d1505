#!/usr/bin/env python3
"""Diagnostic timing of the regression holiday state model (ba_ss_add_regression_holiday, bsts
AddRegressionHoliday): ms per round and device time per kernel class of ba_ss_sweep on [level, 7 seasons]
with one model of 10 holidays of width 3 (about 5 % of the days active) beside the same list without it, both
on the general kernel (ba_ss_set_tuning(e, 0)) and the same data.  The list without the model, run on the
parent commit too, times the plain instances' strided read of the series.  Not a bench line.
usage: ss_regholiday_bench.py [T p chains [timed rounds]]   (default: T = 2000, p = 100, 1024 chains, 10 rounds)"""
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
nsw = int(sys.argv[4]) if len(sys.argv) > 4 else 10
rng = np.random.default_rng(8675309)
X = rng.standard_normal((T, p))
beta = np.zeros(p)
beta[:5] = rng.choice([-2.0, -1.0, 1.0, 1.5], 5)
# ten holidays, each a window of three days with its own pattern that comes back every 548 steps: 30 of 548
# days, about 5 %, are active
WIDTH, NHOL = 3, 10
starts = tuple(20 + 33 * h for h in range(NHOL))
cal = np.full(T, -1, np.int32)
effect = np.zeros(T)
for h, s in enumerate(starts):
    shape = rng.standard_normal(WIDTH)
    for t0 in range(s, T - WIDTH, 548):
        cal[t0:t0 + WIDTH] = WIDTH * h + np.arange(WIDTH)
        effect[t0:t0 + WIDTH] += shape
week = rng.standard_normal(7)
y = (np.cumsum(0.02 + 0.05 * rng.standard_normal(T)) + (week - week.mean())[np.arange(T) % 7] + effect + X @ beta +
     0.3 * rng.standard_normal(T))
base = general_spec(y, [("level",), ("seasonal", 7, 1)])
model = dict(kind="regression_holiday", widths=[WIDTH] * NHOL, prior=(0.0, float(np.std(y, ddof=1))), calendar=cal)
g0 = np.zeros(p, np.uint8)
g0[0] = 1
prior, _, sig_up = bsts_priors(X, y, 5)
STATE, OWN = "ssm_simsmooth_kernel", "reg_holiday_kernels"


def timed(state_models):
    eng = boom_amd.Engine(chains, seed=4)
    eng.ss_set_data(y, X, None)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"], sigma_upper_limit=sig_up)
    eng.ss_set_state_models(state_models)
    eng.ss_set_tuning(kernel=0)
    eng.set_state(g0)
    eng.ss_sweep(max(2, nsw // 2))   # burn-in: the models grow to their size
    t0 = time.perf_counter()
    eng.ss_sweep(nsw)
    dt = time.perf_counter() - t0
    eng.set_kernel_timing(True)
    eng.kernel_times(reset=True)
    eng.ss_sweep(nsw)
    kt = eng.kernel_times(reset=True)
    eng.set_kernel_timing(False)
    return dict(ms_per_round=dt / nsw * 1e3, kernel_ms_per_round={k: round(v[0] / nsw, 4) for k, v in kt.items()},
                launches_per_round={k: v[1] / nsw for k, v in kt.items()},
                kbar=float(eng.get_states()[0].sum(1).mean()))


out = dict(T=T, p=p, chains=chains, rounds=nsw, active_fraction=float((cal >= 0).mean()))
out["without"] = timed(base)
if hasattr(boom_amd.Engine, "ss_add_regression_holiday"):   # (the parent commit: the list without the model alone)
    out["with"] = timed(base + [model])
    a, b = out["with"], out["without"]
    out["round_ratio"] = a["ms_per_round"] / b["ms_per_round"]
    out["state_kernel_ms"] = [a["kernel_ms_per_round"].get(STATE, 0.0), b["kernel_ms_per_round"].get(STATE, 0.0)]
    out["own_kernels_ms"] = a["kernel_ms_per_round"].get(OWN, 0.0)
print(json.dumps(out))
