#!/usr/bin/env python3
"""Diagnostic timing of the random-walk holiday state model (state model kind 10, bsts
AddRandomWalkHoliday): ms per round and device time per kernel class of ba_ss_sweep on [level, 7
seasons, three holidays of width 3] -- the holiday instances of the general kernel -- beside the same
list with a 4-season seasonal block in place of every holiday: the same state dimension and the same
number of state-error rows, on the existing scalar instance of the same kernel (ba_ss_set_tuning(e, 0)),
on the same data.  Not a bench line.
usage: ss_holiday_bench.py [T p chains [timed rounds]]   (default: T = 2000, p = 100, 1024 chains, 10 rounds)"""
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
from ss_holiday_oracle import holiday_block  # noqa: E402

T, p, chains = (int(v) for v in (sys.argv[1:4] or (2000, 100, 1024)))
nsw = int(sys.argv[4]) if len(sys.argv) > 4 else 10
rng = np.random.default_rng(8675309)
X = rng.standard_normal((T, p))
beta = np.zeros(p)
beta[:5] = rng.choice([-2.0, -1.0, 1.0, 1.5], 5)
# three holidays a "year" of 365 steps, each a window of three days with its own effect
starts = (40, 150, 300)
cal = [np.full(T, -1, np.int32) for _ in starts]
effect = np.zeros(T)
for h, s in enumerate(starts):
    shape = rng.standard_normal(3)
    for t0 in range(s, T - 3, 365):
        cal[h][t0:t0 + 3] = (0, 1, 2)
        effect[t0:t0 + 3] += shape
week = rng.standard_normal(7)
y = (np.cumsum(0.02 + 0.05 * rng.standard_normal(T)) + (week - week.mean())[np.arange(T) % 7] + effect + X @ beta +
     0.3 * rng.standard_normal(T))
sdy = float(np.std(y, ddof=1))
base = general_spec(y, [("level",), ("seasonal", 7, 1)])
holidays = base + [holiday_block(3, c, sdy, 0.5) for c in cal]
seasonal = base + general_spec(y, [("seasonal", 4, 1)] * 3)
g0 = np.zeros(p, np.uint8)
g0[0] = 1
prior, _, sig_up = bsts_priors(X, y, 5)
STATE = "ssm_simsmooth_kernel"


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


hol = timed(holidays)
sea = timed(seasonal)
kh, ks = hol["kernel_ms_per_round"].get(STATE, 0.0), sea["kernel_ms_per_round"].get(STATE, 0.0)
print(json.dumps(dict(T=T, p=p, chains=chains, rounds=nsw, holidays=hol, seasonal=sea,
                      round_ms=[hol["ms_per_round"], sea["ms_per_round"]], state_kernel_ms=[kh, ks],
                      state_kernel_ratio=(kh / ks if ks else None))))
