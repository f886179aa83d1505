#!/usr/bin/env python3
"""Diagnostic timing of the dynamic regression state model (ba_ss_add_dynamic_regression, bsts
AddDynamicRegression): ms per round and device time per kernel class of ba_ss_sweep on [level, 7 seasons,
dynamic regression d = 4] -- the DR instances of the general kernel -- beside the same list with four more
local levels in the block's place: the same state dimension, the same state-error rows and the same
variance slots, on the existing scalar instance of the same kernel (ba_ss_set_tuning(e, 0)), on the same
data.  Not a bench line.
usage: ss_dynreg_bench.py [T p chains [timed rounds]]   (default: T = 2000, p = 100, 1024 chains, 10 rounds)"""
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
from ss_dynreg_oracle import dynreg_block  # noqa: E402

T, p, chains = (int(v) for v in (sys.argv[1:4] or (2000, 100, 1024)))
nsw = int(sys.argv[4]) if len(sys.argv) > 4 else 10
D = 4
rng = np.random.default_rng(8675309)
X = rng.standard_normal((T, p))
beta = np.zeros(p)
beta[:5] = rng.choice([-2.0, -1.0, 1.0, 1.5], 5)
# four predictors whose coefficients wander
Xd = rng.standard_normal((T, D))
coef = np.array([1.0, -0.5, 0.8, 0.3]) + np.cumsum(0.03 * rng.standard_normal((T, D)), axis=0)
week = rng.standard_normal(7)
y = (np.cumsum(0.02 + 0.05 * rng.standard_normal(T)) + (week - week.mean())[np.arange(T) % 7] + np.sum(Xd * coef, 1) +
     X @ beta + 0.3 * rng.standard_normal(T))
sdy = float(np.std(y, ddof=1))
base = general_spec(y, [("level",), ("seasonal", 7, 1)])
dynamic = base + [dynreg_block(Xd, sdy, np.full(D, 0.05))]
levels = base + general_spec(y, [("level",)] * D)
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


dyn = timed(dynamic)
lev = timed(levels)
kd, kl = dyn["kernel_ms_per_round"].get(STATE, 0.0), lev["kernel_ms_per_round"].get(STATE, 0.0)
print(json.dumps(dict(T=T, p=p, chains=chains, rounds=nsw, dynamic=dyn, levels=lev,
                      round_ms=[dyn["ms_per_round"], lev["ms_per_round"]], state_kernel_ms=[kd, kl],
                      state_kernel_ratio=(kd / kl if kl else None))))
