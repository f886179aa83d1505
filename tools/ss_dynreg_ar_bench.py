#!/usr/bin/env python3
"""Diagnostic timing of the AR dynamic regression (ba_ss_add_dynamic_regression_ar, bsts AddDynamicRegression
with DynamicRegressionArOptions): ms per round and device time per kernel class of ba_ss_sweep on [level,
7 seasons, AR dynamic regression xdim = 3, lags = 2] -- the DR instances of the general kernel -- beside the
stand-in, the same list with three plain autoregressions of 2 lags (kind 4) in the model's place: the same
state dimension, autoregression slots, variance slots and normals, on the PLAIN instance of the same kernel
(ba_ss_set_tuning(e, 0)), on the same data.  Not a bench line.
usage: ss_dynreg_ar_bench.py [T p chains [timed rounds [repeats]]] [--stand-in-only]
       (default: T = 2000, p = 100, 1024 chains, 10 rounds, 3 repeats; --stand-in-only: a library without the
       model, for the comparison with an earlier commit)"""
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

args = [a for a in sys.argv[1:] if not a.startswith("--")]
stand_in_only = "--stand-in-only" in sys.argv
T, p, chains = (int(v) for v in (args[:3] or (2000, 100, 1024)))
nsw = int(args[3]) if len(args) > 3 else 10
repeats = int(args[4]) if len(args) > 4 else 3
D, LAGS = 3, 2
PHI = np.array([[0.5, 0.2], [0.3, -0.2], [0.6, 0.1]])
rng = np.random.default_rng(8675309)
X = rng.standard_normal((T, p))
beta = np.zeros(p)
beta[:5] = rng.choice([-2.0, -1.0, 1.0, 1.5], 5)
# three predictors whose coefficients follow stationary autoregressions of two lags
Xd = rng.standard_normal((T, D))
coef = np.zeros((T, D))
shock = 0.05 * rng.standard_normal((T, D))
for t in range(2, T):
    coef[t] = PHI[:, 0] * coef[t - 1] + PHI[:, 1] * coef[t - 2] + shock[t]
week = rng.standard_normal(7)
y = (np.cumsum(0.02 + 0.05 * rng.standard_normal(T)) + (week - week.mean())[np.arange(T) % 7] + np.sum(Xd * coef, 1) +
     X @ beta + 0.3 * rng.standard_normal(T))
sdy = float(np.std(y, ddof=1))
base = general_spec(y, [("level",), ("seasonal", 7, 1)])
stand_in = base + general_spec(y, [("ar", LAGS, PHI[i]) for i in range(D)])
for b in stand_in[2:]:
    b["initial_sigma"], b["a0"], b["P0"] = np.array([0.05]), np.zeros(LAGS), np.ones(LAGS)
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
    rounds = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        eng.ss_sweep(nsw)
        rounds.append((time.perf_counter() - t0) / nsw * 1e3)
    eng.set_kernel_timing(True)
    eng.kernel_times(reset=True)
    eng.ss_sweep(nsw)
    kt = eng.kernel_times(reset=True)
    eng.set_kernel_timing(False)
    return dict(ms_per_round=float(np.median(rounds)), ms_per_round_repeats=[round(r, 4) for r in rounds],
                kernel_ms_per_round={k: round(v[0] / nsw, 4) for k, v in kt.items()},
                launches_per_round={k: v[1] / nsw for k, v in kt.items()},
                kbar=float(eng.get_states()[0].sum(1).mean()))


out = dict(T=T, p=p, chains=chains, rounds=nsw, repeats=repeats)
out["stand_in"] = timed(stand_in)
ks = out["stand_in"]["kernel_ms_per_round"].get(STATE, 0.0)
if not stand_in_only:
    from ss_dynreg_ar_oracle import dynreg_ar_blocks, engine_blocks  # noqa: E402
    model = base + engine_blocks(dynreg_ar_blocks(Xd, LAGS, sdy, np.full(D, 0.05), PHI))
    out["model"] = timed(model)
    km = out["model"]["kernel_ms_per_round"].get(STATE, 0.0)
    out.update(round_ms=[out["model"]["ms_per_round"], out["stand_in"]["ms_per_round"]], state_kernel_ms=[km, ks],
               round_ratio=out["model"]["ms_per_round"] / out["stand_in"]["ms_per_round"],
               state_kernel_ratio=(km / ks if ks else None))
print(json.dumps(out))
