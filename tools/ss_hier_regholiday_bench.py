#!/usr/bin/env python3
"""Diagnostic timing of the hierarchical regression holiday state model
(ba_ss_add_hierarchical_regression_holiday, bsts AddHierarchicalRegressionHoliday): ms per round and device time
per kernel class of ba_ss_sweep on [level, 7 seasons] with one hierarchical model of 10 holidays of width 3 (6 %
of the days active), beside (a) the same list with the plain model of the same holidays and (b) the list without
a model, all on the general kernel (ba_ss_set_tuning(e, 0)) and the same data.  The class "reg_holiday_kernels"
holds rhh_draw_kernel, rh_draw_kernel and rh_observe_kernel together.  The list without a model runs on the
parent commit's library too (an engine without the new call times it alone).  Not a bench line.
usage: ss_hier_regholiday_bench.py [T p chains [timed rounds [burn-in rounds]]]
       (default: T = 2000, p = 100, 1024 chains, 20 rounds after 10)"""
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
nsw = int(sys.argv[4]) if len(sys.argv) > 4 else 20
burn = int(sys.argv[5]) if len(sys.argv) > 5 else 10
rng = np.random.default_rng(8675309)
X = rng.standard_normal((T, p))
beta = np.zeros(p)
beta[:5] = rng.choice([-2.0, -1.0, 1.0, 1.5], 5)
# ten holidays, each a window of three days with its own pattern that comes back every 500 steps: 30 of 500
# days, 6 %, are active
WIDTH, NHOL, PERIOD = 3, 10, 500
cal = np.full(T, -1, np.int32)
effect = np.zeros(T)
for h in range(NHOL):
    shape = rng.standard_normal(WIDTH)
    for t0 in range(20 + 33 * h, T - WIDTH, PERIOD):
        cal[t0:t0 + WIDTH] = WIDTH * h + np.arange(WIDTH)
        effect[t0:t0 + WIDTH] += shape
week = rng.standard_normal(7)
y = (np.cumsum(0.02 + 0.05 * rng.standard_normal(T)) + (week - week.mean())[np.arange(T) % 7] + effect + X @ beta +
     0.3 * rng.standard_normal(T))
base = general_spec(y, [("level",), ("seasonal", 7, 1)])
sdy = float(np.std(y, ddof=1))
plain = dict(kind="regression_holiday", widths=[WIDTH] * NHOL, prior=(0.0, sdy), calendar=cal)
hier = dict(kind="hierarchical_regression_holiday", nholidays=NHOL, width=WIDTH,
            mean_prior=(np.zeros(WIDTH), sdy * sdy * np.eye(WIDTH)), variance_prior=(sdy * sdy * np.eye(WIDTH), WIDTH + 1.0),
            calendar=cal)
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
    eng.ss_sweep(burn)   # burn-in: the models grow to their size
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


out = dict(T=T, p=p, chains=chains, rounds=nsw, burn_in=burn, active_fraction=float((cal >= 0).mean()))
out["without"] = timed(base)
if hasattr(boom_amd.Engine, "ss_add_hierarchical_regression_holiday"):   # (the parent commit: the list without a model alone)
    out["plain"] = timed(base + [plain])
    out["hierarchical"] = timed(base + [hier])
    for key in ("plain", "hierarchical"):
        out[key + "_round_ratio"] = out[key]["ms_per_round"] / out["without"]["ms_per_round"]
        out[key + "_own_kernels_ms"] = out[key]["kernel_ms_per_round"].get(OWN, 0.0)
    out["state_kernel_ms"] = [out[k]["kernel_ms_per_round"].get(STATE, 0.0) for k in ("hierarchical", "plain", "without")]
print(json.dumps(out))
