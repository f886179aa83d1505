#!/usr/bin/env python3
"""Diagnostic timing of the Student local linear trend state model (state model kind 8): ms per round
and device time per kernel class of ba_ss_sweep on [Student trend + seasonal], beside the same list
with a plain local linear trend (kind 2) through the general kernel (ba_ss_set_tuning(e, 0)) on the
same data -- the number the QT instances' state draw is to be read against.  Not a bench line.
usage: ss_student_trend_bench.py [T p chains [timed rounds [nseasons]]]   (default: T = 2000, p = 100,
1024 chains, 10 rounds, 12 seasons)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import boom_amd  # noqa: E402
from cases import bsts_priors  # noqa: E402
from student_trend_cases import as_plain_trend, student_trend_spec  # noqa: E402

T, p, chains = (int(v) for v in (sys.argv[1:4] or (2000, 100, 1024)))
nsw = int(sys.argv[4]) if len(sys.argv) > 4 else 10
nseasons = int(sys.argv[5]) if len(sys.argv) > 5 else 12
rng = np.random.default_rng(8675309)
X = rng.standard_normal((T, p))
beta = np.zeros(p)
beta[:5] = rng.choice([-2.0, -1.0, 1.0, 1.5], 5)
# a level with a few shifts: what the Student trend is for
level = np.cumsum(0.1 * rng.standard_normal(T) + np.where(rng.uniform(size=T) < 0.01, 3.0 * rng.standard_normal(T), 0.0))
season = np.tile(rng.standard_normal(nseasons), T // nseasons + 1)[:T]
y = level + season + X @ beta + 0.5 * rng.standard_normal(T)
blocks = student_trend_spec(y, [("student_trend",), ("seasonal", nseasons, 1)])
g0 = np.zeros(p, np.uint8)
g0[0] = 1
prior, _, sig_up = bsts_priors(X, y, 5)
STATE, TREND = "ssm_simsmooth_kernel", "student_trend_kernels"


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


student = timed(blocks)
plain = timed(as_plain_trend(blocks))
ks, kg = student["kernel_ms_per_round"].get(STATE, 0.0), plain["kernel_ms_per_round"].get(STATE, 0.0)
print(json.dumps(dict(T=T, p=p, chains=chains, rounds=nsw, nseasons=nseasons,
                      student_trend=student, plain_trend_general_kernel=plain,
                      round_ms=[student["ms_per_round"], plain["ms_per_round"]], state_draw_ms=[ks, kg],
                      state_draw_ratio=(ks / kg) if kg else None,
                      trend_kernels_ms=student["kernel_ms_per_round"].get(TREND, 0.0))))
