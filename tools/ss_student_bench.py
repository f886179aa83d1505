#!/usr/bin/env python3
"""Diagnostic timing of the state space Student-t family (ba_ss_student_sweep): ms per round and
device time per kernel class, beside the Gaussian general-kernel round (ba_ss_sweep after
ba_ss_set_tuning(e, 0)) of the same state model list on the same data -- the number the Student
round is to be read against.  Not a bench line.
usage: ss_student_bench.py [T p chains [timed rounds [nseasons]]]   (default: T = 2000, p = 100,
1024 chains, 10 rounds; nseasons = 0: a local level, else a local linear trend + that many seasons)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import boom_amd  # noqa: E402
from cases import bsts_priors, general_spec  # noqa: E402
from ss_bench_timing import timed  # noqa: E402

T, p, chains = (int(v) for v in (sys.argv[1:4] or (2000, 100, 1024)))
nsw = int(sys.argv[4]) if len(sys.argv) > 4 else 10
nseasons = int(sys.argv[5]) if len(sys.argv) > 5 else 0
rng = np.random.default_rng(8675309)
X = rng.standard_normal((T, p))
beta = np.zeros(p)
beta[:5] = rng.choice([-2.0, -1.0, 1.0, 1.5], 5)
level = np.cumsum(0.1 * rng.standard_normal(T))
season = np.tile(rng.standard_normal(max(nseasons, 1)), T // max(nseasons, 1) + 1)[:T] if nseasons else 0.0
y = level + season + X @ beta + 0.5 * rng.standard_t(3.0, T)
desc = [("trend",), ("seasonal", nseasons, 1)] if nseasons else [("level",)]
blocks = general_spec(y, desc)
g0 = np.zeros(p, np.uint8)
g0[0] = 1


stu = boom_amd.Engine(chains, seed=4)
stu.ss_student_set_data(y, X, None)
stu.sss_set_slab(np.zeros(p), 0.01 * np.eye(p), scales_with_sigsq=True)
stu.set_spike(np.full(p, 5.0 / p))
stu.set_sigma_prior(1.0, 1.0)
stu.ss_set_state_models(blocks)
stu.set_state(g0)
student = timed(stu, stu.ss_student_sweep, nsw)
del stu

prior, _, sig_up = bsts_priors(X, y, 5)
gau = boom_amd.Engine(chains, seed=4)
gau.ss_set_data(y, X, None)
gau.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"], sigma_upper_limit=sig_up)
gau.ss_set_state_models(blocks)
gau.ss_set_tuning(kernel=0)
gau.set_state(g0)
gaussian = timed(gau, gau.ss_sweep, nsw)

ks, kg = student["kernel_ms_per_round"].get("ssm_simsmooth_kernel", 0.0), gaussian["kernel_ms_per_round"].get("ssm_simsmooth_kernel", 0.0)
print(json.dumps(dict(T=T, p=p, chains=chains, rounds=nsw, state_models=[d[0] for d in desc], nseasons=nseasons,
                      student=student, gaussian_general_kernel=gaussian,
                      state_draw_ratio=(ks / kg) if kg else None)))
