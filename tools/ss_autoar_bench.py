#!/usr/bin/env python3
"""Diagnostic timing of the spike-and-slab autoregression state model (state model kind 9, bsts
AddAutoAr): ms per round and device time per kernel class of ba_ss_sweep on [trend, AutoAr(lags)],
beside [trend, Ar(lags)] (kind 4, the ArPosteriorSampler inside the state kernel) through the same
general kernel (ba_ss_set_tuning(e, 0)) on the same data.  Not a bench line.
usage: ss_autoar_bench.py [T p chains [timed rounds [lags]]]   (default: T = 2000, p = 100, 1024 chains,
10 rounds, 10 lags)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import boom_amd  # noqa: E402
from autoar_cases import as_plain_ar, autoar_spec  # noqa: E402
from cases import bsts_priors  # noqa: E402

T, p, chains = (int(v) for v in (sys.argv[1:4] or (2000, 100, 1024)))
nsw = int(sys.argv[4]) if len(sys.argv) > 4 else 10
lags = int(sys.argv[5]) if len(sys.argv) > 5 else 10
rng = np.random.default_rng(8675309)
X = rng.standard_normal((T, p))
beta = np.zeros(p)
beta[:5] = rng.choice([-2.0, -1.0, 1.0, 1.5], 5)
# a slow level and an AR(2) of which the prior has to find the order
u = np.zeros(T)
e = 0.5 * rng.standard_normal(T)
for t in range(2, T):
    u[t] = 0.6 * u[t - 1] - 0.3 * u[t - 2] + e[t]
y = np.cumsum(0.02 + 0.05 * rng.standard_normal(T)) + u + X @ beta + 0.3 * rng.standard_normal(T)
# bsts's AddAutoAr defaults: a zero-mean slab, inclusion probability falling with the lag
opt = dict(truncate=1, slab_mean=np.zeros(lags), slab_precision=np.eye(lags) / 0.25,
           inclusion_probabilities=0.8 ** np.arange(1, lags + 1))
blocks = autoar_spec(y, [("trend",), ("autoar", lags, opt)])
g0 = np.zeros(p, np.uint8)
g0[0] = 1
prior, _, sig_up = bsts_priors(X, y, 5)
STATE, SPIKE = "ssm_simsmooth_kernel", "ar_spike_kernel"


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
    out = dict(ms_per_round=dt / nsw * 1e3, kernel_ms_per_round={k: round(v[0] / nsw, 4) for k, v in kt.items()},
               launches_per_round={k: v[1] / nsw for k, v in kt.items()},
               kbar=float(eng.get_states()[0].sum(1).mean()))
    if any(b["kind"] == 9 for b in state_models):
        out["lags_included"] = float(np.mean([eng.ss_get_ar_inclusion(c, 1).sum() for c in range(min(chains, 64))]))
    return out


auto = timed(blocks)
plain = timed(as_plain_ar(blocks))
ks, kg = auto["kernel_ms_per_round"].get(STATE, 0.0), plain["kernel_ms_per_round"].get(STATE, 0.0)
print(json.dumps(dict(T=T, p=p, chains=chains, rounds=nsw, lags=lags, auto_ar=auto, plain_ar=plain,
                      round_ms=[auto["ms_per_round"], plain["ms_per_round"]], state_kernel_ms=[ks, kg],
                      ar_spike_kernel_ms=auto["kernel_ms_per_round"].get(SPIKE, 0.0))))
