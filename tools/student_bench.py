#!/usr/bin/env python3
"""Diagnostic timing of the Student-t spike-and-slab path (ba_student_sweep): ms per round,
device time per kernel class, and the phase split (imputation + GEMMs, vectors of V, sweep,
sigma^2 / nu).  Not a bench line.
usage: student_bench.py [n p signals chains [timed sweeps]]   (default: the headline shape,
n = 1e4, p = 512, 8 signals, 1024 chains)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import boom_amd  # noqa: E402

n, p, nsig, chains = (int(v) for v in (sys.argv[1:5] or (10000, 512, 8, 1024)))
nsw = int(sys.argv[5]) if len(sys.argv) > 5 else 20
rng = np.random.default_rng(8675309)
X = rng.standard_normal((n, p))
X[:, 0] = 1.0
beta = np.zeros(p)
beta[:nsig] = rng.choice([-2.0, -1.0, 1.0, 1.5], nsig)
y = X @ beta + rng.standard_t(3.0, n)
eng = boom_amd.Engine(chains, seed=4)
eng.student_set_data(X, y)
eng.sss_set_slab(np.zeros(p), 0.01 * np.eye(p), scales_with_sigsq=True)
eng.set_spike(np.full(p, min(0.5, nsig / p)))
eng.set_sigma_prior(1.0, 1.0)
eng.student_set_nu_prior(0, 0.1, 100.0)
g0 = np.zeros(p, np.uint8)
g0[0] = 1
eng.set_state(g0)
eng.student_sweep(max(2, nsw // 2))          # burn-in: the models grow to their size
t0 = time.perf_counter()
eng.student_sweep(nsw)
dt = time.perf_counter() - t0
eng.set_kernel_timing(True)
eng.kernel_times(reset=True)
eng.student_sweep(nsw)
kt = eng.kernel_times(reset=True)
eng.set_kernel_timing(False)
gam = eng.get_states()[0]
per = {k: v[0] / nsw for k, v in kt.items()}
new = per.get("student_impute_kernel", 0.0) + per.get("student_sigma_nu_kernel", 0.0)
gemm = (per.get("xtwx_cols_kernel<false>+plain_reduce_kernel", 0.0)
        + per.get("xtwx_cols_kernel<true>+xtwx_cols_reduce_kernel", 0.0))
out = dict(n=n, p=p, chains=chains, sweeps=nsw, ms_per_round=dt / nsw * 1e3,
           kernel_ms_per_round={k: round(v, 4) for k, v in per.items()},
           launches={k: v[1] for k, v in kt.items()},
           phases_ms=dict(impute=per.get("student_impute_kernel", 0.0),
                          rows_gemm=per.get("xtwx_cols_kernel<false>+plain_reduce_kernel", 0.0),
                          cols_gemm=per.get("xtwx_cols_kernel<true>+xtwx_cols_reduce_kernel", 0.0),
                          sweep=per.get("ssvs_sweep_kernel", 0.0) + per.get("ssvs_big_kernel", 0.0),
                          sigma_nu=per.get("student_sigma_nu_kernel", 0.0)),
           new_over_gemm=(new / gemm) if gemm else None,
           kbar=float(gam.sum(1).mean()), nu_mean=float(eng.student_get_nu().mean()))
print(json.dumps(out))
