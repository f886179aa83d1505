#!/usr/bin/env python3
"""Diagnostic timing of the quantile regression spike-and-slab path (ba_quantile_sweep): ms per
round, device time per kernel class, and the phase split (imputation, GEMMs, vectors of V,
sweep).  Not a bench line.
usage: quantile_bench.py [n p signals chains [timed sweeps [quantile]]]   (default: the headline
shape, n = 1e4, p = 512, 8 signals, 1024 chains, the median)"""
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
q = float(sys.argv[6]) if len(sys.argv) > 6 else 0.5
rng = np.random.default_rng(8675309)
X = rng.standard_normal((n, p))
X[:, 0] = 1.0
beta = np.zeros(p)
beta[:nsig] = rng.choice([-2.0, -1.0, 1.0, 1.5], nsig)
y = X @ beta + rng.standard_t(3.0, n)
eng = boom_amd.Engine(chains, seed=4)
eng.quantile_set_data(X, y, q)
eng.sss_set_slab(np.zeros(p), 0.01 * np.eye(p), scales_with_sigsq=False)
eng.set_spike(np.full(p, min(0.5, nsig / p)))
g0 = np.zeros(p, np.uint8)
g0[0] = 1
eng.set_state(g0)
eng.quantile_sweep(max(2, nsw // 2))          # burn-in: the models grow to their size
t0 = time.perf_counter()
eng.quantile_sweep(nsw)
dt = time.perf_counter() - t0
eng.set_kernel_timing(True)
eng.kernel_times(reset=True)
eng.quantile_sweep(nsw)
kt = eng.kernel_times(reset=True)
eng.set_kernel_timing(False)
gam = eng.get_states()[0]
per = {k: v[0] / nsw for k, v in kt.items()}
imp = kt.get("quantile_impute_kernel", (0.0, 0))
out = dict(n=n, p=p, chains=chains, sweeps=nsw, quantile=q, ms_per_round=dt / nsw * 1e3,
           kernel_ms_per_round={k: round(v, 4) for k, v in per.items()},
           launches={k: v[1] for k, v in kt.items()},
           impute_ms_per_launch=(imp[0] / imp[1]) if imp[1] else None,
           phases_ms=dict(impute=per.get("quantile_impute_kernel", 0.0),
                          rows_gemm=per.get("xtwx_cols_kernel<false>+plain_reduce_kernel", 0.0),
                          cols_gemm=per.get("xtwx_cols_kernel<true>+xtwx_cols_reduce_kernel", 0.0),
                          sweep=per.get("ssvs_sweep_kernel", 0.0) + per.get("ssvs_big_kernel", 0.0)),
           kbar=float(gam.sum(1).mean()))
print(json.dumps(out))
