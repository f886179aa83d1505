#!/usr/bin/env python3
"""Diagnostic timing of the multinomial logit spike-and-slab path (ba_mlogit_sweep): ms per round,
device time per kernel class, the phase split (imputation, the two GEMM-shaped kernels, sweep),
the share of the round's kernel time spent in those two, and the mean model size.  Not a bench line.
usage: mlogit_bench.py [n M psub pch chains [rounds]]   (default: n = 1e4, M = 4, psub = 128,
pch = 0, 1024 chains, 10 rounds)
The subject block of choice m is zero outside rows i M + m: the GEMM and column kernels run over
the whole expanded design, zeros included, so their share here is what exploiting the block
structure could take away."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import boom_amd  # noqa: E402

n, M, psub, pch, chains = (int(v) for v in (sys.argv[1:6] or (10000, 4, 128, 0, 1024)))
nsw = int(sys.argv[6]) if len(sys.argv) > 6 else 10
nsig = 4
rng = np.random.default_rng(8675309)
Xs = rng.standard_normal((n, psub))
Xs[:, 0] = 1.0
Xc = rng.standard_normal((n * M, pch)) if pch else None
D = (M - 1) * psub + pch
B = np.zeros((M, psub))                      # row m: choice m's subject coefficients (0: the baseline)
for m in range(1, M):
    B[m, :nsig] = rng.choice([-1.5, -1.0, 1.0, 1.5], nsig)
eta = Xs @ B.T
if pch:
    eta += (Xc @ rng.choice([-1.0, 1.0], pch)).reshape(n, M)
g = -np.log(-np.log(rng.random((n, M))))     # Gumbel utilities: the multinomial logit law
y = np.argmax(eta + g, axis=1).astype(np.int32)
eng = boom_amd.Engine(chains, seed=4)
eng.mlogit_set_data(y, Xs, Xc, M)
eng.sss_set_slab(np.zeros(D), 0.01 * np.eye(D), scales_with_sigsq=False)
pi = np.full(D, min(0.5, nsig * (M - 1) / D))
pi[0] = 1.0                                  # (a forced intercept: the empty model is absorbing)
eng.set_spike(pi)
g0 = np.zeros(D, np.uint8)
g0[0] = 1
eng.set_state(g0)
eng.mlogit_sweep(max(2, nsw // 2))           # burn-in: the models grow to their size
t0 = time.perf_counter()
eng.mlogit_sweep(nsw)
dt = time.perf_counter() - t0
eng.set_kernel_timing(True)
eng.kernel_times(reset=True)
eng.mlogit_sweep(nsw)
kt = eng.kernel_times(reset=True)
eng.set_kernel_timing(False)
gam = eng.get_states()[0]
per = {k: v[0] / nsw for k, v in kt.items()}
rows = per.get("xtwx_cols_kernel<false>+plain_reduce_kernel", 0.0)
cols = per.get("xtwx_cols_kernel<true>+xtwx_cols_reduce_kernel", 0.0)
total = sum(per.values())
out = dict(n=n, M=M, psub=psub, pch=pch, D=D, chains=chains, rounds=nsw, ms_per_round=dt / nsw * 1e3,
           kernel_ms_per_round={k: round(v, 4) for k, v in per.items()},
           launches={k: v[1] for k, v in kt.items()},
           phases_ms=dict(impute=per.get("mlogit_impute_kernel", 0.0), rows_gemm=rows, cols_gemm=cols,
                          sweep=per.get("ssvs_sweep_kernel", 0.0)),
           gemm_share_of_kernel_time=(rows + cols) / total if total > 0 else None,
           kbar=float(gam.sum(1).mean()))
print(json.dumps(out))
