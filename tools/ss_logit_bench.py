#!/usr/bin/env python3
"""Diagnostic timing of the state space logit family (ba_ss_logit_sweep): ms per round and device
time per kernel class for Bernoulli data (every step on the per-trial branch) and for binomial
data at 20 trials a step (every step on the large-sample branch at clt_threshold 5), beside the
Poisson round (ba_ss_poisson_sweep) of the same state model list on the same predictors -- the
numbers the logit round is to be read against.  Not a bench line.
One JSON line per shape: a local level, then a local linear trend + 12 seasons.  A round is timed
as measuring-on-mi355x asks: a burn-in (the models grow to their size), then the median of the
timed rounds, each ended by a synchronisation; the kernel classes' device times come from a
second pass with the kernel timer on.
usage: ss_logit_bench.py [T p chains [timed rounds]]   (default: T = 2000, p = 100, 1024 chains,
10 rounds).  The Poisson counts are clipped to 26, the largest count whose mixture
tests/golden/poisson_exposure.npz holds."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import boom_amd  # noqa: E402
from cases import general_spec  # noqa: E402

T, p, chains = (int(v) for v in (sys.argv[1:4] or (2000, 100, 1024)))
nsw = int(sys.argv[4]) if len(sys.argv) > 4 else 10
TRIALS = 20
g = np.load(os.path.join(ROOT, "tests", "golden", "poisson_exposure.npz"))
mix = dict(counts=g["mix_counts"], ncomp=g["mix_ncomp"], mu=g["mix_mu"], sigma=g["mix_sigma"],
           weight=g["mix_weight"], largest_index=int(g["mix_largest_index"]))
g0 = np.zeros(p, np.uint8)
g0[0] = 1


def timed(eng, sweep):
    sweep(max(2, nsw // 2))   # burn-in: the models grow to their size
    rounds = []
    for _ in range(nsw):
        t0 = time.perf_counter()
        sweep(1)              # (synchronises)
        rounds.append(time.perf_counter() - t0)
    eng.set_kernel_timing(True)
    eng.kernel_times(reset=True)
    sweep(nsw)
    kt = eng.kernel_times(reset=True)
    eng.set_kernel_timing(False)
    return dict(ms_per_round=float(np.median(rounds)) * 1e3, ms_per_round_min=min(rounds) * 1e3,
                ms_per_round_max=max(rounds) * 1e3,
                kernel_ms_per_round={k: round(v[0] / nsw, 4) for k, v in kt.items()},
                launches_per_round={k: v[1] / nsw for k, v in kt.items()},
                kbar=float(eng.get_states()[0].sum(1).mean()))


def logit_round(successes, trials, X, blocks):
    eng = boom_amd.Engine(chains, seed=4)
    eng.ss_logit_set_data(successes, trials, X, None, clt_threshold=5)
    eng.sss_set_slab(np.zeros(p), np.eye(p), scales_with_sigsq=False)
    eng.set_spike(np.full(p, 5.0 / p))
    eng.ss_set_state_models(blocks)
    eng.set_state(g0)
    return timed(eng, eng.ss_logit_sweep)


def shape(nseasons):
    rng = np.random.default_rng(8675309)
    X = rng.standard_normal((T, p))
    beta = np.zeros(p)
    beta[:5] = rng.choice([-0.4, -0.2, 0.2, 0.3], 5)
    level = np.cumsum(0.02 * rng.standard_normal(T))
    season = (np.tile(0.3 * rng.standard_normal(nseasons), T // nseasons + 1)[:T] if nseasons else 0.0)
    eta = level + season + X @ beta
    prob = 1 / (1 + np.exp(-eta))
    bern = rng.binomial(1, prob).astype(float)
    binom = rng.binomial(TRIALS, prob).astype(float)
    exposure = rng.uniform(0.5, 2.0, T)
    counts = np.minimum(rng.poisson(exposure * np.exp(1.0 + eta)), 26).astype(float)
    y = np.log((binom + 0.5) / (TRIALS - binom + 0.5))   # (the empirical logit: it sizes the state priors)
    desc = [("trend",), ("seasonal", nseasons, 1)] if nseasons else [("level",)]
    blocks = general_spec(y, desc)

    bernoulli = logit_round(bern, np.ones(T), X, blocks)
    binomial = logit_round(binom, np.full(T, float(TRIALS)), X, blocks)

    poi = boom_amd.Engine(chains, seed=4)
    poi.ss_poisson_set_data(counts, exposure, X, mix, None)
    poi.sss_set_slab(np.zeros(p), np.eye(p), scales_with_sigsq=False)
    poi.set_spike(np.full(p, 5.0 / p))
    poi.ss_set_state_models(blocks)
    poi.set_state(g0)
    poisson = timed(poi, poi.ss_poisson_sweep)
    del poi

    draw = lambda r: r["kernel_ms_per_round"].get("ssm_simsmooth_kernel", 0.0)   # noqa: E731
    kb, kn, kp = draw(bernoulli), draw(binomial), draw(poisson)
    print(json.dumps(dict(T=T, p=p, chains=chains, rounds=nsw, state_models=[d[0] for d in desc], nseasons=nseasons,
                          logit_bernoulli=bernoulli, logit_binomial20=binomial, poisson=poisson,
                          state_draw_ratio_to_poisson=dict(bernoulli=(kb / kp) if kp else None,
                                                           binomial20=(kn / kp) if kp else None))), flush=True)


for ns in (0, 12):
    shape(ns)
