#!/usr/bin/env python3
"""Diagnostic timing of the state space Poisson family (ba_ss_poisson_sweep): ms per round and
device time per kernel class, beside the Student-t round (ba_ss_student_sweep) and the Gaussian
general-kernel round (ba_ss_sweep after ba_ss_set_tuning(e, 0)) of the same state model list on
the same predictors -- the numbers the Poisson round is to be read against.  Not a bench line.
One JSON line per shape: a local level, then a local linear trend + 12 seasons.
usage: ss_poisson_bench.py [T p chains [timed rounds]]   (default: T = 2000, p = 100, 1024 chains,
10 rounds).  The counts are clipped to 26, the largest count whose mixture
tests/golden/poisson_exposure.npz holds."""
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
g = np.load(os.path.join(ROOT, "tests", "golden", "poisson_exposure.npz"))
mix = dict(counts=g["mix_counts"], ncomp=g["mix_ncomp"], mu=g["mix_mu"], sigma=g["mix_sigma"],
           weight=g["mix_weight"], largest_index=int(g["mix_largest_index"]))
g0 = np.zeros(p, np.uint8)
g0[0] = 1


def shape(nseasons):
    rng = np.random.default_rng(8675309)
    X = rng.standard_normal((T, p))
    beta = np.zeros(p)
    beta[:5] = rng.choice([-0.4, -0.2, 0.2, 0.3], 5)
    level = 1.0 + np.cumsum(0.02 * rng.standard_normal(T))
    season = (np.tile(0.3 * rng.standard_normal(nseasons), T // nseasons + 1)[:T] if nseasons else 0.0)
    exposure = rng.uniform(0.5, 2.0, T)
    counts = np.minimum(rng.poisson(exposure * np.exp(level + season + X @ beta)), 26).astype(float)
    y = np.log(counts + 0.5)   # (the Gaussian and Student rounds' series; it sizes the state priors)
    desc = [("trend",), ("seasonal", nseasons, 1)] if nseasons else [("level",)]
    blocks = general_spec(y, desc)

    poi = boom_amd.Engine(chains, seed=4)
    poi.ss_poisson_set_data(counts, exposure, X, mix, None)
    poi.sss_set_slab(np.zeros(p), np.eye(p), scales_with_sigsq=False)
    poi.set_spike(np.full(p, 5.0 / p))
    poi.ss_set_state_models(blocks)
    poi.set_state(g0)
    poisson = timed(poi, poi.ss_poisson_sweep, nsw)
    del poi

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
    del gau

    draw = lambda r: r["kernel_ms_per_round"].get("ssm_simsmooth_kernel", 0.0)   # noqa: E731
    kp, ks, kg = draw(poisson), draw(student), draw(gaussian)
    print(json.dumps(dict(T=T, p=p, chains=chains, rounds=nsw, state_models=[d[0] for d in desc], nseasons=nseasons,
                          poisson=poisson, student=student, gaussian_general_kernel=gaussian,
                          state_draw_ratio_to_student=(kp / ks) if ks else None,
                          state_draw_ratio_to_gaussian=(kp / kg) if kg else None)), flush=True)


for ns in (0, 12):
    shape(ns)
