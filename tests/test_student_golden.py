"""Pins the Student-t restatement (tests/student_oracle.py, the parity yardstick of
ba_student_sweep) against fixtures of the compiled, unmodified reference's
TRegressionSpikeSlabSampler (tests/golden/make_golden_student.py).  Runs anywhere: no GPU,
no reference tree.

The restatement runs in its ("mt", seed) mode: the reference's one MT19937-64 stream in
draw() order.  Only the RNG provider differs from the substream mode the device is compared
with, so these fixtures pin the arithmetic of both.

Bars (as tests/test_oracle_golden.py): inclusion indicators bit-exact; beta, sigma^2, nu and
the complete-data suf's sum of weights, y'Wy and X'Wy <= 1e-9 relative; the slice
comparisons' smallest relative margin above 1e-9 (the restatement's log density is not the
reference's dt(), so a comparison that close could flip).  Each edge case also checks that
it reached its edge.
"""
import os

import numpy as np
import pytest

from student_oracle import StudentOracle

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-9
NAMES = ["student_base", "student_gamma_maxflips", "student_sigma_limit",
         "student_slab_mean_max_size", "student_no_selection", "student_p72",
         "student_heavy_tails", "student_gaussian", "student_start"]


def relerr(a, b, floor=1e-3):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def run_restatement(oracle, g):
    nup = g["nu_prior"]
    o = StudentOracle(oracle, g["X"], g["y"], g["mu"], g["prec"], g["pi"], 0, 0, g["init_gamma"],
                      beta0=g["init_beta"], sigsq0=float(g["init_sigsq"]),
                      nu0=float(g["init_nu"]), nu_prior=(int(nup[0]), float(nup[1]), float(nup[2])),
                      sigma_prior=tuple(float(v) for v in g["sigma_prior"]),
                      sigma_max=float(g["sigma_max"]), max_flips=int(g["max_flips"]),
                      max_model_size=int(g["max_model_size"]),
                      allow_selection=bool(g["allow_selection"]), rng_setup=("mt", int(g["seed"])))
    sufs = []
    for s in range(int(g["nsweeps"])):
        gam, beta, sigsq, nu = o.draw()
        assert np.array_equal(gam, g["gamma"][s]), s
        assert relerr(beta, g["beta"][s]) < RTOL, s
        assert relerr(sigsq, g["sigsq"][s]) < RTOL, s
        assert relerr(nu, g["nu"][s]) < RTOL, s
        assert relerr(o.suf["sumw"], g["sumw"][s]) < RTOL, s
        assert relerr(o.suf["yty"], g["yty"][s]) < RTOL, s
        assert relerr(o.suf["xty"], g["xty"][s]) < RTOL, s
        sufs.append(dict(o.suf))
    assert o.margin > 1e-9, o.margin
    return o, sufs


@pytest.mark.parametrize("name", NAMES)
def test_student_restatement_matches_reference(oracle, name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    o, sufs = run_restatement(oracle, g)
    nu, sigsq, gam = g["nu"], g["sigsq"], g["gamma"]
    p = g["X"].shape[1]
    # what each case is there for
    if name == "student_heavy_tails":
        assert nu.min() < 1.0                                # the weights' GS branch
    if name == "student_gaussian":
        assert nu.max() > 90.0                               # near Uniform(0.1, 100)'s bound
    if name == "student_sigma_limit":
        smax2 = float(g["sigma_max"]) ** 2
        assert np.all(sigsq <= smax2)
        # the untruncated 1 / sigma^2 | . has its mode below the cut 1 / sigma_max^2: the
        # truncated draw lies beyond the mode
        n, df = g["X"].shape[0], float(g["sigma_prior"][0])
        ss = np.array([s["wsse_suf"] for s in sufs]) + df * float(g["sigma_prior"][1]) ** 2
        mode = (n + df - 2) / ss
        assert np.sum(mode < 1.0 / smax2) >= len(ss) // 2
    if name == "student_gamma_maxflips":
        assert int(g["nu_prior"][0]) == 1
        assert np.all(np.sum(gam[1:] != gam[:-1], axis=1) <= int(g["max_flips"]))
    if name == "student_slab_mean_max_size":
        assert np.all(gam.sum(axis=1) <= int(g["max_model_size"]))
        assert np.any(g["mu"] != 0)
    if name == "student_no_selection":
        assert np.all(gam == g["init_gamma"])
    if name == "student_p72":
        assert gam.sum(axis=1).max() > 64 and p > 64
    if name == "student_start":
        assert float(g["init_nu"]) != 30.0 and float(g["init_sigsq"]) != 1.0
        assert np.any(g["init_beta"] != 0)
    # the suf the weights built: sum of weights against n, y'Wy against the data
    assert np.all(g["sumw"] > 0) and np.all(g["yty"] > 0)
