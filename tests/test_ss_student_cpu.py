"""The yardstick of the state space Student-t family (tests/ss_student_oracle.py) checked on
the CPU before the device is compared with it:
  1. with all weights 1 its filter and smoother reproduce the oracle's state draws of the
     Gaussian structural model (Oracle.ssg_run: the C restatement pinned on the compiled
     reference) for the same seed, blocks and parameters, within 1e-12 relative;
  2. with fixed parameters and varying weights its state draws have the mean and covariance
     of the joint Gaussian posterior computed by one dense solve (dense_posterior, written
     without a filter);
  3. the seeds of the device's whole-round parity cases (tests/test_ss_student_gpu.py) keep
     their slice margins above the skip threshold, so that no case there is skipped.
"""
import ctypes as C

import numpy as np
import pytest
import ss_student_oracle as sso
from cases import bsts_priors, general_data, general_spec
from oracle_lib import ssvs_options
from ss_family_cases import ROUND_CASES, round_case


@pytest.mark.parametrize("desc,T,missing", [
    ([("trend",), ("seasonal", 4, 1)], 70, 0.05),
    ([("level",), ("seasonal", 5, 3, 1)], 45, 0.0),
    ([("seasonal", 20, 1)], 40, 0.05),
])
def test_unit_weights_reproduce_the_gaussian_oracle(oracle, desc, T, missing):
    p, seed, chain, nsw = 4, 23, 2, 3
    seas = [(b[1], b[2]) for b in desc if b[0] == "seasonal"]
    X, y, _, obs = general_data(T, p, 2, seas, seed=3 + T, missing_frac=missing)
    obs = np.ones(T, np.uint8) if obs is None else obs
    prior, _, sig_up = bsts_priors(X, y, 2)
    blocks = general_spec(y, desc)
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    ref = oracle.ssg_run(y, X, obs, prior, ssvs_options(sigma_upper_limit=sig_up), blocks,
                         ("philox", seed, chain), g0, nsw)
    assert ref["status"] == 0
    L = oracle.lib
    L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_rnorm.restype = C.c_double
    rng = oracle.rng_philox(seed, chain, 2, 0)
    rnorm = lambda mu, sd: L.bo_rnorm(C.byref(rng), float(mu), float(sd))   # noqa: E731
    S = sso.Structure(blocks)
    ob = obs.astype(bool)
    # the sampler's first impute_state: the parameters as they were set
    var = [np.asarray(b["initial_sigma"], float) ** 2 for b in blocks]
    sso.impute_state(S, var, y.copy(), ob, np.full(T, 1.0), rnorm)
    for s in range(nsw):
        var = [ref["variances"][s, k, :len(var[k])] for k in range(len(blocks))]
        inc = np.flatnonzero(ref["gamma"][s])
        ystar = y - X[:, inc] @ ref["beta"][s][inc]
        H = sso.observation_variances(np.ones(T), np.ones(T, bool), ref["sigsq"][s], 30.0)
        st = sso.impute_state(S, var, ystar, ob, H, rnorm)
        scale = np.abs(ref["state"][s]).max()
        assert np.max(np.abs(st - ref["state"][s])) < 1e-12 * scale, s


def test_varying_weights_match_the_dense_posterior():
    S, var, y, obs, w, sigsq, nu, H = sso.fixed_case()[1:]
    assert H[3] == sigsq * nu / (nu - 2) and H[7] == H[3]
    mean, cov = sso.dense_posterior(S, var, y, obs, H)
    # fixed before any draw was looked at: the seed, the number of draws and the bound
    n, seed = 20000, 20261
    d = len(mean)
    bound = sso.bonferroni_bound(d + d * (d + 1) // 2)
    rs = np.random.Generator(np.random.PCG64(seed))
    rnorm = lambda mu, sd: mu if sd == 0 else mu + sd * rs.standard_normal()   # noqa: E731
    FK = sso.gains(S, var, obs, H)
    draws = np.stack([sso.impute_state(S, var, y, obs, H, rnorm, FK).reshape(-1) for _ in range(n)])
    zm, zc = sso.moment_z(draws, mean, cov)
    print("largest |z|: mean %.3f covariance %.3f, bound %.3f" % (np.abs(zm).max(), np.abs(zc).max(), bound))
    assert np.abs(zm).max() < bound
    assert np.abs(zc).max() < bound


def test_parity_seeds_keep_their_margins(oracle):
    """the whole-round cases of the device test: every checked chain's slice margin stays
    above 1e-9 over the rounds compared, so none of them is skipped (the cap is one in ten)"""
    cases = range(len(ROUND_CASES["student"]))
    skipped = 0
    for k in cases:
        c = round_case("student", k)
        for chain in c["check"]:
            o = c["oracle"](oracle, chain)
            for _ in range(c["rounds"]):
                o.draw()
            skipped += o.margin < 1e-9
    total = sum(len(round_case("student", k)["check"]) for k in cases)
    assert skipped * 10 <= total, (skipped, total)
