"""The restatement of the Student local linear trend state model (tests/ss_student_trend_oracle.py, the
parity yardstick of state model kind 8), without a GPU:

  (a) with all weights 1 it is ss_student_oracle.impute_state's draw for the same list with kind 2
  (b) with all normals zero the draw is the posterior mean: dense_posterior's with the per-step Q_t
  (c) NuPosteriorFast and NuPosteriorRobust against scipy's gamma and t densities
  (d) the unimodal slice draw reads no uniform while it doubles
  (e) the loop cases the GPU test runs: every slice comparison has a relative margin above 1e-9
  (f) the library, the header and capi.py carry the four new entry points
"""
import os
import re

import numpy as np
import pytest
from scipy import stats

import ss_student_oracle as sso
import ss_student_trend_oracle as sto
import student_trend_cases as stc
from cases import general_data
from student_oracle import nu_log_prior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ba_ss_trend_get_weights", "ba_ss_trend_set_weights", "ba_ss_trend_get_weight_suf",
           "ba_ss_trend_draw_parameters")


def state_stream(oracle, seed, chain):
    import ctypes as C
    L = oracle.lib
    L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_rnorm.restype = C.c_double
    rng = oracle.rng_philox(seed, chain, 2, 0)
    return lambda mu, sd: L.bo_rnorm(C.byref(rng), float(mu), float(sd))


def small_case(desc, T, missing):
    X, y, _, _ = general_data(T, 3, 2, [(b[1], b[2]) for b in desc if b[0] == "seasonal"], seed=T)
    obs = np.ones(T, bool)
    obs[missing] = False
    blocks = stc.student_trend_spec(y, desc)
    return y, obs, blocks


# ---- (a) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc", [[("student_trend",)], [("seasonal", 4, 1), ("student_trend",)]])
def test_unit_weights_give_the_plain_trend_draw(oracle, desc):
    T, seed, chain, sigsq = 23, 91, 2, 0.7
    y, obs, blocks = small_case(desc, T, [5])
    S = sto.TrendStructure(blocks, T)
    var = [np.asarray(b["initial_sigma"], float) ** 2 for b in blocks]
    H = np.full(T, sigsq)
    got = sto.impute_state(S, var, y, obs, H, state_stream(oracle, seed, chain))
    want = sso.impute_state(sso.Structure(stc.as_plain_trend(blocks)), var, y, obs, H, state_stream(oracle, seed, chain))
    assert np.max(np.abs(got - want)) <= 1e-12 * np.abs(want).max()


# ---- (b) ---------------------------------------------------------------------------------------------
def test_zero_normals_give_the_dense_posterior_mean():
    T, sigsq = 14, 0.6
    y, obs, blocks = small_case([("student_trend",), ("seasonal", 4, 1)], T, [6])
    S = sto.TrendStructure(blocks, T)
    rs = np.random.Generator(np.random.PCG64(4))
    S.w = np.exp(rs.uniform(np.log(1e-2), np.log(1e2), (2, T)))   # four decades
    var = [np.asarray(b["initial_sigma"], float) ** 2 for b in blocks]
    H = np.full(T, sigsq)
    got = sto.impute_state(S, var, y, obs, H, lambda mu, sd: mu)
    mean, _ = sso.dense_posterior(S, var, y, obs, H)
    assert np.max(np.abs(got.reshape(-1) - mean)) <= 1e-9 * np.abs(mean).max()
    # ... and the weights matter: the plain trend's mean is another
    plain, _ = sso.dense_posterior(sso.Structure(stc.as_plain_trend(blocks)), var, y, obs, H)
    assert np.max(np.abs(plain - mean)) > 1e-3 * np.abs(mean).max()


# ---- (c) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", [(0, 1.0, 500.0), (1, 2.0, 0.1)])
def test_nu_posteriors_against_scipy(prior):
    rs = np.random.Generator(np.random.PCG64(8))
    w = rs.gamma(2.5, 1 / 2.5, 37)
    n, sw, sl = float(len(w)), float(np.sum(w)), float(np.sum(np.log(w)))
    for nu1, nu2 in [(1.5, 7.0), (3.0, 9.5)]:
        d = sto.nu_posterior_fast(nu1, n, sw, sl, prior) - sto.nu_posterior_fast(nu2, n, sw, sl, prior)
        ref = [np.sum(stats.gamma.logpdf(w, v / 2, scale=2 / v)) + nu_log_prior(v, prior) for v in (nu1, nu2)]
        assert abs(d - (ref[0] - ref[1])) <= 1e-10 * max(abs(ref[0]), abs(ref[1]))
    r, sigma = 0.4 * rs.standard_t(4, 41), 0.37
    for nu in (2.5, 11.0, 80.0):
        ref = np.sum(stats.t.logpdf(r / sigma, nu) - np.log(sigma)) + nu_log_prior(nu, prior)
        assert abs(sto.nu_posterior_robust(nu, r, sigma, prior) - ref) <= 1e-11 * abs(ref)
    assert sto.nu_posterior_fast(0.5, n, sw, sl, (0, 1.0, 500.0)) == -np.inf
    assert sto.nu_posterior_robust(501.0, r, sigma, (0, 1.0, 500.0)) == -np.inf


# ---- (d) ---------------------------------------------------------------------------------------------
def test_unimodal_slice_reads_no_uniform_while_doubling(oracle):
    import ctypes as C
    L = oracle.lib
    rs = np.random.Generator(np.random.PCG64(3))
    w = rs.gamma(20.0, 1 / 20.0, 60)   # nu near 40: from x = 2 with dx = 1 the limit doubles several times
    n, sw, sl = float(len(w)), float(np.sum(w)), float(np.sum(np.log(w)))
    logf = lambda nu: sto.nu_posterior_fast(nu, n, sw, sl, (0, 1.0, 500.0))   # noqa: E731
    most = 0
    for i in range(20):
        rng = oracle.rng_philox(77, i, sto.PARAM_STREAM, 0)
        info = {}
        x, _ = sto.slice_draw_unimodal(lambda: L.bo_unif(C.byref(rng)), lambda: L.bo_exp_rand(C.byref(rng)),
                                       logf, 2.0, 1.0, info)
        assert info["uniforms_in_doubling"] == 0
        assert 1.0 <= x <= 500.0
        most = max(most, info["doublings"])
    assert most >= 3


# ---- (e) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(stc.LOOP_CASES)))
def test_loop_cases_have_slice_margins(oracle, k):
    case = stc.loop_case(k)
    arms = set()
    for ch in case["check"]:
        o, ystar = stc.loop_oracle(oracle, case, ch)
        for r in range(case["rounds"]):
            arms.update(bool(v > 10) for v in o.nu)
            o.draw_parameters()
            o.impute_state(ystar, case["sigsq"])
            assert np.all(np.isfinite(o.w)) and np.all(o.w > 0)
            assert np.all(o.w[:, -1] == 1.0)   # entry T - 1 is never redrawn
        assert o.margin > 1e-9, (k, ch, o.margin)
        assert o.draws == case["rounds"]
    assert (case["nu0"][0] > 10) in arms


def test_loop_cases_cover_both_arms_and_options():
    a, b = stc.loop_case(0), stc.loop_case(1)
    assert a["nu0"][0] <= 10 < b["nu0"][0]
    assert all(np.all(np.isfinite(blk["sigma_upper_limit"])) for blk in a["blocks"])
    assert b["nu_priors"][0][0] == 1


# ---- (f) ---------------------------------------------------------------------------------------------
def test_header_declares_and_capi_binds_the_trend_entries():
    txt = open(os.path.join(ROOT, "include", "boom_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from boom_amd.capi import SIGNATURES
    import boom_amd
    lib = boom_amd.load_library()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("ss_trend_get_weights", "ss_trend_set_weights", "ss_trend_get_weight_suf", "ss_trend_draw_parameters"):
        assert hasattr(boom_amd.Engine, name), name
