"""The restatement of the AR dynamic regression (tests/ss_dynreg_ar_oracle.py) pinned before anything is
compared with it, the host-only check of the list's arithmetic, and the library's new entry point -- no GPU.

  (a) ArPosteriorSampler in numpy against the C oracle (oracle/boom_oracle.c through oracle_lib): the oracle's
      general state-space model is driven round by round; after every round its autoregression block's
      ArModel statistics are recomputed from its state draw (ar_suf) and, from the second round on, phi,
      sigma^2 and the sampler's stream position are predicted from the round before -- all bit for bit.
      Three of the five cases took the fallback, draw_phi_univariate: both "fallback" cases in each of their
      5 compared draws (lags 2 narrows its interval 53 times) and the 16-lag case in one of 5 (8 candidates
      refused); 11 of the 25 draws in all.  No comparison is skipped (share 0): every stationarity decision
      of every case keeps a margin above 1e-9.
  (b) xdim = 1, x = 1 is an autoregression: the restatement's state draw equals the C oracle's for a kind-4
      block beside 4 seasons within 1e-12 (tests/test_student_trend_cpu.py's gate for its twin), round by
      round at the oracle's parameters and stream position
  (c) with zero normals impute_state is dense_posterior's mean within 1e-9: xdim = 2, lags = 2 with the plain
      form's hard rows (a column of zeros over stretches holding t = 0 and T - 1, an all-zero row, a
      missing observation)
  (d) the scaling identity: x -> 2 x with a0, sigma, sigma_guess, sigma_max -> 1/2 and P0 -> 1/4, phi
      unchanged, gives coefficient states of exactly half and the same phi over three whole rounds
  (e) the seeds of the GPU test's loops: no decision within 1e-9 of a threshold; the fallback case goes
      through draw_phi_univariate in every round, the ordinary one in none
  (f) tests/cpp/ssg_dynreg_ar_check.cpp, built with the address and undefined-behaviour sanitizers
  (g) the library exports the call and SIGNATURES binds it
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ss_dynreg_ar_cases as sac
import ss_dynreg_ar_oracle as sda
import ss_dynreg_cases as sdc
from cases import bsts_priors, general_data, general_spec
from oracle_lib import BoRng, _dp, ssvs_options

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the C oracle's general state-space model, one round at a time -------------------------------------------
def oracle_rounds(o, y, X, obs, blocks, seed, chain, rounds):
    """bo_ssm_draw x rounds on Philox streams as Oracle.ssg_run seeds them; per round: gamma, beta, sigsq of the
    regression, every block's variances and phi, the state draw, the autoregression blocks' ArModel statistics,
    and where the state stream and the blocks' sampler streams stand (the generators' raw bytes)"""
    L = o.lib
    prior, _, sig_up = bsts_priors(X, y, 2)
    m = o._ssg_build(y, X, obs, prior, blocks)
    T, p = X.shape
    reg = L.bo_ssm_regression(m)
    opts = ssvs_options(sigma_upper_limit=sig_up)
    L.bo_ssvs_set_options(reg, opts["max_model_size"], opts["sigma_upper_limit"], opts["swap_threshold"],
                          opts["max_flips"], opts["draw_beta"], opts["draw_sigma"])
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    L.bo_ssvs_set_state(reg, g0.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(np.zeros(p)), 1.0)
    L.bo_rng_seed_philox(L.bo_ssvs_rng(reg), seed, chain, 0, 0)
    nb = len(blocks)
    for b in range(nb):
        for v in range(len(blocks[b]["df"])):
            L.bo_rng_seed_philox(C.c_void_p(L.bo_ssm_block_rng(m, b, v)), seed, chain, L.bo_ssm_block_stream_id(m, b, v), 0)
    L.bo_rng_seed_philox(L.bo_ssm_state_rng(m), seed, chain, 2, 0)
    L.bo_ssm_block_get_ar_suf.argtypes = [C.c_void_p, C.c_int] + [C.POINTER(C.c_double)] * 4

    def raw(ptr):
        return bytes(C.cast(C.c_void_p(ptr), C.POINTER(BoRng)).contents)

    dim = L.bo_ssm_state_dimension(m)
    out = []
    for _ in range(rounds):
        assert L.bo_ssm_draw(m) == 0
        g, bb, s = np.zeros(p, np.uint8), np.zeros(p), C.c_double()
        L.bo_ssvs_get_state(reg, g.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(bb), C.byref(s))
        r = dict(gamma=g, beta=bb, sigsq=s.value, var=[], phi=[], suf=[], sampler=[],
                 state=np.ctypeslib.as_array(L.bo_ssm_state(m), (T, dim)).copy(), stream=raw(L.bo_ssm_state_rng(m)))
        for b in range(nb):
            var, phi = np.zeros(2), np.zeros(16)
            L.bo_ssm_block_get(m, b, _dp(var), None, None, _dp(phi))
            r["var"].append(var[:len(blocks[b]["df"])].copy())
            r["phi"].append(phi[:blocks[b]["lags"]].copy())
            r["sampler"].append(raw(L.bo_ssm_block_rng(m, b, 0)) if len(blocks[b]["df"]) else b"")
            if blocks[b]["kind"] == 4:
                Lg = blocks[b]["lags"]
                xtx, xty, yty, n = np.zeros((Lg, Lg)), np.zeros(Lg), C.c_double(), C.c_double()
                L.bo_ssm_block_get_ar_suf(m, b, _dp(xtx), _dp(xty), C.byref(yty), C.byref(n))
                r["suf"].append(dict(xtx=xtx.T.copy(), xty=xty, yty=yty.value, n=n.value))   # (column-major there)
            else:
                r["suf"].append(None)
        out.append(r)
    L.bo_ssm_destroy(m)
    return out


def growing_series(T):
    t = np.arange(T)
    return 0.5 * 1.06 ** t + 0.01 * np.sin(t)


def sampler_case(name):
    """(y, X, observed, blocks, which block is the autoregression, how many of the 5 compared draws take the
    fallback)"""
    T = 60
    X, y, _, _ = general_data(T, 3, 2, [], seed=5, ar_coef=[0.6, -0.2])
    if name == "L2":
        return y, X, None, general_spec(y, [("level",), ("ar", 2, [0.3, 0.1])]), 1, 0
    if name == "L4, missing, upper limit":
        obs = np.ones(T, np.uint8)
        obs[[7, 30]] = 0
        return y, X, obs, general_spec(y, [("ar", 4, [0.2, 0.1, 0.0, -0.1]), ("level",)]), 0, 0
    if name == "L16, no upper limit":
        blocks = general_spec(y, [("level",), ("ar", 16)])
        blocks[1]["sigma_upper_limit"] = np.array([np.inf])
        return y, X, None, blocks, 1, 1
    y = growing_series(T)
    if name == "fallback L1":
        blocks = general_spec(y, [("ar", 1, [0.5])])
        blocks[0]["sigma_upper_limit"] = np.array([np.inf])
        return y, X, None, blocks, 0, 5
    assert name == "fallback L2"
    return y, X, None, general_spec(y, [("ar", 2, [0.5, 0.1])]), 0, 5


SAMPLER_CASES = ["L2", "L4, missing, upper limit", "L16, no upper limit", "fallback L1", "fallback L2"]


@pytest.mark.parametrize("name", SAMPLER_CASES)
def test_sampler_restatement_matches_the_c_oracle_bit_for_bit(oracle, name):
    y, X, obs, blocks, which, falls_back = sampler_case(name)
    rounds, seed, chain = 6, 11 + SAMPLER_CASES.index(name), 1
    rec = oracle_rounds(oracle, y, X, obs, blocks, seed, chain, rounds)
    b = blocks[which]
    first = sum(k["dim"] for k in blocks[:which])
    samp = sda.ArSampler(oracle, b["lags"], float(b["df"][0]), float(b["sigma_guess"][0]), float(b["sigma_upper_limit"][0]))
    assert b"" != rec[0]["sampler"][which] != rec[1]["sampler"][which]
    fell = narrowed = 0
    for r in range(rounds):
        # the statistics of the round's state draw
        mine = sda.ar_suf(rec[r]["state"][:, first:first + b["lags"]])
        want = rec[r]["suf"][which]
        assert np.array_equal(mine["xtx"], want["xtx"]) and np.array_equal(mine["xty"], want["xty"]), (name, r)
        assert mine["yty"] == want["yty"] and mine["n"] == want["n"] == len(y) - 1, (name, r)
        if r == 0:
            continue
        # this round's draw from the round before: its phi, sigma^2, statistics and stream position
        rng = BoRng.from_buffer_copy(rec[r - 1]["sampler"][which])
        phi, sigsq = samp.draw(rng, rec[r - 1]["phi"][which], rec[r - 1]["var"][which][0], rec[r - 1]["suf"][which])
        assert np.array_equal(phi, rec[r]["phi"][which]), (name, r, phi, rec[r]["phi"][which])
        assert sigsq == rec[r]["var"][which][0], (name, r)
        assert bytes(rng) == rec[r]["sampler"][which], (name, r)
        assert 1 <= samp.proposals <= 3 and (samp.proposals == 3 or not samp.univariate), (name, r, samp.proposals)
        fell += samp.univariate
        narrowed += samp.narrowed
    assert samp.margin > 1e-9, (name, samp.margin)   # (no case is skipped for a decision too close to call)
    print("%s: %d of %d draws through draw_phi_univariate (%d candidates refused); smallest stationarity margin %.3e"
          % (name, fell, rounds - 1, narrowed, samp.margin))
    # (3 of the 5 cases take the fallback, 11 of the 25 draws; "fallback L2" narrows its interval on the way)
    assert fell == falls_back, (name, fell)
    if name == "fallback L2":
        assert narrowed > 0


def rnorm_from(oracle, raw):
    L = oracle.lib
    L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_rnorm.restype = C.c_double
    rng = BoRng.from_buffer_copy(raw)
    return lambda mu, sd: L.bo_rnorm(C.byref(rng), float(mu), float(sd))


def test_one_predictor_of_ones_is_an_autoregression(oracle):
    T, seed, chain, rounds = 40, 7, 2, 4
    X, y, obs = sdc.data(T, seasonal=((4, 1),), missing=(0, 17))
    sdy = float(np.std(y, ddof=1))
    plain = general_spec(y, [("ar", 2, [0.3, 0.1]), ("seasonal", 4, 1)])
    rec = oracle_rounds(oracle, y, X, obs, plain, seed, chain, rounds)
    ob = obs.astype(bool)
    worst = 0.0
    for r in range(1, rounds):
        dyn = sda.dynreg_ar_blocks(np.ones((T, 1)), 2, sdy, plain[0]["initial_sigma"], [rec[r]["phi"][0]],
                                   a0=plain[0]["a0"], P0=plain[0]["P0"]) + plain[1:]
        inc = np.flatnonzero(rec[r]["gamma"])
        got = sda.impute_state(sda.Structure(dyn), rec[r]["var"], y - X[:, inc] @ rec[r]["beta"][inc], ob,
                               np.full(T, rec[r]["sigsq"]), rnorm_from(oracle, rec[r - 1]["stream"]))
        want = rec[r]["state"]
        assert np.abs(want[:, :2]).max() > 0
        worst = max(worst, np.max(np.abs(got - want)) / np.abs(want).max())
        mine = sda.ar_suf(got[:, :2])
        for key in ("xtx", "xty", "yty"):
            assert np.allclose(mine[key], rec[r]["suf"][0][key], rtol=1e-11, atol=0), (r, key)
    print("xdim = 1, x = 1 against the C oracle's kind-4 block: relative error %.3e" % worst)
    assert worst < 1e-12


def hard_case():
    T = 30
    X, y, obs = sdc.data(T, seasonal=(), missing=(11,))
    sdy = float(np.std(y, ddof=1))
    x = sdc.predictors(T, 2, 71, hard=T)
    assert np.all(x[:5, 1] == 0) and np.all(x[T - 6:, 1] == 0) and np.all(x[9] == 0)
    assert (x < 0).any() and (x > 0).any()
    blocks = general_spec(y, [("level",)]) + sda.dynreg_ar_blocks(x, 2, sdy, [0.3, 0.6], sac.PHI2[:2], a0=[[0.25, -1.5], [0.75, 0.5]])
    return T, X, y, obs.astype(bool), blocks, [b["initial_sigma"] ** 2 for b in blocks]


def test_zero_normals_give_the_dense_posterior_mean():
    T, X, y, ob, blocks, var = hard_case()
    assert not ob[11]
    S = sda.Structure(blocks)
    H = np.full(T, 0.5)
    got = sda.impute_state(S, var, y, ob, H, lambda mu, sd: mu)
    mean, cov = sda.dense_posterior(S, var, y, ob, H)
    err = np.max(np.abs(got.reshape(-1) - mean)) / np.abs(mean).max()
    print("zero normals against the dense posterior mean: relative error %.3e" % err)
    assert err < 1e-9
    assert np.all(np.diag(cov) > 0)
    # Z_t holds x_t at the coefficients' first components and 0 on their lags
    assert np.array_equal(S.Z(3), [1.0, blocks[1]["predictors"][3, 0], 0.0, blocks[2]["predictors"][3, 0], 0.0])
    assert np.array_equal(S.Tmat(0)[1:3, 1:3], [[0.5, -0.2], [1.0, 0.0]])
    assert np.array_equal(S.rqr(0, var), [var[0][0], 0.09, 0.0, 0.36, 0.0])
    assert sda.ssm.block_stream_ids(sac.list_plain_ahead(y, T)) == [[10, 26], [1], [12], [28], [44]]


def test_scaling_the_predictors_halves_the_coefficients_bit_for_bit(oracle):
    T, X, y, ob, blocks, var = hard_case()
    a = sda.DynRegArOracle(oracle, T, ob, blocks, 9, 1)
    b = sda.DynRegArOracle(oracle, T, ob, sda.scaled(blocks), 9, 1)
    for r in range(4):
        if r:
            a.draw_state_models()
            b.draw_state_models()
        one, two = a.impute_state(y, 0.5), b.impute_state(y, 0.5)
        assert np.array_equal(two[:, 0], one[:, 0]), r
        assert np.array_equal(two[:, 1:], 0.5 * one[:, 1:]) and np.abs(one[:, 1:]).max() > 0, r
        for k in (1, 2):
            assert np.array_equal(a.phi[k], b.phi[k]), (r, k)
            assert np.array_equal(b.var[k], 0.25 * a.var[k]), (r, k)
            assert all(np.array_equal(b.ar_suf[k][key], 0.25 * a.ar_suf[k][key]) for key in ("xtx", "xty", "yty")), (r, k)
        assert np.array_equal(a.var[0], b.var[0]), r
    assert a.positions() == b.positions()
    assert not np.array_equal(a.phi[1], blocks[1]["initial_phi"])


@pytest.mark.parametrize("which", ["loop", "fallback"])
def test_gpu_loop_seeds_decide_with_margin(oracle, which):
    c = sac.loop_case() if which == "loop" else sac.fallback_case()
    ystar = c["y"] - c["X"] @ c["b0"]
    for ch in c["check"]:
        o = sda.DynRegArOracle(oracle, c["T"], c["obs"], c["blocks"], c["seed"], ch)
        o.impute_state(ystar, c["sig0"])
        for _ in range(c["rounds"]):
            o.draw_state_models()
            o.impute_state(ystar, c["sig0"])
        assert o.margin > 1e-9 and o.ar_margin > 1e-9, (ch, o.margin, o.ar_margin)
        assert all(np.all(v > 0) for v in o.var)
        assert o.fallbacks == (c["rounds"] if which == "fallback" else 0), (ch, o.fallbacks)


def test_ar_dynamic_regression_list_arithmetic():
    exe = os.path.join(HERE, "cpp", "build", "ssg_dynreg_ar_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-f", "dynreg_ar.mk", "build/ssg_dynreg_ar_check"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failures" in out.stdout, out.stdout


def test_library_exports_the_ar_dynamic_regression_entry_point():
    import boom_amd
    from boom_amd.capi import SIGNATURES
    lib = boom_amd.load_library()
    assert "ba_ss_add_dynamic_regression_ar" in SIGNATURES
    assert getattr(lib, "ba_ss_add_dynamic_regression_ar") is not None
    assert len(SIGNATURES["ba_ss_add_dynamic_regression_ar"][1]) == 13
