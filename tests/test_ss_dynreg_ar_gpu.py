"""The AR dynamic regression on the device (ba_ss_add_dynamic_regression_ar, bsts AddDynamicRegression with
DynamicRegressionArOptions): autoregression blocks with a row of data in the DR instances of the general
structural kernel, their ArPosteriorSampler draws, forecast, prediction errors and look-ahead.

  1 identity      xdim = 1, lags = 2, x = 1 beside [4 seasons] against [kind 4, lags = 2 | 4 seasons], both
                  through the general kernel, 12 rounds, bit for bit (SMALL; with 20 seasons more: LDC 33)
  2 scaling       x -> 2 x with a0, sigma, sigma_guess, sigma_max -> 1/2 and P0 -> 1/4, phi unchanged: the
                  coefficients' draws halve, bit for bit (tests/test_ss_dynreg_ar_cpu.py has it on the
                  restatement first)
  3 filter edges  one impute_state against the restatement (tests/ss_dynreg_ar_oracle.py) at T = 70 and 130:
                  SMALL and LDC 33, GLOB on and off, lags 1, 2 and 3, xdim 1 to 4, a plain dynamic regression
                  ahead of the model (its first column is 2), the plain form's hard rows in each
  4 whole rounds  ba_ss_sweep(1) x 12 against the restatement given the device's regression draw;
                  ba_ss_sweep(12) and ba_ss_draw_next under a look-ahead of 4 the same draws, bit for bit; a
                  second case whose every round goes through draw_phi_univariate
  5 distribution  4096 chains' state draws against the dense Gaussian posterior at fixed phi
  6 forecast      against the restatement on the forecast stream over two calls; too few rows are refused
  7 errors        ba_ss_prediction_errors by the long-double gate
  8 interface     every refusal and its text, in both orders; the accessors
  9 pybind        boom.DynamicRegressionArStateModel at the facade's default look-ahead == the plain loop

Stream positions have no accessor: a position that differs shows in the next round's draws, which every
bit-for-bit comparison below goes on to make.
"""
import ctypes as C

import numpy as np
import pytest

import prediction_errors_ref as per
import ss_dynreg_ar_cases as sac
import ss_dynreg_ar_oracle as sda
import ss_dynreg_cases as sdc
import ss_dynreg_oracle as sdo
import ss_student_oracle as sso
from cases import bsts_priors, general_spec
from ss_gpu_helpers import RTOL, close, refused
from ss_gpu_helpers import engine as list_engine

gpu = pytest.mark.gpu


def engine(chains, seed, y, X, obs, blocks, g0, kernel=None):
    return list_engine(chains, seed, y, X, obs, sda.engine_blocks(blocks), g0, kernel=kernel)


def same_model(su, sv):
    return all(np.array_equal(su[key], sv[key]) for key in ("variances", "phi", "xtx", "xty", "yty", "n"))


# ---- 1. identity ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pad", [False, True])
def test_one_predictor_of_ones_equals_an_autoregression(pad):
    """[xdim = 1, lags = 2, x = 1 | 4 seasons (| 20 seasons: state dimension 24, not SMALL)] against the same
    list with an autoregression of 2 lags (kind 4), both through the general kernel.  The products with 1.0
    are exact and the sums run in the same order: state, phi, sigma^2, statistics and -- through the rounds
    that follow -- stream positions coincide in every bit."""
    T, chains, seed, rounds = 70, 4, 79, 12
    seas = [("seasonal", 4, 1)] + ([("seasonal", 20, 1)] if pad else [])
    X, y, obs = sdc.data(T, seasonal=((4, 1),))
    sdy = float(np.std(y, ddof=1))
    plain = general_spec(y, [("ar", 2, [0.3, 0.1])] + seas)
    plain[0]["a0"] = np.array([0.375, -0.25])
    dyn = sda.dynreg_ar_blocks(np.ones((T, 1)), 2, sdy, plain[0]["initial_sigma"], [plain[0]["initial_phi"]],
                               a0=plain[0]["a0"], P0=plain[0]["P0"]) + plain[1:]
    assert sum(b["dim"] for b in dyn) == (24 if pad else 5)
    g0 = np.zeros(sdc.P, np.uint8)
    g0[0] = 1
    a = engine(chains, seed, y, X, obs, dyn, g0)
    b = engine(chains, seed, y, X, obs, plain, g0, kernel=0)
    moved = False
    for r in range(rounds):
        a.ss_sweep(1)
        b.ss_sweep(1)
        for u, v in zip(a.get_states(), b.get_states()):
            assert np.array_equal(u, v), r
        for c in range(chains):
            u, v = a.ss_get_state_draw(c), b.ss_get_state_draw(c)
            assert np.abs(v).max() > 0
            assert np.array_equal(u, v), (r, c, np.max(np.abs(u - v)))
            su, sv = a.ss_get_state_model(c, 0), b.ss_get_state_model(c, 0)
            assert same_model(su, sv), (r, c, su, sv)
            moved = moved or not np.array_equal(su["phi"], plain[0]["initial_phi"])
            for k in range(1, len(dyn)):
                su, sv = a.ss_get_state_model(c, k), b.ss_get_state_model(c, k)
                assert all(np.array_equal(su[key], sv[key]) for key in ("variances", "suf_n", "suf_ss")), (r, c, k)
            su, sv = a.ss_get_chain_suf(c), b.ss_get_chain_suf(c)
            assert su["yty"] == sv["yty"] and np.array_equal(su["xty"], sv["xty"]), (r, c)
    assert moved


# ---- 2. the scaling identity -----------------------------------------------------------------------------
@gpu
def test_scaling_the_predictors_halves_the_coefficients_bit_for_bit():
    T, chains, seed, sigsq = 70, 4, 80, 0.5
    X, y, obs = sdc.data(T)
    blocks = sac.list_small(y, T)
    blocks[2]["a0"], blocks[3]["a0"] = np.array([0.25, -1.5]), np.array([0.75, 0.5])
    gam, beta = sdc.chain_parameters(chains, 4)
    a = engine(chains, seed, y, X, obs, blocks, gam[0])
    b = engine(chains, seed, y, X, obs, sda.scaled(blocks), gam[0])
    for c in range(chains):
        a.set_state(gam[c], beta[c], sigsq, chain=c)
        b.set_state(gam[c], beta[c], sigsq, chain=c)
    a.ss_impute_state()
    b.ss_impute_state()
    for c in range(chains):
        u, v = a.ss_get_state_draw(c), b.ss_get_state_draw(c)
        assert np.abs(u[:, 4:]).max() > 0
        assert np.array_equal(v[:, :4], u[:, :4]), c
        assert np.array_equal(v[:, 4:], 0.5 * u[:, 4:]), c
        for k in (2, 3):
            su, sv = a.ss_get_state_model(c, k), b.ss_get_state_model(c, k)
            assert np.array_equal(sv["phi"], su["phi"]) and np.array_equal(su["phi"], blocks[k]["initial_phi"]), (c, k)
            assert np.array_equal(sv["variances"], 0.25 * su["variances"]), (c, k)
            assert all(np.array_equal(sv[key], 0.25 * su[key]) for key in ("xtx", "xty", "yty")) and sv["n"] == su["n"] == T - 1, (c, k)


# ---- 3. one impute_state against the restatement -----------------------------------------------------------
def check_state_models(eng, o, ch, tag):
    """variances, phi and statistics by ss_gpu_helpers.close (phi and the ArModel statistics against their
    largest entry: they are sums whose terms cancel); the state draw against its largest entry"""
    for j in range(len(o.blocks)):
        sm = eng.ss_get_state_model(ch, j)
        if o.is_ar[j]:
            assert len(sm["variances"]) == 1 and close(sm["variances"], o.var[j]), tag + (j,)
            assert np.max(np.abs(sm["phi"] - o.phi[j])) <= RTOL * max(np.abs(o.phi[j]).max(), 1e-300), tag + (j, sm["phi"], o.phi[j])
            suf = o.ar_suf[j]
            assert sm["n"] == suf["n"] == o.T - 1, tag + (j,)
            assert np.max(np.abs(sm["xtx"] - suf["xtx"])) <= RTOL * np.abs(suf["xtx"]).max(), tag + (j,)
            assert np.max(np.abs(sm["xty"] - suf["xty"])) <= RTOL * np.abs(suf["xtx"]).max(), tag + (j,)
            assert close(sm["yty"], suf["yty"]), tag + (j,)
            continue
        nv = len(sm["variances"])
        assert nv == (o.blocks[j]["dim"] if o.blocks[j]["kind"] == sdo.DYNREG else len(o.var[j])), tag + (j, nv)
        assert close(sm["variances"], o.var[j]), tag + (j,)
        assert np.array_equal(sm["suf_n"], o.suf_n[j][:nv]), tag + (j, sm["suf_n"], o.suf_n[j])
        assert close(sm["suf_ss"], o.suf_ss[j][:nv]), tag + (j,)
    st = eng.ss_get_state_draw(ch)
    err = np.max(np.abs(st - o.state))
    assert err < RTOL * np.abs(o.state).max(), tag + (err,)
    return err / np.abs(o.state).max()


@gpu
@pytest.mark.parametrize("name", list(sac.EDGE_CASES))
def test_impute_state_matches_restatement(oracle, name):
    T, make, kw = sac.EDGE_CASES[name]
    chains, seed, sigsq = 3, 43, 0.8
    X, y, obs = sdc.data(T, **kw)
    assert not obs.all()
    blocks = make(y, T)
    gam, beta = sdc.chain_parameters(chains, 8, X.shape[1])
    eng = engine(chains, seed, y, X, obs, blocks, gam[0])
    for c in range(chains):
        eng.set_state(gam[c], beta[c], sigsq, chain=c)
    eng.ss_impute_state()
    worst = 0.0
    for c in range(chains):
        o = sda.DynRegArOracle(oracle, T, obs, blocks, seed, c)
        inc = np.flatnonzero(gam[c])
        o.impute_state(y - X[:, inc] @ beta[c][inc], sigsq)
        worst = max(worst, check_state_models(eng, o, c, (name, c)))
    print("%s: state draw, worst error / max |state| %.3e" % (name, worst))


# ---- 4. whole rounds ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", ["loop", "fallback"])
def test_whole_rounds_match_restatement(oracle, which):
    c = sac.loop_case() if which == "loop" else sac.fallback_case()
    T, X, y, obs, blocks, rounds = c["T"], c["X"], c["y"], c["obs"], c["blocks"], c["rounds"]
    ar = [k for k, b in enumerate(blocks) if b["kind"] == sda.DYNREG_AR]

    def fresh():
        e = engine(c["chains"], c["seed"], y, X, obs, blocks, c["g0"])
        e.set_state(c["g0"], c["b0"], c["sig0"])
        return e

    def parameters(e, ch, k):
        sm = e.ss_get_state_model(ch, k, suf=False)
        return np.concatenate([sm["variances"], sm.get("phi", np.zeros(0))])

    eng = fresh()
    ora = {ch: sda.DynRegArOracle(oracle, T, obs, blocks, c["seed"], ch) for ch in c["check"]}
    for o in ora.values():
        o.impute_state(y - X @ c["b0"], c["sig0"])   # the first call's impute_state, with the parameters as they stand
    ob = obs.astype(bool)
    record = []
    for r in range(rounds):
        eng.ss_sweep(1)
        gam, beta, sig = eng.get_states()
        for ch, o in ora.items():
            # the state-model half, given the device's regression draw of this round
            o.draw_state_models()
            o.impute_state(y - X @ (beta[ch] * gam[ch]), sig[ch])
            check_state_models(eng, o, ch, (which, ch, r))
            # the regression's statistics of the device's own state draw
            Zs = np.array([o.S.Z(t) @ s for t, s in enumerate(eng.ss_get_state_draw(ch))])
            e = np.where(ob, y - Zs, 0.0)
            suf = eng.ss_get_chain_suf(ch)
            assert close(suf["yty"], e @ e) and np.max(np.abs(suf["xty"] - X.T @ e)) < RTOL * np.abs(X.T @ e).max(), (ch, r)
            assert suf["n"] == ob.sum()
        record.append(dict(states=(gam.copy(), beta.copy(), sig.copy()), path=eng.ss_get_state_draw(0),
                           par=[parameters(eng, 0, k) for k in range(len(blocks))]))
    for ch, o in ora.items():
        assert o.margin > 1e-9 and o.ar_margin > 1e-9, (ch, o.margin, o.ar_margin)
        # (the fallback case: every draw of the coefficient's sampler went through draw_phi_univariate)
        assert o.fallbacks == (rounds * len(ar) if which == "fallback" else 0), (ch, o.fallbacks)
    final = [[eng.ss_get_state_model(ch, k) for k in range(len(blocks))] for ch in range(c["chains"])]
    # one call of all the rounds
    eng2 = fresh()
    eng2.ss_sweep(rounds)
    for u, v in zip(eng.get_states(), eng2.get_states()):
        assert np.array_equal(u, v)
    for ch in range(c["chains"]):
        assert np.array_equal(eng.ss_get_state_draw(ch), eng2.ss_get_state_draw(ch))
        for k in range(len(blocks)):
            v = eng2.ss_get_state_model(ch, k)
            assert all(np.array_equal(final[ch][k][key], v[key]) for key in v), (ch, k)
    # ... and the same draws handed out under a look-ahead of 4: the record carries phi and the variances
    eng3 = fresh()
    eng3.ss_set_lookahead(4)
    for r in range(rounds):
        eng3.ss_draw_next()
        for u, v in zip(record[r]["states"], eng3.get_states()):
            assert np.array_equal(u, v), r
        assert np.array_equal(record[r]["path"], eng3.ss_get_state_draw(0)), r
        for k in range(len(blocks)):
            assert np.array_equal(record[r]["par"][k], parameters(eng3, 0, k)), (r, k)
    for k in range(len(blocks)):
        v = eng3.ss_get_state_model(0, k)
        assert all(np.array_equal(final[0][k][key], v[key]) for key in v), k


# ---- 5. distribution -----------------------------------------------------------------------------------------
@gpu
def test_state_draws_have_the_dense_posterior_moments():
    """level + xdim = 2, lags = 2 at T = 40, phi and the variances fixed: 200 means and 20 100 covariances"""
    T, chains, sigsq = 40, 4096, 0.6
    X, y, obs = sdc.data(T, seasonal=(), missing=(7,))
    sdy = float(np.std(y, ddof=1))
    blocks = general_spec(y, [("level",)]) + sda.dynreg_ar_blocks(sdc.predictors(T, 2, 72, hard=T), 2, sdy, [0.6, 0.4], sac.PHI2[:2])
    g0 = np.zeros(sdc.P, np.uint8)
    eng = engine(chains, 20266, y, X, obs, blocks, g0)
    eng.set_state(g0, np.zeros(sdc.P), sigsq)
    eng.ss_impute_state()
    draws = np.stack([eng.ss_get_state_draw(c).reshape(-1) for c in range(chains)])
    S = sda.Structure(blocks)
    var = [b["initial_sigma"] ** 2 for b in blocks]
    mean, cov = sda.dense_posterior(S, var, y, obs.astype(bool), np.full(T, sigsq))
    d = len(mean)
    assert d == 200
    bound = sso.bonferroni_bound(d + d * (d + 1) // 2)   # (level 1e-3, fixed with the seed before any run)
    zm, zc = sso.moment_z(draws, mean, cov)
    print("largest |z|: mean %.3f covariance %.3f, bound %.3f" % (np.abs(zm).max(), np.abs(zc).max(), bound))
    assert np.abs(zm).max() < bound
    assert np.abs(zc).max() < bound


# ---- 6. forecast -----------------------------------------------------------------------------------------------
def swept_engine(chains=4, seed=55, sweeps=3):
    T = 70
    X, y, obs = sdc.data(T)
    blocks = sac.list_small(y, T)
    g0 = np.zeros(sdc.P, np.uint8)
    g0[0] = 1
    eng = engine(chains, seed, y, X, obs, blocks, g0)
    eng.ss_sweep(sweeps)
    return eng, T, X, y, obs, blocks, seed


def oracle_at(oracle, eng, T, obs, blocks, seed, c):
    """the restatement at the device's parameters of chain c"""
    o = sda.DynRegArOracle(oracle, T, obs, blocks, seed, c)
    sm = [eng.ss_get_state_model(c, k, suf=False) for k in range(len(blocks))]
    o.var = [m["variances"] for m in sm]
    o.phi = [m["phi"] if ar else None for m, ar in zip(sm, o.is_ar)]
    o.restructure()
    return o


@gpu
def test_forecast_matches_restatement(oracle):
    """horizon 10 twice: the predictors' rows T .. T + 9; the second call reads on in the forecast stream"""
    import boom_amd
    eng, T, X, y, obs, blocks, seed = swept_engine()
    rs = np.random.Generator(np.random.PCG64(9))
    newX = rs.standard_normal((sdc.HORIZON, sdc.P))
    first, second = eng.ss_forecast(newX), eng.ss_forecast(newX)
    gam, beta, sig = eng.get_states()
    for c in range(eng.chains):
        o = oracle_at(oracle, eng, T, obs, blocks, seed, c)
        for fc in (first, second):
            want = o.forecast(eng.ss_get_state_draw(c)[-1], sig[c], newX @ (beta[c] * gam[c]))
            assert np.max(np.abs(fc[c] - want)) < RTOL * max(1.0, np.abs(want).max()), c
        assert not np.array_equal(first[c], second[c])
    with pytest.raises(boom_amd.BoomAmdError) as e:
        eng.ss_forecast(np.zeros((sdc.HORIZON + 1, sdc.P)))
    assert "the predictors of state model 2 have 80 rows: a forecast of horizon 11 needs 81" in str(e.value), str(e.value)
    # ... and served once the rows are there (add_forecast_data): all the model's columns, on its first block
    x = np.hstack([blocks[2]["predictors"], blocks[3]["predictors"]])
    eng.ss_set_dynamic_predictors(2, np.vstack([x, x[:1]]))
    assert eng.ss_forecast(np.zeros((sdc.HORIZON + 1, sdc.P))).shape == (eng.chains, sdc.HORIZON + 1)


# ---- 7. prediction errors ----------------------------------------------------------------------------------------
@gpu
def test_prediction_errors_match_restatement(oracle):
    eng, T, X, y, obs, blocks, seed = swept_engine(seed=56)
    full = eng.ss_prediction_errors(variances=True, log_likelihood=True)
    std = eng.ss_prediction_errors(standardize=True)
    gam, beta, sig = eng.get_states()
    worst = {}
    for c in range(eng.chains):
        o = oracle_at(oracle, eng, T, obs, blocks, seed, c)
        ref, gate = sda.ssm.reference_and_gate(o.S, o.var, sig[c], y, X, gam[c], beta[c], obs)
        dev = per.device_deviation(ref, full["errors"][c], full["variances"][c], std[c], full["log_likelihood"][c])
        assert np.all(full["errors"][c][obs == 0] == 0)
        for k, v in dev.items():
            r = v / gate["v" if k == "std" else k]
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= 1.0, (c, k, v, gate)
    print("worst device / gate  v %.3f  std %.3f  F %.3f  loglik %.3f" % (worst["v"], worst["std"], worst["F"], worst["loglik"]))


# ---- 8. interface ------------------------------------------------------------------------------------------------
@gpu
def test_refusals_accessors_and_their_texts():
    import boom_amd
    T = 30
    X, y, obs = sdc.data(T, seasonal=(), missing=())
    sdy = float(np.std(y, ddof=1))
    x = sdc.predictors(T, 2, 73)
    g0 = np.zeros(sdc.P, np.uint8)

    def model(pred=x, lags=2, **kw):
        """the model's one dict for ss_set_state_models"""
        phi = np.tile([0.4, 0.1][:lags], (pred.shape[1], 1))
        return dict(sda.engine_blocks(sda.dynreg_ar_blocks(pred, lags, sdy, initial_phi=phi))[0], **kw)

    def dimensions(e):
        m, nb = C.c_int32(), C.c_int32()
        assert e.lib.ba_ss_state_dimension(e._h, C.byref(m), C.byref(nb)) == 0
        return m.value, nb.value

    def blocks(pred=x, lags=2, **kw):
        return general_spec(y, [("level",)]) + [model(pred, lags, **kw)]

    eng = boom_amd.Engine(2, seed=1)
    eng.ss_set_data(y, X, None)
    # the arguments
    bad = x.copy()
    bad[3, 1] = np.inf
    refused(lambda: eng.ss_set_state_models(blocks(bad)), "the predictors of a dynamic regression must be finite")
    bad[3, 1] = np.nan
    refused(lambda: eng.ss_set_state_models(blocks(bad)), "the predictors of a dynamic regression must be finite")
    refused(lambda: eng.ss_set_state_models(blocks(P0=np.array([1.0, 1.0, 1.0, 0.0]))), "initial state variances must be positive")
    refused(lambda: eng.ss_set_state_models(blocks(sigma_upper_limit=np.array([1.0, -1.0]))), "sigma_max must be non-negative.")
    refused(lambda: eng.ss_set_state_models(blocks(initial_sigma=np.array([0.3, 0.0]))), "initial sigma must be positive")
    refused(lambda: eng.ss_set_state_models(blocks(initial_phi=np.array([0.4, 0.1, 0.7, 0.6]))), "the initial autoregression coefficients are not stationary")
    # the limits
    lag0 = dict(model(), lags=0, a0=np.zeros(0), P0=np.zeros(0), initial_phi=None)
    refused(lambda: eng.ss_set_state_models([lag0]), "lags must be positive")
    lag17 = dict(model(), lags=17, a0=np.zeros(34), P0=np.ones(34), initial_phi=None)
    refused(lambda: eng.ss_set_state_models([lag17]), "more than 16 lags")
    five = dict(model(np.ones((T, 5)), 1), initial_phi=None)
    refused(lambda: eng.ss_set_state_models([five]), "more than 4 autoregression state models")
    refused(lambda: eng.ss_set_state_models(general_spec(y, [("ar", 2), ("ar", 1), ("ar", 1)]) + [model()]),
            "more than 4 autoregression state models")
    assert dimensions(eng) == (4, 3)   # (all or none: the three autoregressions alone)
    refused(lambda: eng.ss_set_state_models(general_spec(y, [("level",)] * 7) + [model()]), "more than 8 state models")
    refused(lambda: eng.ss_set_state_models(general_spec(y, [("seasonal", 62, 1)]) + [model()]), "state dimension exceeds 64")
    refused(lambda: eng.ss_set_state_models([sdo.dynreg_block(np.ones((T, 15)), sdy), model()]), "more than 16 variance parameters")
    # a fifth slot in the other order: the model first, a kind-4 block behind four coefficients
    four = dict(model(np.ones((T, 4)), 1), initial_phi=None)
    refused(lambda: eng.ss_set_state_models([four] + general_spec(y, [("ar", 1)])), "more than 4 autoregression state models")
    # the accessors: the model's blocks are state models 1 and 2
    eng.ss_set_state_models(blocks())
    refused(lambda: eng.ss_set_dynamic_predictors(0, x[:, :1]), "not a dynamic regression state model")
    refused(lambda: eng.ss_get_dynamic_predictors(0), "not a dynamic regression state model")
    later = "a block of an AR dynamic regression that is not the model's first: its predictors are set and read on the model's first block"
    refused(lambda: eng.ss_set_dynamic_predictors(2, x), later)
    refused(lambda: eng.ss_get_dynamic_predictors(2), later)
    refused(lambda: eng.ss_set_dynamic_predictors(1, bad), "the predictors of a dynamic regression must be finite")
    assert np.array_equal(eng.ss_get_dynamic_predictors(1), x)
    # too few rows: every call that launches
    eng = list_engine(2, 1, y, X, None, blocks(x[:T - 1]), g0)
    for fn in (lambda: eng.ss_sweep(1), eng.ss_impute_state, eng.ss_draw_next, eng.ss_prediction_errors):
        refused(fn, "the predictors of state model 1 have 29 rows, the series has 30 time points")
    eng.ss_set_dynamic_predictors(1, x)
    assert np.array_equal(eng.ss_get_dynamic_predictors(1), x)
    eng.ss_sweep(2)
    for k in (1, 2):
        sm = eng.ss_get_state_model(0, k)
        assert sm["n"] == T - 1 and sm["yty"] > 0 and len(sm["variances"]) == 1 and len(sm["phi"]) == 2
        assert np.all(np.linalg.eigvalsh(sm["xtx"]) > 0)
    assert eng.ss_get_state_draw(0).shape == (T, 5)
    refused(lambda: eng.ss_forecast(np.zeros((1, sdc.P))), "a forecast of horizon 1 needs 31")
    # under a look-ahead the setter is a mutator: the draws after it are those of a run without the look-ahead
    eng.ss_set_lookahead(4)
    eng.ss_draw_next()
    eng.ss_set_dynamic_predictors(1, np.vstack([x, x[:2]]))
    eng.ss_draw_next()
    plain = list_engine(2, 1, y, X, None, blocks(), g0)
    plain.ss_sweep(4)
    for u, v in zip(eng.get_states(), plain.get_states()):
        assert np.array_equal(u, v)
    assert eng.ss_forecast(np.zeros((2, sdc.P))).shape == (2, 2)
    # the other observation families: the model added on such data ...
    text = "the dynamic regression is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)"
    from ss_family_cases import count_series, golden_mix
    Xc, counts, exposure, _ = count_series(T, sdc.P, 4)
    families = [
        (lambda e: e.ss_student_set_data(y, X, None), lambda e: e.ss_student_sweep(1), True),
        (lambda e: e.ss_poisson_set_data(counts, exposure, Xc, golden_mix(), None), lambda e: e.ss_poisson_sweep(1), False),
        (lambda e: e.ss_logit_set_data(np.minimum(counts, 3.0), np.full(T, 3.0), Xc), lambda e: e.ss_logit_sweep(1), False),
    ]
    for set_data, sweep, scales in families:
        e2 = boom_amd.Engine(2, seed=1)
        set_data(e2)
        refused(lambda: e2.ss_set_state_models(blocks()), text)
        # ... and the list first, the family's data and first call after it
        e3 = boom_amd.Engine(2, seed=1)
        e3.ss_set_data(y, X, None)
        e3.ss_set_state_models(blocks())
        set_data(e3)
        e3.sss_set_slab(np.zeros(sdc.P), 0.1 * np.eye(sdc.P), scales_with_sigsq=scales)
        e3.set_spike(np.full(sdc.P, 0.5))
        if scales:
            e3.set_sigma_prior(1.0, 1.0)
        e3.set_state(g0)
        refused(lambda: sweep(e3), text)
    # a Student local linear trend, a random-walk holiday, a calendar seasonal in the same list, in both orders
    import ss_holiday_oracle as sho
    import student_trend_cases as stc
    dyn = [model()]
    others = [
        (stc.student_trend_spec(y, [("student_trend",)]), "a list that holds both a dynamic regression and a Student local linear trend is not built"),
        ([sho.holiday_block(2, np.zeros(T, np.int32), sdy)], "a list that holds both a dynamic regression and a random-walk holiday is not built"),
        ([dict(general_spec(y, [("seasonal", 12, 1)])[0], kind="calendar_seasonal")], "a list that holds both a dynamic regression and a calendar seasonal is not built"),
    ]
    e4 = boom_amd.Engine(2, seed=1)
    e4.ss_set_data(y, X, None)
    for other, text in others:
        refused(lambda: e4.ss_set_state_models(other + dyn), text)
        refused(lambda: e4.ss_set_state_models(dyn + other), text)
    # a plain dynamic regression beside it is allowed: they share the table by column
    e5 = list_engine(2, 1, y, X, None, [sdo.dynreg_block(x, sdy)] + dyn, g0)
    e5.ss_sweep(1)
    assert dimensions(e5) == (6, 3) and e5.ss_get_state_draw(0).shape == (T, 6)
    assert np.array_equal(e5.ss_get_dynamic_predictors(0), x) and np.array_equal(e5.ss_get_dynamic_predictors(1), x)


# ---- 9. the pybind class -------------------------------------------------------------------------------------------
@gpu
def test_pybind_class_agrees_with_the_c_abi():
    """boom.DynamicRegressionArStateModel(predictors, lags) in a StateSpaceRegressionModel: three rounds at the
    facade's default look-ahead == the engine's plain loop through the C-ABI on the same seed, bit for bit"""
    import boom_amd
    import boom_amd._boom as boom
    T, chains, seed = 70, 3, 24
    X, y, obs = sdc.data(T)
    blocks = sac.loop_case()["blocks"]   # level + 4 seasons + xdim = 2, lags = 2
    prior, _, sig_up = bsts_priors(X, y, 2)
    model = boom.StateSpaceRegressionModel(y, X, [bool(o) for o in obs], chains=chains, seed=seed)
    b = blocks[0]
    level = boom.LocalLevelStateModel(float(b["initial_sigma"][0]))
    level.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    level.set_initial_state_mean(float(b["a0"][0]))
    level.set_initial_state_variance(float(b["P0"][0]))
    b = blocks[1]
    seas = boom.SeasonalStateModel(4)
    seas.set_sigsq(b["initial_sigma"][0] ** 2)
    seas.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    seas.set_initial_state_mean(b["a0"])
    seas.set_initial_state_variance(b["P0"][0])
    m = sda.engine_blocks(blocks[2:])[0]
    dyn = boom.DynamicRegressionArStateModel(m["predictors"], 2)
    assert dyn.state_dimension == 4 and dyn.xdim == 2 and dyn.lags == 2 and np.array_equal(dyn.predictors, m["predictors"])
    dyn.set_sigsq(m["initial_sigma"] ** 2)
    dyn.set_phi(m["initial_phi"])
    for i in range(2):
        dyn.set_prior(i, m["df"][i], m["sigma_guess"][i], m["sigma_upper_limit"][i])
    dyn.set_initial_state_mean(m["a0"])
    dyn.set_initial_state_variance(m["P0"])
    for s in (level, seas, dyn):
        model.add_state(s)
    sampler = boom.StateSpacePosteriorSampler(model, boom.MvnGivenScalarSigma(prior["b"], prior["ominv"]),
                                              boom.ChisqModel(prior["df"], prior["sigma_guess"]),
                                              boom.VariableSelectionPrior(prior["pi"]), sig_up)
    model.set_method(sampler)
    assert model.state_dimension == 8
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_set_data(y, X, obs)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"], sigma_upper_limit=sig_up)
    eng.ss_set_state_models(sda.engine_blocks(blocks))
    eng.set_state(np.zeros(sdc.P, np.uint8))
    for _ in range(3):
        model.sample_posterior()
        eng.ss_sweep(1)
    for u, v in zip(model.chain_states(), eng.get_states()):
        assert np.array_equal(u, v)
    for c in range(chains):
        sm = [eng.ss_get_state_model(c, k) for k in (2, 3)]
        assert np.array_equal(model.state_variances(c)[2:4], [sm[0]["variances"][0], sm[1]["variances"][0]])
        assert np.array_equal(model.dynamic_regression_ar_phi(c), np.stack([sm[0]["phi"], sm[1]["phi"]]))
        assert np.array_equal(model.state(c), eng.ss_get_state_draw(c).T)
