"""The dynamic regression state model on the device (ba_ss_add_dynamic_regression, bsts AddDynamicRegression
with independent random walks): the DR instances of the general structural kernel (an observation row of
data), the variance draws, forecast, prediction errors and look-ahead.

  1 identity      d = 1, x = 1 beside [4 seasons] against [level + 4 seasons], bit for bit (SMALL, LDC 33)
  2 doubling      x -> 2 x with a0, sigma -> 1/2 and P0 -> 1/4: the coefficients' draws halve, bit for bit
  3 filter edges  one impute_state against the restatement (tests/ss_dynreg_oracle.py) at T = 70 and 130:
                  SMALL with first != 0, SMALL at its edge (d = 16 alone), LDC 33, GLOB, two dynamic blocks;
                  test (b)'s hard rows in each (a column of zeros over stretches holding t = 0 and T - 1,
                  all-zero rows -- one on the last step of a time block --, a missing observation, mixed
                  signs).  Every list keeps 64 steps per time block but d = 16 alone, which the LDS of its
                  predictor rows brings to 32 (tests/cpp/ssg_dynreg_check.cpp): its edges are 31 | 32, ...
  4 whole rounds  ba_ss_sweep(1) x 12 against the restatement given the device's regression draw;
                  ba_ss_sweep(12) and ba_ss_draw_next under a look-ahead of 4 the same draws, bit for bit
  5 distribution  4096 chains' state draws against the dense Gaussian posterior
  6 forecast      against the restatement on the forecast stream; too few predictor rows are refused
  7 errors        ba_ss_prediction_errors by ss_holiday_oracle's long-double gate
  8 interface     every refusal and its text, in both orders
  9 pybind        boom.DynamicRegressionStateModel at the facade's default look-ahead == the plain loop
"""
import numpy as np
import pytest

import prediction_errors_ref as per
import ss_dynreg_cases as sdc
import ss_dynreg_oracle as sdo
import ss_holiday_oracle as sho
import ss_student_oracle as sso
from cases import bsts_priors, general_spec
from ss_gpu_helpers import RTOL, close, engine, refused
from test_ss_dynreg_cpu import doubled

gpu = pytest.mark.gpu


# ---- 1. identity ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pad", [False, True])
def test_one_predictor_of_ones_equals_a_local_level(pad):
    """[d = 1, x = 1 | 4 seasons (| 20 seasons: state dimension 23, not SMALL)] against the same list with
    a local level, both through the general kernel; equal variances as given.  The products with 1.0 are
    exact and the sums run in the same order: every bit coincides."""
    T, chains, seed, sigsq = 70, 4, 77, 0.5
    seas = [("seasonal", 4, 1)] + ([("seasonal", 20, 1)] if pad else [])
    X, y, obs = sdc.data(T, seasonal=((4, 1),))
    sdy = float(np.std(y, ddof=1))
    plain = general_spec(y, [("level",)] + seas)
    plain[0]["a0"] = np.array([0.375])
    dyn = [sdo.dynreg_block(np.ones((T, 1)), sdy, plain[0]["initial_sigma"], a0=plain[0]["a0"])] + plain[1:]
    dyn[0]["P0"] = plain[0]["P0"]
    assert sum(b["dim"] for b in dyn) == (23 if pad else 4)
    gam, beta = sdc.chain_parameters(chains, 3)
    a = engine(chains, seed, y, X, obs, dyn, gam[0])
    b = engine(chains, seed, y, X, obs, plain, gam[0], kernel=0)
    for c in range(chains):
        a.set_state(gam[c], beta[c], sigsq, chain=c)
        b.set_state(gam[c], beta[c], sigsq, chain=c)
    a.ss_impute_state()
    b.ss_impute_state()
    for c in range(chains):
        u, v = a.ss_get_state_draw(c), b.ss_get_state_draw(c)
        assert np.abs(v).max() > 0
        assert np.array_equal(u, v), (c, np.max(np.abs(u - v)))
        for k in range(len(dyn)):
            su, sv = a.ss_get_state_model(c, k), b.ss_get_state_model(c, k)
            assert np.array_equal(su["suf_n"], sv["suf_n"]), (c, k)
            assert np.array_equal(su["suf_ss"], sv["suf_ss"]), (c, k)
        su, sv = a.ss_get_chain_suf(c), b.ss_get_chain_suf(c)
        assert su["yty"] == sv["yty"] and np.array_equal(su["xty"], sv["xty"]), c


# ---- 2. the doubling identity ----------------------------------------------------------------------------
@gpu
def test_doubling_the_predictors_halves_the_coefficients_bit_for_bit():
    T, chains, seed, sigsq = 70, 4, 78, 0.5
    X, y, obs = sdc.data(T)
    blocks = sdc.list_small(y, T)
    blocks[2]["a0"] = np.array([0.25, -1.5, 0.75])
    gam, beta = sdc.chain_parameters(chains, 4)
    a = engine(chains, seed, y, X, obs, blocks, gam[0])
    b = engine(chains, seed, y, X, obs, doubled(blocks), gam[0])
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
        su, sv = a.ss_get_state_model(c, 2), b.ss_get_state_model(c, 2)
        assert np.array_equal(sv["suf_ss"], 0.25 * su["suf_ss"]) and np.array_equal(sv["suf_n"], su["suf_n"]), c


# ---- 3. one impute_state against the restatement -----------------------------------------------------------
GLOB_DATA = dict(seasonal=(), trig=[(12.0, [1.0, 2.0])], missing=(31, 64, 128))
EDGE_CASES = {
    "small, T=70": (70, sdc.list_small, {}),
    "small, T=130": (130, sdc.list_small, {}),
    "edge (d = 16 alone), T=70": (70, sdc.list_edge, dict(seasonal=())),
    "edge (d = 16 alone), T=130": (130, sdc.list_edge, dict(seasonal=())),
    "LDC 33, T=70": (70, sdc.list_ldc33, dict(seasonal=((20, 1),))),
    "LDC 33, T=130": (130, sdc.list_ldc33, dict(seasonal=((20, 1),))),
    "GLOB, T=70": (70, sdc.list_glob, GLOB_DATA),
    "GLOB, T=130": (130, sdc.list_glob, GLOB_DATA),
    "two blocks, T=70": (70, sdc.list_two, dict(seasonal=())),
    "two blocks, T=130": (130, sdc.list_two, dict(seasonal=())),
    # the dynamic regression's instances no list above reaches (2 chains, p = 2)
    "instance LDC 33, GLOB": sdc.instance_case(18, True),
    "instance LDC 61": sdc.instance_case(34, False),
    "instance LDC 61, GLOB": sdc.instance_case(34, True),
    "instance LDC 65": sdc.instance_case(61, False),
    "instance LDC 65, GLOB": sdc.instance_case(61, True),
}


def check_state_models(eng, o, ch, tag):
    for j in range(len(o.blocks)):
        sm = eng.ss_get_state_model(ch, j)
        nv = len(sm["variances"])
        assert nv == (o.blocks[j]["dim"] if o.blocks[j]["kind"] == sdo.DYNREG else len(o.var[j])), tag + (j, nv)
        assert close(sm["variances"], o.var[j]), tag + (j,)
        assert np.array_equal(sm["suf_n"], o.suf_n[j][:nv]), tag + (j, sm["suf_n"], o.suf_n[j])
        assert close(sm["suf_ss"], o.suf_ss[j][:nv]), tag + (j,)
    st = eng.ss_get_state_draw(ch)
    err = np.max(np.abs(st - o.state))
    assert err < 1e-8 * np.abs(o.state).max(), tag + (err,)
    return err / np.abs(o.state).max()


@gpu
@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_impute_state_matches_restatement(oracle, name):
    T, make, kw = EDGE_CASES[name]
    chains, seed, sigsq = (2 if name.startswith("instance") else 3), 41, 0.8
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
        o = sdo.DynRegOracle(oracle, T, obs, blocks, seed, c)
        inc = np.flatnonzero(gam[c])
        o.impute_state(y - X[:, inc] @ beta[c][inc], sigsq)
        worst = max(worst, check_state_models(eng, o, c, (name, c)))
    print("%s: state draw, worst error / max |state| %.3e" % (name, worst))


# ---- 4. whole rounds ---------------------------------------------------------------------------------------
@gpu
def test_whole_rounds_match_restatement(oracle):
    c = sdc.loop_case()
    T, X, y, obs, blocks, rounds = c["T"], c["X"], c["y"], c["obs"], c["blocks"], c["rounds"]

    def fresh():
        e = engine(c["chains"], c["seed"], y, X, obs, blocks, c["g0"])
        e.set_state(c["g0"], c["b0"], c["sig0"])
        return e

    eng = fresh()
    ora = {ch: sdo.DynRegOracle(oracle, T, obs, blocks, c["seed"], ch) for ch in c["check"]}
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
            check_state_models(eng, o, ch, (ch, r))
            # the regression's statistics of the device's own state draw
            Zs = np.array([o.S.Z(t) @ s for t, s in enumerate(eng.ss_get_state_draw(ch))])
            e = np.where(ob, y - Zs, 0.0)
            suf = eng.ss_get_chain_suf(ch)
            assert close(suf["yty"], e @ e) and np.max(np.abs(suf["xty"] - X.T @ e)) < RTOL * np.abs(X.T @ e).max(), (ch, r)
            assert suf["n"] == ob.sum()
        record.append(dict(states=(gam.copy(), beta.copy(), sig.copy()), path=eng.ss_get_state_draw(0),
                           var=[eng.ss_get_state_model(0, k, suf=False)["variances"] for k in range(len(blocks))]))
    for o in ora.values():
        assert o.margin > 1e-9
    final = [[eng.ss_get_state_model(ch, k) for k in range(len(blocks))] for ch in range(c["chains"])]
    # one call of 12 rounds
    eng2 = fresh()
    eng2.ss_sweep(rounds)
    for u, v in zip(eng.get_states(), eng2.get_states()):
        assert np.array_equal(u, v)
    for ch in range(c["chains"]):
        assert np.array_equal(eng.ss_get_state_draw(ch), eng2.ss_get_state_draw(ch))
        for k in range(len(blocks)):
            v = eng2.ss_get_state_model(ch, k)
            assert all(np.array_equal(final[ch][k][key], v[key]) for key in v), (ch, k)
    # ... and the same 12 draws handed out under a look-ahead of 4: the snapshot needs nothing new (the
    # variances sit in the state models' slots, the predictors are one table for every draw)
    eng3 = fresh()
    eng3.ss_set_lookahead(4)
    for r in range(rounds):
        eng3.ss_draw_next()
        for u, v in zip(record[r]["states"], eng3.get_states()):
            assert np.array_equal(u, v), r
        assert np.array_equal(record[r]["path"], eng3.ss_get_state_draw(0)), r
        for k in range(len(blocks)):
            assert np.array_equal(record[r]["var"][k], eng3.ss_get_state_model(0, k, suf=False)["variances"]), (r, k)
    for k in range(len(blocks)):
        v = eng3.ss_get_state_model(0, k)
        assert all(np.array_equal(final[0][k][key], v[key]) for key in v), k


# ---- 5. distribution -----------------------------------------------------------------------------------------
@gpu
def test_state_draws_have_the_dense_posterior_moments():
    """level + dynamic regression d = 2 at T = 30, variances fixed: 90 means and 4095 covariances"""
    T, chains, sigsq = 30, 4096, 0.6
    X, y, obs = sdc.data(T, seasonal=(), missing=(7,))
    sdy = float(np.std(y, ddof=1))
    blocks = general_spec(y, [("level",)]) + [sdo.dynreg_block(sdc.predictors(T, 2, 38, hard=T), sdy, [0.6, 0.4])]
    g0 = np.zeros(sdc.P, np.uint8)
    eng = engine(chains, 20265, y, X, obs, blocks, g0)
    eng.set_state(g0, np.zeros(sdc.P), sigsq)
    eng.ss_impute_state()
    draws = np.stack([eng.ss_get_state_draw(c).reshape(-1) for c in range(chains)])
    S = sdo.Structure(blocks)
    var = [b["initial_sigma"] ** 2 for b in blocks]
    mean, cov = sho.dense_posterior(S, var, y, obs.astype(bool), np.full(T, sigsq))
    d = len(mean)
    bound = sso.bonferroni_bound(d + d * (d + 1) // 2)   # (level 1e-3, fixed with the seed before any run)
    zm, zc = sso.moment_z(draws, mean, cov)
    print("largest |z|: mean %.3f covariance %.3f, bound %.3f" % (np.abs(zm).max(), np.abs(zc).max(), bound))
    assert np.abs(zm).max() < bound
    assert np.abs(zc).max() < bound


# ---- 6. forecast -----------------------------------------------------------------------------------------------
def swept_engine(chains=4, seed=53, sweeps=3):
    T = 70
    X, y, obs = sdc.data(T)
    blocks = sdc.list_small(y, T)
    blocks[2]["initial_sigma"] = np.array([0.3, 0.2, 0.5])
    g0 = np.zeros(sdc.P, np.uint8)
    g0[0] = 1
    eng = engine(chains, seed, y, X, obs, blocks, g0)
    eng.ss_sweep(sweeps)
    return eng, T, X, y, obs, blocks, seed


@gpu
def test_forecast_matches_restatement(oracle):
    """horizon 10: the predictors' rows T .. T + 9"""
    import boom_amd
    eng, T, X, y, obs, blocks, seed = swept_engine()
    rs = np.random.Generator(np.random.PCG64(9))
    newX = rs.standard_normal((sdc.HORIZON, sdc.P))
    fc = eng.ss_forecast(newX)
    gam, beta, sig = eng.get_states()
    for c in range(eng.chains):
        o = sdo.DynRegOracle(oracle, T, obs, blocks, seed, c)
        o.var = [eng.ss_get_state_model(c, k, suf=False)["variances"] for k in range(len(blocks))]
        want = o.forecast(eng.ss_get_state_draw(c)[-1], sig[c], newX @ (beta[c] * gam[c]))
        assert np.max(np.abs(fc[c] - want)) < 1e-8 * max(1.0, np.abs(want).max()), c
    with pytest.raises(boom_amd.BoomAmdError) as e:
        eng.ss_forecast(np.zeros((sdc.HORIZON + 1, sdc.P)))
    assert "the predictors of state model 2 have 80 rows: a forecast of horizon 11 needs 81" in str(e.value), str(e.value)
    # ... and served once the rows are there (add_forecast_data)
    x = blocks[2]["predictors"]
    eng.ss_set_dynamic_predictors(2, np.vstack([x, x[:1]]))
    assert eng.ss_forecast(np.zeros((sdc.HORIZON + 1, sdc.P))).shape == (eng.chains, sdc.HORIZON + 1)


# ---- 7. prediction errors ----------------------------------------------------------------------------------------
@gpu
def test_prediction_errors_match_restatement(oracle):
    eng, T, X, y, obs, blocks, seed = swept_engine(seed=54)
    full = eng.ss_prediction_errors(variances=True, log_likelihood=True)
    std = eng.ss_prediction_errors(standardize=True)
    S = sdo.Structure(blocks)
    gam, beta, sig = eng.get_states()
    worst = {}
    for c in range(eng.chains):
        var = [eng.ss_get_state_model(c, k, suf=False)["variances"] for k in range(len(blocks))]
        ref, gate = sho.reference_and_gate(S, var, sig[c], y, X, gam[c], beta[c], obs)
        dev = per.device_deviation(ref, full["errors"][c], full["variances"][c], std[c], full["log_likelihood"][c])
        assert np.all(full["errors"][c][obs == 0] == 0)
        for k, v in dev.items():
            r = v / gate["v" if k == "std" else k]
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= 1.0, (c, k, v, gate)
    print("worst device / gate  v %.3f  std %.3f  F %.3f  loglik %.3f" % (worst["v"], worst["std"], worst["F"], worst["loglik"]))


# ---- 8. interface ------------------------------------------------------------------------------------------------
@gpu
def test_refusals_and_their_texts():
    import boom_amd
    T = 30
    X, y, obs = sdc.data(T, seasonal=(), missing=())
    sdy = float(np.std(y, ddof=1))
    x = sdc.predictors(T, 2, 39)
    g0 = np.zeros(sdc.P, np.uint8)

    def blocks(pred=x, **kw):
        return general_spec(y, [("level",)]) + [dict(sdo.dynreg_block(pred, sdy), **kw)]

    eng = boom_amd.Engine(2, seed=1)
    eng.ss_set_data(y, X, None)
    # the arguments
    bad = x.copy()
    bad[3, 1] = np.inf
    refused(lambda: eng.ss_set_state_models(blocks(bad)), "the predictors of a dynamic regression must be finite")
    bad[3, 1] = np.nan
    refused(lambda: eng.ss_set_state_models(blocks(bad)), "the predictors of a dynamic regression must be finite")
    refused(lambda: eng.ss_set_state_models(blocks(P0=np.array([1.0, 0.0]))), "initial state variances must be positive")
    refused(lambda: eng.ss_set_state_models(blocks(sigma_upper_limit=np.array([1.0, -1.0]))), "sigma_max must be non-negative.")
    refused(lambda: eng.ss_set_state_models([sdo.dynreg_block(np.ones((T, 17)), sdy)]), "more than 16 variance parameters")
    refused(lambda: eng.ss_set_state_models(general_spec(y, [("seasonal", 60, 1)]) + [sdo.dynreg_block(np.ones((T, 6)), sdy)]),
            "state dimension exceeds 64")
    # a numeric kind 12 goes to ba_ss_add_state_model and is refused as any unknown kind
    refused(lambda: eng.ss_set_state_models([dict(general_spec(y, [("level",)])[0], kind=12)]),
            "10 (random-walk holiday) or 11 (calendar seasonal)")
    # predictors on a block that is none, a block index out of range
    eng.ss_set_state_models(blocks())
    refused(lambda: eng.ss_set_dynamic_predictors(0, x[:, :1]), "not a dynamic regression state model")
    refused(lambda: eng.ss_get_dynamic_predictors(0), "not a dynamic regression state model")
    eng._blocks.append(dict(kind="dynamic_regression", nvar=2, lags=0))
    refused(lambda: eng.ss_set_dynamic_predictors(2, x), "state model index out of range")
    eng._blocks.pop()
    refused(lambda: eng.ss_set_dynamic_predictors(1, bad), "the predictors of a dynamic regression must be finite")
    assert np.array_equal(eng.ss_get_dynamic_predictors(1), x)
    # too few rows: every call that launches
    eng = engine(2, 1, y, X, None, blocks(x[:T - 1]), g0)
    for fn in (lambda: eng.ss_sweep(1), eng.ss_impute_state, eng.ss_draw_next, eng.ss_prediction_errors):
        refused(fn, "the predictors of state model 1 have 29 rows, the series has 30 time points")
    eng.ss_set_dynamic_predictors(1, x)
    eng.ss_sweep(2)
    sm = eng.ss_get_state_model(0, 1)
    assert np.array_equal(sm["suf_n"], [T - 1, T - 1]) and np.all(sm["suf_ss"] > 0) and len(sm["variances"]) == 2
    refused(lambda: eng.ss_forecast(np.zeros((1, sdc.P))), "a forecast of horizon 1 needs 31")
    # under a look-ahead the setter is a mutator: the draws after it are those of a run without the look-ahead
    eng.ss_set_lookahead(4)
    eng.ss_draw_next()
    eng.ss_set_dynamic_predictors(1, np.vstack([x, x[:2]]))
    eng.ss_draw_next()
    plain = engine(2, 1, y, X, None, blocks(), g0)
    plain.ss_sweep(4)
    for u, v in zip(eng.get_states(), plain.get_states()):
        assert np.array_equal(u, v)
    assert eng.ss_forecast(np.zeros((2, sdc.P))).shape == (2, 2)
    # the other observation families: the block added on such data ...
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
    import student_trend_cases as stc
    dyn = blocks()[1:]
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


# ---- 9. the pybind class -------------------------------------------------------------------------------------------
@gpu
def test_pybind_class_agrees_with_the_c_abi():
    """boom.DynamicRegressionStateModel(predictors) in a StateSpaceRegressionModel: three rounds at the
    facade's default look-ahead == the engine's plain loop through the C-ABI on the same seed, bit for bit"""
    import boom_amd
    import boom_amd._boom as boom
    T, chains, seed = 70, 3, 23
    X, y, obs = sdc.data(T)
    blocks = sdc.loop_case()["blocks"]   # level + 4 seasons + d = 3
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
    b = blocks[2]
    dyn = boom.DynamicRegressionStateModel(b["predictors"])
    assert dyn.state_dimension == 3 and np.array_equal(dyn.predictors, b["predictors"])
    dyn.set_sigsq(b["initial_sigma"] ** 2)
    for i in range(3):
        dyn.set_prior(i, b["df"][i], b["sigma_guess"][i], b["sigma_upper_limit"][i])
    dyn.set_initial_state_mean(b["a0"])
    dyn.set_initial_state_variance(b["P0"])
    for s in (level, seas, dyn):
        model.add_state(s)
    sampler = boom.StateSpacePosteriorSampler(model, boom.MvnGivenScalarSigma(prior["b"], prior["ominv"]),
                                              boom.ChisqModel(prior["df"], prior["sigma_guess"]),
                                              boom.VariableSelectionPrior(prior["pi"]), sig_up)
    model.set_method(sampler)
    assert model.state_dimension == 7
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_set_data(y, X, obs)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"], sigma_upper_limit=sig_up)
    eng.ss_set_state_models(blocks)
    eng.set_state(np.zeros(sdc.P, np.uint8))
    for _ in range(3):
        model.sample_posterior()
        eng.ss_sweep(1)
    for u, v in zip(model.chain_states(), eng.get_states()):
        assert np.array_equal(u, v)
    for c in range(chains):
        sm = eng.ss_get_state_model(c, 2)
        assert np.array_equal(model.state_variances(c)[2:5], sm["variances"])
        assert np.array_equal(model.state(c), eng.ss_get_state_draw(c).T)
