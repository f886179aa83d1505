"""The hierarchical regression holiday state model on the device through the C-ABI
(ba_ss_add_hierarchical_regression_holiday, bsts AddHierarchicalRegressionHoliday): to the state space model an
offset on every chain's series as the plain model (reg_holiday_kernel.hip), with its own sampler,
rhh_draw_kernel (hier_holiday_kernel.hip).  T = 70 and 130, 4 chains, p = 3; the calendars are
ss_hier_regholiday_cases'.

  1 twin identity  an engine with the model (coefficients set, read back) against an engine without it on
                   y - effect, one impute_state: state draw, block statistics, xty, yty, nobs bit for bit -- on a
                   PLAIN and an HD list, and with a plain and a hierarchical model on one list in both orders
  2 rounds         12 x ba_ss_sweep(1): every round's draw against the restatement
                   (tests/ss_hier_regholiday_oracle.py) given the device's sigma^2, totals, mu and Omega, on one
                   generator that runs through all 12 rounds (the first sweep from known totals, the second
                   continues the stream, ...), within the probe test's gate; ba_ss_sweep(12) the same bits;
                   a call whose chains are parked and caught up the same bits
  3 forecast and prediction errors equal the twin's, bit for bit; after a setter the series is not stale
  4 interface      getters and setters (chain = -1), every new refusal with its text in both orders where the
                   order matters, the capi block kind (every engine here is built from it), the pybind class
"""
import numpy as np
import pytest

import ss_hier_regholiday_cases as hrc
import ss_hier_regholiday_oracle as hro
import ss_holiday_oracle as sho
import ss_regholiday_cases as src
import ss_regholiday_oracle as sro
from cases import bsts_priors, general_data, general_spec
from test_ss_regholiday_gpu import engine, refused, same_draw

gpu = pytest.mark.gpu
CHAINS = 4


def effects_off(y, models, coefs):
    return sro.offset_series(y, models, coefs)


# ---- 1. the twin identity ----------------------------------------------------------------------------------
def base_list(name, y, T):
    if name == "HD":
        cal = np.full(T + hrc.HORIZON, -1, np.int32)
        cal[5:7], cal[63:65] = (0, 1), (0, 1)   # (63, 64: beside the hierarchical model's holiday 0)
        return general_spec(y, [("level",)]) + [sho.holiday_block(2, cal, float(np.std(y, ddof=1)))]
    return src.list_small(y)


TWINS = [("PLAIN", 70, "h"), ("PLAIN", 130, "h"), ("HD", 70, "h"), ("PLAIN", 70, "hp"), ("PLAIN", 130, "ph")]


@gpu
@pytest.mark.parametrize("name,T,order", TWINS)
def test_twin_identity_bit_for_bit(name, T, order):
    """order: "h" the hierarchical model alone, "hp" / "ph" a hierarchical and a plain model on one list; the
    coefficients go in through ba_ss_set_regression_holiday on all chains and are read back"""
    seed, sigsq = 71, 0.7
    X, y, obs = hrc.data(T)
    base = base_list(name, y, T)
    models, coefs = [], []
    for ch in order:
        models.append(hrc.hier(T, np.zeros(6)) if ch == "h" else hrc.plain(T, np.zeros(4)))
        coefs.append(hrc.COEFS if ch == "h" else src.COEFS[1])
    gam, beta = src.chain_parameters(CHAINS, 5)
    a = engine(CHAINS, seed, y, X, obs, base + models, gam[0], kernel=3)
    for k, c in enumerate(coefs):
        a.ss_set_regression_holiday(-1, k, c)
    b = engine(CHAINS, seed, effects_off(y, models, coefs), X, obs, base, gam[0], kernel=0)
    for c in range(CHAINS):
        a.set_state(gam[c], beta[c], sigsq, chain=c)
        b.set_state(gam[c], beta[c], sigsq, chain=c)
    a.ss_impute_state()
    b.ss_impute_state()
    for c in range(CHAINS):
        same_draw(a, c, b, c, len(base), (name, T, order, c))
        for k, want in enumerate(coefs):
            got = a.ss_get_regression_holiday(c, k)
            assert np.array_equal(got["coefficients"], want)
            if order[k] == "h":
                assert np.array_equal(got["counts"], hrc.expected_counts(T)), got["counts"]
                assert np.all(got["totals"][got["counts"] == 0] == 0.0) and np.all(got["totals"][got["counts"] > 0] != 0.0)


# ---- 2. rounds ---------------------------------------------------------------------------------------------
def fresh(T, seed, models, g0, sig0=0.7, p=hrc.P, X=None, y=None, obs=None, **kw):
    if X is None:
        X, y, obs = hrc.data(T)
    e = engine(CHAINS, seed, y, X, obs, src.list_small(y) + models, g0, **kw)
    e.set_state(g0, np.zeros(len(g0)), sig0)
    return e


@gpu
@pytest.mark.parametrize("order", ["h", "ph"])
def test_twelve_rounds_match_restatement(oracle, order):
    """every round: the device's totals, mu and Omega before ba_ss_sweep(1) and its sigma^2 after it go into the
    restatement, whose generator is never re-seeded: round r's draw starts where round r - 1's ended.  Gate: the
    probe test's, 4 |float64 - long double| + 8 ulp of the output's largest magnitude.  Then ba_ss_sweep(12) on a
    fresh engine: the same bits."""
    T, seed, rounds = 70, 72, 12
    models = [hrc.plain(T)] * (order == "ph") + [hrc.hier(T)]
    k = len(models) - 1
    g0 = np.zeros(hrc.P, np.uint8)
    g0[0] = 1
    eng = fresh(T, seed, models, g0)
    eng.ss_impute_state()
    src_rng = [hro.PhiloxDraws(oracle, seed, c) for c in range(CHAINS)]
    assert np.array_equal(eng.ss_get_hierarchical_regression_holiday(0, k)["mean"], np.zeros(hrc.D))
    assert np.array_equal(eng.ss_get_hierarchical_regression_holiday(0, k)["precision"], np.eye(hrc.D))
    worst = 0.0
    for r in range(rounds):
        before = [(eng.ss_get_regression_holiday(c, k), eng.ss_get_hierarchical_regression_holiday(c, k)) for c in range(CHAINS)]
        assert all(np.abs(b[0]["totals"]).max() > 0 for b in before)
        eng.ss_sweep(1)
        sig = eng.get_states()[2]
        for c in range(CHAINS):
            rh, hy = before[c]
            lo, hi = hro.draw_both(models[k], sig[c], rh["totals"], rh["counts"], hy["mean"], hy["precision"], src_rng[c])
            got_h = eng.ss_get_hierarchical_regression_holiday(c, k)
            got = dict(beta=eng.ss_get_regression_holiday(c, k)["coefficients"].reshape(hrc.H, hrc.D), mu=got_h["mean"],
                       omega=got_h["precision"])
            for key in ("mu", "omega"):
                ratio = float(np.max(np.abs(got[key] - lo[key]) / hro.gate(lo[key], hi[key], float(np.max(np.abs(lo[key]))))))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (r, c, key, got[key], lo[key])
            for h in range(hrc.H):
                g = hro.gate(lo["beta"][h], hi["beta"][h], float(np.max(np.abs(lo["beta"][h]))))
                ratio = float(np.max(np.abs(got["beta"][h] - lo["beta"][h]) / g))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (r, c, h, got["beta"][h], lo["beta"][h])
    print("12 rounds (%s): worst error / gate %.3e" % (order, worst))
    eng2 = fresh(T, seed, models, g0)
    eng2.ss_sweep(rounds)
    # (eng made one impute_state more, before its first sweep: the state stream is one draw ahead, so the twelve
    # are compared on engines with the same history)
    eng3 = fresh(T, seed, models, g0)
    for _ in range(rounds):
        eng3.ss_sweep(1)
    same_engines(eng2, eng3, len(models))


def same_engines(a, b, nmodels):
    for u, v in zip(a.get_states(), b.get_states()):
        assert np.array_equal(u, v)
    for c in range(CHAINS):
        assert np.array_equal(a.ss_get_state_draw(c), b.ss_get_state_draw(c))
        for k in range(nmodels):
            u, v = a.ss_get_regression_holiday(c, k), b.ss_get_regression_holiday(c, k)
            assert all(np.array_equal(u[key], v[key]) for key in v), (c, k)
    u, v = a.ss_get_hierarchical_regression_holiday(CHAINS - 1, nmodels - 1), b.ss_get_hierarchical_regression_holiday(CHAINS - 1, nmodels - 1)
    assert all(np.array_equal(u[key], v[key]) for key in v) and not np.array_equal(u["precision"], np.eye(hrc.D))


@gpu
def test_catch_up_of_parked_chains_gives_the_same_bits():
    """the plain test's arrangement, 20 signals among 24 regressors from the empty model: inside ba_ss_sweep(12)
    chains outgrow the launch capacity of 16, sit the rest of the call out and are caught up one (sweep, state
    draw) pair at a time -- rhh_draw_kernel with them.  (The seed is one at which a chain passes 16 variables in
    the fifth round and stays there; the assertion below holds the arrangement to that.)"""
    T, p, seed, rounds = 70, 24, 65, 12
    X, y, _, _ = general_data(T, p, 20, [(4, 1)], seed=7)
    obs = np.ones(T, np.uint8)
    obs[list(hrc.MISSING)] = 0
    models = [hrc.plain(T), hrc.hier(T)]
    g0 = np.zeros(p, np.uint8)
    a = fresh(T, seed, models, g0, X=X, y=y, obs=obs, model_size=20)
    b = fresh(T, seed, models, g0, X=X, y=y, obs=obs, model_size=20)
    a.ss_sweep(rounds)
    for _ in range(rounds):
        b.ss_sweep(1)
    assert a.get_states()[0].sum(1).max() > 16
    same_engines(a, b, 2)


# ---- 3. forecast and prediction errors ---------------------------------------------------------------------------
@gpu
def test_forecast_and_prediction_errors_equal_the_twins():
    T, seed, sigsq = 70, 74, 0.7
    X, y, obs = hrc.data(T)
    base = src.list_small(y)
    models = [hrc.hier(T), hrc.plain(T)]
    rs = np.random.Generator(np.random.PCG64(10))
    coefs = [[np.round(rs.standard_normal(6) * 64) / 64, np.round(rs.standard_normal(4) * 64) / 64] for _ in range(CHAINS)]
    gam, beta = src.chain_parameters(CHAINS, 9)
    newX = rs.standard_normal((hrc.HORIZON, hrc.P))
    a = engine(CHAINS, seed, y, X, obs, base + models, gam[0])
    for c in range(CHAINS):
        a.set_state(gam[c], beta[c], sigsq, chain=c)
        for k in range(2):
            a.ss_set_regression_holiday(c, k, coefs[c][k])
    a.ss_impute_state()
    fa = a.ss_forecast(newX)
    ea = a.ss_prediction_errors(variances=True, log_likelihood=True)
    for c in range(CHAINS):
        b = engine(CHAINS, seed, effects_off(y, models, coefs[c]), X, obs, base, gam[0], kernel=0)
        b.set_state(gam[c], beta[c], sigsq, chain=c)
        b.ss_impute_state()
        fb = b.ss_forecast(newX)[c]
        want = sro.forecast_offset(fb, models, coefs[c], T)
        assert not np.array_equal(want, fb)
        assert np.array_equal(fa[c], want), (c, fa[c] - want)
        eb = b.ss_prediction_errors(variances=True, log_likelihood=True)
        for key in ("errors", "variances", "log_likelihood"):
            assert np.array_equal(ea[key][c], eb[key][c]), (c, key)
    # a setter alone: the prediction errors read the series of the coefficients as they are now
    a.ss_set_regression_holiday(0, 0, coefs[1][0])
    a.ss_set_regression_holiday(0, 1, coefs[1][1])
    b = engine(CHAINS, seed, effects_off(y, models, coefs[1]), X, obs, base, gam[0], kernel=0)
    b.set_state(gam[0], beta[0], sigsq, chain=0)
    b.ss_impute_state()
    assert np.array_equal(a.ss_prediction_errors(chains=(0, 1))[0], b.ss_prediction_errors(chains=(0, 1))[0])


# ---- 4. interface --------------------------------------------------------------------------------------------
@gpu
def test_getters_setters_and_refusals():
    import boom_amd
    T = 30
    X, y, _, _ = general_data(T, hrc.P, 2, [], seed=3)
    level = general_spec(y, [("level",)])
    cal = np.full(T, -1, np.int32)
    cal[[3, 4, 10, 11]] = (0, 1, 2, 3)
    g0 = np.zeros(hrc.P, np.uint8)
    I2 = np.eye(2)

    def model(**kw):
        return dict(hro.hier_model(2, 2, (np.zeros(2), I2), (I2, 3.0), cal), **kw)

    eng = boom_amd.Engine(2, seed=1)
    eng.ss_set_data(y, X, None)
    # the arguments
    refused(lambda: eng.ss_set_state_models([model()]), "a regression holiday model goes on a list of state models: add a state model first")
    refused(lambda: eng.ss_set_state_models(level + [model(nholidays=0, calendar=None, coefficients=None)]), "a regression holiday model needs at least one holiday")
    wide = dict(hro.hier_model(1, 17, (np.zeros(17), np.eye(17)), (np.eye(17), 20.0), None))
    refused(lambda: eng.ss_set_state_models(level + [wide]), "the holidays of a hierarchical regression holiday model are at most 16 days wide")
    text = "the variance guess weight must exceed the holidays' width less 1 (the Wishart prior's degrees of freedom)"
    refused(lambda: eng.ss_set_state_models(level + [model(variance_prior=(I2, 1.0))]), text)
    refused(lambda: eng.ss_set_state_models(level + [model(variance_prior=(I2, 0.5))]), text)
    refused(lambda: eng.ss_set_state_models(level + [model(variance_prior=(I2, np.inf))]), "the variance guess weight must be finite")
    notpd, skew, nonfin = np.array([[1.0, 2.0], [2.0, 1.0]]), np.array([[2.0, 0.5], [0.25, 2.0]]), np.array([[np.nan, 0.0], [0.0, 1.0]])
    for bad in (notpd, skew):
        refused(lambda: eng.ss_set_state_models(level + [model(mean_prior=(np.zeros(2), bad))]),
                "the prior variance of the holidays' mean must be symmetric and positive definite")
        refused(lambda: eng.ss_set_state_models(level + [model(variance_prior=(bad, 3.0))]),
                "the variance guess must be symmetric and positive definite")
    refused(lambda: eng.ss_set_state_models(level + [model(mean_prior=(np.zeros(2), nonfin))]),
            "the prior variance of the holidays' mean and the variance guess must be finite")
    refused(lambda: eng.ss_set_state_models(level + [model(mean_prior=(np.array([0.0, np.inf]), I2))]),
            "the prior mean of the holidays' mean must be finite")
    refused(lambda: eng.ss_set_state_models(level + [model(coefficients=np.array([0.0, np.nan, 0.0, 0.0]))]), "the initial coefficients must be finite")
    refused(lambda: eng.ss_set_state_models(level + [model()] * 5), "more than 4 regression holiday models")
    big = dict(hro.hier_model(16, 16, (np.zeros(16), np.eye(16)), (np.eye(16), 17.0), None))
    eng.ss_set_state_models(level + [big])   # (256 coefficients: the limit itself)
    refused(lambda: eng.ss_set_state_models(level + [big, model()]), "more than 256 regression holiday coefficients")
    bad = cal.copy()
    bad[7] = 4
    refused(lambda: eng.ss_set_state_models(level + [model(calendar=bad)]),
            "regression holiday calendar entry 7 is 4: it must be -1 (inactive) or a coefficient index in [0, 4)")
    # the model is no block; no calendar, a short calendar: every call that launches (the plain model's rows)
    eng = engine(2, 1, y, X, None, level + [model(calendar=None, coefficients=[0.5, -0.25, 1.0, 2.0])], g0)
    assert eng._ssm_dim == 1 and len(eng._blocks) == 1
    for fn in (lambda: eng.ss_sweep(1), eng.ss_impute_state, eng.ss_draw_next, eng.ss_prediction_errors):
        refused(fn, "regression holiday model 0 has no calendar: call ba_ss_set_regression_holiday_calendar first")
    eng.ss_set_regression_holiday_calendar(0, cal)
    assert np.array_equal(eng.ss_get_regression_holiday_calendar(0), cal)
    # getters and setters
    got = eng.ss_get_hierarchical_regression_holiday(1, 0)
    assert np.array_equal(got["mean"], [0.0, 0.0]) and np.array_equal(got["precision"], I2)
    assert np.array_equal(eng.ss_get_regression_holiday(1, 0)["coefficients"], [0.5, -0.25, 1.0, 2.0])
    assert np.array_equal(eng.ss_get_regression_holiday(1, 0)["counts"], [1, 1, 1, 1])
    prec = np.array([[2.0, 0.5], [0.5, 1.0]])
    eng.ss_set_hierarchical_regression_holiday(1, 0, [1.5, -2.5], prec)
    got = eng.ss_get_hierarchical_regression_holiday(1, 0)
    assert np.array_equal(got["mean"], [1.5, -2.5]) and np.array_equal(got["precision"], prec)
    assert np.array_equal(eng.ss_get_hierarchical_regression_holiday(0, 0)["precision"], I2)
    eng.ss_set_hierarchical_regression_holiday(-1, 0, [3.0, 4.0], 2 * prec)
    for c in range(2):
        got = eng.ss_get_hierarchical_regression_holiday(c, 0)
        assert np.array_equal(got["mean"], [3.0, 4.0]) and np.array_equal(got["precision"], 2 * prec)
    refused(lambda: eng.ss_set_hierarchical_regression_holiday(0, 0, [0.0, 0.0], notpd), "the precision must be symmetric and positive definite")
    refused(lambda: eng.ss_set_hierarchical_regression_holiday(0, 0, [0.0, 0.0], skew), "the precision must be symmetric and positive definite")
    refused(lambda: eng.ss_set_hierarchical_regression_holiday(0, 0, [0.0, 0.0], nonfin), "the precision must be finite")
    refused(lambda: eng.ss_set_hierarchical_regression_holiday(0, 0, [np.nan, 0.0], prec), "the mean must be finite")
    refused(lambda: eng.ss_get_hierarchical_regression_holiday(2, 0), "chain index out of range")
    refused(lambda: eng.ss_get_hierarchical_regression_holiday(0, 1), "regression holiday model index out of range")
    eng.ss_sweep(2)
    got = eng.ss_get_hierarchical_regression_holiday(0, 0)
    assert not np.array_equal(got["mean"], [3.0, 4.0]) and np.array_equal(got["precision"], got["precision"].T)
    assert np.all(np.linalg.eigvalsh(got["precision"]) > 0)
    # a plain model is not a hierarchical one
    e4 = engine(2, 1, y, X, None, level + [sro.reg_holiday_model((2, 2), (0.0, 1.0), cal), model()], g0)
    refused(lambda: e4.ss_get_hierarchical_regression_holiday(0, 0), "not a hierarchical regression holiday model")
    e4._rhh_width[0] = 2
    refused(lambda: e4.ss_set_hierarchical_regression_holiday(0, 0, [0.0, 0.0], I2), "not a hierarchical regression holiday model")
    assert np.array_equal(e4.ss_get_hierarchical_regression_holiday(0, 1)["precision"], I2)
    # a look-ahead above 1, in both orders
    text = "the look-ahead does not carry a regression holiday's coefficients: use a look-ahead of 1"
    refused(lambda: eng.ss_set_lookahead(4), text)
    eng.ss_set_lookahead(1)
    eng.ss_draw_next()
    e5 = boom_amd.Engine(2, seed=1)
    e5.ss_set_data(y, X, None)
    e5.ss_set_lookahead(4)
    prior, _, sig_up = bsts_priors(X, y, 2)
    e5.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"], sigma_upper_limit=sig_up)
    e5.ss_set_state_models(level + [model()])
    e5.set_state(g0)
    refused(e5.ss_draw_next, text)
    # the other observation families, in both orders
    text = "the regression holiday is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)"
    e2 = boom_amd.Engine(2, seed=1)
    e2.ss_student_set_data(y, X, None)
    refused(lambda: e2.ss_set_state_models(level + [model()]), text)
    e3 = boom_amd.Engine(2, seed=1)
    e3.ss_set_data(y, X, None)
    e3.ss_set_state_models(level + [model()])
    e3.ss_student_set_data(y, X, None)
    e3.sss_set_slab(np.zeros(hrc.P), 0.1 * np.eye(hrc.P), scales_with_sigsq=True)
    e3.set_spike(np.full(hrc.P, 0.5))
    e3.set_sigma_prior(1.0, 1.0)
    e3.set_state(g0)
    refused(lambda: e3.ss_student_sweep(1), text)
    # the list reset drops the model
    eng.ss_set_state_models(level)
    refused(lambda: eng.ss_get_regression_holiday_calendar(0), "regression holiday model index out of range")


@gpu
def test_pybind_class_agrees_with_the_c_abi():
    """boom.HierarchicalRegressionHolidayStateModel in a StateSpaceRegressionModel beside a plain model: three rounds
    at the facade's default look-ahead (which it turns off for this model) == the engine's plain loop through the
    C-ABI on the same seed, bit for bit; holiday_mean / holiday_precision read the chain's mu and Omega"""
    import boom_amd._boom as boom
    T, chains, seed = 70, 3, 25
    X, y, obs = hrc.data(T)
    base = src.list_small(y)
    models = [hrc.hier(T), hrc.plain(T)]
    prior, _, sig_up = bsts_priors(X, y, 2)
    model = boom.StateSpaceRegressionModel(y, X, [bool(o) for o in obs], chains=chains, seed=seed)
    b = base[0]
    level = boom.LocalLevelStateModel(float(b["initial_sigma"][0]))
    level.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    level.set_initial_state_mean(float(b["a0"][0]))
    level.set_initial_state_variance(float(b["P0"][0]))
    b = base[1]
    seas = boom.SeasonalStateModel(4)
    seas.set_sigsq(b["initial_sigma"][0] ** 2)
    seas.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    seas.set_initial_state_mean(b["a0"])
    seas.set_initial_state_variance(b["P0"][0])
    model.add_state(level)
    model.add_state(seas)
    m = models[0]
    hh = boom.HierarchicalRegressionHolidayStateModel(m["nholidays"], m["width"], m["mean_prior"][0], m["mean_prior"][1],
                                                      m["variance_prior"][0], m["variance_prior"][1])
    assert hh.number_of_coefficients == 6
    hh.set_calendar(list(m["calendar"]))
    hh.set_coefficients(m["coefficients"])
    model.add_state(hh)
    m = models[1]
    rh = boom.RegressionHolidayStateModel(m["widths"], m["prior"][0], m["prior"][1])
    rh.set_calendar(list(m["calendar"]))
    rh.set_coefficients(m["coefficients"])
    model.add_state(rh)
    sampler = boom.StateSpacePosteriorSampler(model, boom.MvnGivenScalarSigma(prior["b"], prior["ominv"]),
                                              boom.ChisqModel(prior["df"], prior["sigma_guess"]),
                                              boom.VariableSelectionPrior(prior["pi"]), sig_up)
    model.set_method(sampler)
    assert model.state_dimension == 4
    eng = engine(chains, seed, y, X, obs, base + models, np.zeros(hrc.P, np.uint8))
    for _ in range(3):
        model.sample_posterior()
        eng.ss_sweep(1)
    for u, v in zip(model.chain_states(), eng.get_states()):
        assert np.array_equal(u, v)
    for c in range(chains):
        assert np.array_equal(model.state(c), eng.ss_get_state_draw(c).T)
        for k in range(2):
            assert np.array_equal(model.regression_holiday_coefficients(c, k), eng.ss_get_regression_holiday(c, k)["coefficients"])
        got = eng.ss_get_hierarchical_regression_holiday(c, 0)
        assert np.array_equal(hh.holiday_mean(c), got["mean"]) and np.array_equal(hh.holiday_precision(c), got["precision"])
        assert not np.array_equal(got["precision"], np.eye(2))
