"""The regression holiday state model on the device (ba_ss_add_regression_holiday, bsts AddRegressionHoliday):
an offset on every chain's observation series (the general structural kernel reads the series through a
stride), rh_draw_kernel and rh_observe_kernel (reg_holiday_kernel.hip), forecast and prediction errors.

  1 twin identity  an engine with the models and coefficients set against an engine without them on
                   y - effect, one impute_state: state draw, block statistics, xty, yty, nobs bit for bit --
                   PLAIN on SMALL and LDC 33, HD beside a random-walk holiday, DR beside a dynamic regression,
                   QT beside a Student trend; once more with different coefficients on every chain
  2 totals         the device's totals against a long-double recomputation from the device's own state draw
  3 draw           one ba_ss_sweep(1) from known totals against the restatement (tests/ss_regholiday_oracle.py)
  4 whole rounds   12 x ba_ss_sweep(1) against the restatement given the device's regression draws;
                   ba_ss_sweep(12) the same bits; a call whose chains outgrow the launch capacity and are
                   caught up the same bits
  5 forecast and prediction errors against the twin's, bit for bit; a short calendar is refused
  6 interface      refusals and texts in both orders, round trips, the list reset, the pybind class
"""
import numpy as np
import pytest

import ss_dynreg_cases as sdc
import ss_dynreg_oracle as sdo
import ss_holiday_oracle as sho
import ss_regholiday_cases as src
import ss_regholiday_oracle as sro
import student_trend_cases as stc
from cases import bsts_priors, general_data, general_spec
from ss_gpu_helpers import refused

gpu = pytest.mark.gpu
CHAINS = 4


def engine(chains, seed, y, X, obs, blocks, g0, kernel=None, model_size=2):
    import boom_amd
    prior, _, sig_up = bsts_priors(X, y, model_size)
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_set_data(y, X, obs)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"],
                   sigma_upper_limit=sig_up)
    eng.ss_set_state_models(blocks)
    if kernel is not None:
        eng.ss_set_tuning(kernel=kernel)
    eng.set_state(g0)
    return eng


def same_draw(a, ca, b, cb, nb, tag):
    """chain ca of engine a and chain cb of engine b: state draw, block statistics, xty, yty, nobs as bits"""
    u, v = a.ss_get_state_draw(ca), b.ss_get_state_draw(cb)
    assert np.abs(v).max() > 0
    assert np.array_equal(u, v), tag + (np.max(np.abs(u - v)),)
    for k in range(nb):
        su, sv = a.ss_get_state_model(ca, k), b.ss_get_state_model(cb, k)
        for key in sv:
            assert np.array_equal(su[key], sv[key]), tag + (k, key)
    su, sv = a.ss_get_chain_suf(ca), b.ss_get_chain_suf(cb)
    assert su["yty"] == sv["yty"] and su["n"] == sv["n"] and np.array_equal(su["xty"], sv["xty"]), tag


# ---- 1. the twin identity ----------------------------------------------------------------------------------
def variant_list(name, y, T):
    sdy = float(np.std(y, ddof=1))
    if name == "PLAIN, SMALL":
        return src.list_small(y)
    if name == "PLAIN, LDC 33":
        return src.list_ldc33(y)
    if name == "HD":
        cal = np.full(T + src.HORIZON, -1, np.int32)
        cal[5:7], cal[63:65] = (0, 1), (0, 1)   # (its own windows; 63, 64 beside both regression holiday models)
        return general_spec(y, [("level",)]) + [sho.holiday_block(2, cal, sdy)]
    if name == "DR":
        return general_spec(y, [("level",)]) + [sdo.dynreg_block(sdc.predictors(T + src.HORIZON, 2, 51, hard=T), sdy, [0.3, 0.5])]
    assert name == "QT"
    return stc.student_trend_spec(y, [("student_trend",), ("seasonal", 4, 1)])


VARIANTS = [("PLAIN, SMALL", 70), ("PLAIN, SMALL", 130), ("PLAIN, LDC 33", 70), ("HD", 70), ("DR", 70), ("QT", 130)]


@gpu
@pytest.mark.parametrize("name,T", VARIANTS)
def test_twin_identity_bit_for_bit(name, T):
    """engine A: the list + two regression holiday models, coefficients by ba_ss_set_regression_holiday;
    engine B: the list alone on y - effect (numpy, the same successive subtraction), on the general kernel as
    A is -- A is asked for the shape-specialised kernel, which must not be taken"""
    seed, sigsq = 61, 0.7
    X, y, obs = src.data(T, seasonal=((20, 1),) if "33" in name else ((4, 1),))
    base = variant_list(name, y, T)
    models = src.models(T, coefficients=(np.zeros(6), np.zeros(4)))
    gam, beta = src.chain_parameters(CHAINS, 5)
    a = engine(CHAINS, seed, y, X, obs, base + models, gam[0], kernel=3)
    for k in range(2):
        a.ss_set_regression_holiday(-1, k, src.COEFS[k])
    b = engine(CHAINS, seed, sro.offset_series(y, models, src.COEFS), X, obs, base, gam[0], kernel=0)
    for c in range(CHAINS):
        a.set_state(gam[c], beta[c], sigsq, chain=c)
        b.set_state(gam[c], beta[c], sigsq, chain=c)
    a.ss_impute_state()
    b.ss_impute_state()
    for c in range(CHAINS):
        same_draw(a, c, b, c, len(base), (name, T, c))
        got = a.ss_get_regression_holiday(c, 0)
        assert np.array_equal(got["coefficients"], src.COEFS[0])


@gpu
def test_twin_identity_with_every_chain_its_own_coefficients():
    """chain c of A against chain c of a twin built for chain c: a kernel that read one chain's series for
    all would pass the test above"""
    T, seed, sigsq = 70, 62, 0.7
    X, y, obs = src.data(T)
    base = src.list_small(y)
    models = src.models(T)
    coefs = src.chain_coefficients(CHAINS)
    gam, beta = src.chain_parameters(CHAINS, 6)
    a = engine(CHAINS, seed, y, X, obs, base + models, gam[0])
    for c in range(CHAINS):
        a.set_state(gam[c], beta[c], sigsq, chain=c)
        for k in range(2):
            a.ss_set_regression_holiday(c, k, coefs[c][k])
    a.ss_impute_state()
    for c in range(CHAINS):
        b = engine(CHAINS, seed, sro.offset_series(y, models, coefs[c]), X, obs, base, gam[0], kernel=0)
        b.set_state(gam[c], beta[c], sigsq, chain=c)
        b.ss_impute_state()
        same_draw(a, c, b, c, len(base), (c,))


# ---- 2. the totals -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("T,big", [(70, False), (130, False), (130, True)])
def test_totals_match_long_double_recomputation(T, big):
    """after one impute_state: total[j] = sum over the coefficient's observed steps of ((y_c - Z'alpha) -
    x'beta) + coefficient, recomputed in numpy.longdouble from the device's state draw, beta and
    coefficients.  Gate: 1e-10 x the sum over those steps of |y| + |x|'|beta| + |Z|'|alpha| + |effect| -- four
    orders above the rounding bound (p + m + 4) 2^-53 at these shapes, far below what a wrong step, sign
    or beta moves.  Worst ratio seen on an MI355X: see DESIGN.md 3.25."""
    seed, sigsq = 63, 0.9
    X, y, obs = src.data(T, seasonal=((20, 1),) if big else ((4, 1),))
    base = src.list_ldc33(y) if big else src.list_small(y)
    models = src.models(T)
    coefs = src.chain_coefficients(CHAINS, seed=19)
    gam, beta = src.chain_parameters(CHAINS, 7)
    a = engine(CHAINS, seed, y, X, obs, base + models, gam[0])
    for c in range(CHAINS):
        a.set_state(gam[c], beta[c], sigsq, chain=c)
        for k in range(2):
            a.ss_set_regression_holiday(c, k, coefs[c][k])
    a.ss_impute_state()
    S = sho.Structure(base)
    want_counts = src.expected_counts(T)
    worst = 0.0
    for c in range(CHAINS):
        st = a.ss_get_state_draw(c)
        Z = np.array([S.Z(t) for t in range(T)])
        zalpha = np.array([np.sum(Z[t].astype(np.longdouble) * st[t].astype(np.longdouble)) for t in range(T)])
        xbeta = np.array([np.sum(X[t].astype(np.longdouble) * beta[c].astype(np.longdouble)) for t in range(T)])
        want = sro.observe(models, coefs[c], y, xbeta, zalpha, obs, dtype=np.longdouble)
        for k, m in enumerate(models):
            got = a.ss_get_regression_holiday(c, k)
            assert np.array_equal(got["counts"], want_counts[k]), (c, k, got["counts"])
            assert np.array_equal(got["counts"], sro.counts(models, obs, T)[k])
            scale = np.zeros(sro.ncoef(m))
            for t in range(T):
                j = m["calendar"][t]
                if j >= 0 and obs[t]:
                    eff = sum(abs(e) for e in sro.effects(models, coefs[c], t) if e is not None)
                    scale[j] += abs(y[t]) + np.abs(X[t]) @ np.abs(beta[c]) + np.abs(Z[t]) @ np.abs(st[t]) + eff
            err = np.abs(got["totals"].astype(np.longdouble) - want[k]).astype(float)
            assert np.all(got["totals"][want_counts[k] == 0] == 0.0)
            live = scale > 0
            assert live.sum() == (want_counts[k] > 0).sum()
            ratio = float(np.max(err[live] / (1e-10 * scale[live])))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (c, k, err, scale)
    print("T = %d, m = %d: totals, worst error / gate %.3e" % (T, S.m, worst))


# ---- 3. the draw ---------------------------------------------------------------------------------------------
@gpu
def test_coefficient_draw_matches_restatement(oracle):
    """ba_ss_impute_state leaves totals; ba_ss_sweep(1) then draws the regression, then every coefficient from
    those totals with the sigma^2 just drawn.  Gate 1e-8 (|mean| + sd) per coefficient, the relative gate of
    test_ss_holiday_gpu.py and test_ss_dynreg_gpu.py; a count of 0 is the prior's draw; the second sweep's
    draws continue the stream where the restatement's generator stands."""
    import ctypes as C
    T, seed = 70, 64
    X, y, obs = src.data(T)
    base = src.list_small(y)
    models = src.models(T)
    g0 = np.zeros(src.P, np.uint8)
    g0[0] = 1
    a = engine(CHAINS, seed, y, X, obs, base + models, g0)
    a.set_state(g0, np.zeros(src.P), 0.8)
    a.ss_impute_state()
    cnts = src.expected_counts(T)
    rngs = [oracle.rng_philox(seed, c, sro.STREAM, 0) for c in range(CHAINS)]
    oracle.lib.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    oracle.lib.bo_rnorm.restype = C.c_double
    worst = 0.0
    for sweep in range(2):
        totals = [[a.ss_get_regression_holiday(c, k)["totals"] for k in range(2)] for c in range(CHAINS)]
        assert any(np.abs(t).max() > 0 for row in totals for t in row)
        a.ss_sweep(1)
        sig = a.get_states()[2]
        for c in range(CHAINS):
            for k, m in enumerate(models):
                got = a.ss_get_regression_holiday(c, k)["coefficients"]
                mu, tau = m["prior"]
                for j in range(sro.ncoef(m)):
                    mean, sd = sro.posterior(totals[c][k][j], cnts[k][j], sig[c], mu, tau)
                    before = rngs[c].pos
                    want = oracle.lib.bo_rnorm(C.byref(rngs[c]), float(mean), float(sd))
                    assert rngs[c].pos > before
                    ratio = abs(got[j] - want) / (1e-8 * (abs(mean) + sd))
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (sweep, c, k, j, got[j], want)
                    if cnts[k][j] == 0:
                        z = (want - mean) / sd
                        assert abs(mean - mu) <= 1e-15 * abs(mu) and abs(sd - tau) <= 1e-15 * tau
                        assert abs(got[j] - (mu + tau * z)) <= 1e-8 * (abs(mu) + tau), (sweep, c, k, j)
    print("coefficient draws, worst error / gate %.3e" % worst)


# ---- 4. whole rounds -----------------------------------------------------------------------------------------
@gpu
def test_whole_rounds_match_restatement(oracle):
    """12 x ba_ss_sweep(1) against the restatement fed the device's regression draws: the coefficients use the
    sigma^2 of this round and totals formed with the beta of the round before; ba_ss_sweep(12) gives the same bits"""
    T, seed, rounds, sig0 = 70, 65, 12, 0.7
    X, y, obs = src.data(T)
    base = src.list_small(y)
    models = src.models(T)
    g0 = np.zeros(src.P, np.uint8)
    g0[0] = 1
    b0 = np.zeros(src.P)

    def fresh():
        e = engine(CHAINS, seed, y, X, obs, base + models, g0)
        e.set_state(g0, b0, sig0)
        return e

    eng = fresh()
    check = (0, 3)
    ora = {c: sro.RegHolidayOracle(oracle, sho.HolidayOracle(oracle, T, obs, base, seed, c), models, y, X, seed, c) for c in check}
    for o in ora.values():
        o.impute_state(b0, sig0)   # the first call's impute_state, with the parameters as they stand
    worst = 0.0
    for r in range(rounds):
        eng.ss_sweep(1)
        gam, beta, sig = eng.get_states()
        for c, o in ora.items():
            st = o.round(beta[c] * gam[c], sig[c])
            dev = eng.ss_get_state_draw(c)
            assert np.max(np.abs(dev - st)) < 1e-8 * np.abs(st).max(), (c, r)
            for k, m in enumerate(models):
                got = eng.ss_get_regression_holiday(c, k)
                mu, tau = m["prior"]
                assert np.all(np.abs(got["coefficients"] - o.coefs[k]) <= 1e-8 * (np.abs(o.coefs[k]) + tau)), (c, r, k)
                scale = np.abs(o.totals[k]) + o.counts[k] * (np.abs(y).max() + np.abs(st).max())
                assert np.all(np.abs(got["totals"] - o.totals[k]) <= 1e-8 * scale), (c, r, k, got["totals"], o.totals[k])
            for k in range(len(base)):
                sm = eng.ss_get_state_model(c, k)
                assert np.all(np.abs(sm["variances"] - o.base.var[k]) <= 1e-8 * o.base.var[k]), (c, r, k)
    for o in ora.values():
        assert o.base.margin > 1e-9
    eng2 = fresh()
    eng2.ss_sweep(rounds)
    for u, v in zip(eng.get_states(), eng2.get_states()):
        assert np.array_equal(u, v)
    for c in range(CHAINS):
        assert np.array_equal(eng.ss_get_state_draw(c), eng2.ss_get_state_draw(c))
        for k in range(2):
            u, v = eng.ss_get_regression_holiday(c, k), eng2.ss_get_regression_holiday(c, k)
            assert all(np.array_equal(u[key], v[key]) for key in v), (c, k)


@gpu
def test_catch_up_of_parked_chains_gives_the_same_bits():
    """20 signals among 24 regressors from the empty model: inside ba_ss_sweep(12) chains outgrow the launch
    capacity of 16, sit the rest of the call out and are caught up one (sweep, state draw) pair at a time --
    the coefficient draw and observe_state with them; round by round nothing is parked for longer than a round"""
    T, p, seed, rounds = 70, 24, 66, 12
    X, y, _, _ = general_data(T, p, 20, [(4, 1)], seed=7)
    obs = np.ones(T, np.uint8)
    obs[[12, 62]] = 0
    base = src.list_small(y)
    models = src.models(T)
    g0 = np.zeros(p, np.uint8)

    def fresh():
        return engine(CHAINS, seed, y, X, obs, base + models, g0, model_size=20)

    a, b = fresh(), fresh()
    a.ss_sweep(rounds)
    for _ in range(rounds):
        b.ss_sweep(1)
    assert a.get_states()[0].sum(1).max() > 16
    for u, v in zip(a.get_states(), b.get_states()):
        assert np.array_equal(u, v)
    for c in range(CHAINS):
        assert np.array_equal(a.ss_get_state_draw(c), b.ss_get_state_draw(c))
        for k in range(2):
            u, v = a.ss_get_regression_holiday(c, k), b.ss_get_regression_holiday(c, k)
            assert all(np.array_equal(u[key], v[key]) for key in v), (c, k)


# ---- 5. forecast and prediction errors -------------------------------------------------------------------------
@gpu
def test_forecast_and_prediction_errors_equal_the_twins():
    import boom_amd
    T, seed, sigsq = 70, 67, 0.7
    X, y, obs = src.data(T)
    base = src.list_small(y)
    models = src.models(T)
    coefs = src.chain_coefficients(CHAINS, seed=23)
    gam, beta = src.chain_parameters(CHAINS, 9)
    rs = np.random.Generator(np.random.PCG64(10))
    newX = rs.standard_normal((src.HORIZON, src.P))
    a = engine(CHAINS, seed, y, X, obs, base + models, gam[0])
    for c in range(CHAINS):
        a.set_state(gam[c], beta[c], sigsq, chain=c)
        for k in range(2):
            a.ss_set_regression_holiday(c, k, coefs[c][k])
    a.ss_impute_state()
    fa = a.ss_forecast(newX)
    ea = a.ss_prediction_errors(variances=True, log_likelihood=True)
    for c in range(CHAINS):
        b = engine(CHAINS, seed, sro.offset_series(y, models, coefs[c]), X, obs, base, gam[0], kernel=0)
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
    b = engine(CHAINS, seed, sro.offset_series(y, models, coefs[1]), X, obs, base, gam[0], kernel=0)
    b.set_state(gam[0], beta[0], sigsq, chain=0)
    b.ss_impute_state()
    assert np.array_equal(a.ss_prediction_errors(chains=(0, 1))[0], b.ss_prediction_errors(chains=(0, 1))[0])
    with pytest.raises(boom_amd.BoomAmdError) as e:
        a.ss_forecast(np.zeros((src.HORIZON + 1, src.P)))
    assert "the calendar of regression holiday model 0 has 80 entries: a forecast of horizon 11 needs 81 (the series' 70 and the horizon)" in str(e.value), str(e.value)


# ---- 6. interface --------------------------------------------------------------------------------------------
@gpu
def test_refusals_round_trips_and_the_list_reset():
    import boom_amd
    T = 30
    X, y, _, _ = general_data(T, src.P, 2, [], seed=3)
    level = general_spec(y, [("level",)])
    cal = np.full(T, -1, np.int32)
    cal[[3, 4, 10]] = (0, 1, 0)
    g0 = np.zeros(src.P, np.uint8)

    def model(**kw):
        return dict(sro.reg_holiday_model((2,), (0.0, 1.0), cal), **kw)

    eng = boom_amd.Engine(2, seed=1)
    eng.ss_set_data(y, X, None)
    # the arguments
    refused(lambda: eng.ss_set_state_models([model()]), "a regression holiday model goes on a list of state models: add a state model first")
    refused(lambda: eng.ss_set_state_models(level + [model(widths=[2, 0])]), "a holiday's width must be at least 1")
    refused(lambda: eng.ss_set_state_models(level + [model(prior=(0.0, 0.0))]), "the prior standard deviation must be positive and finite")
    refused(lambda: eng.ss_set_state_models(level + [model(prior=(0.0, np.inf))]), "the prior standard deviation must be positive and finite")
    refused(lambda: eng.ss_set_state_models(level + [model()] * 5), "more than 4 regression holiday models")
    wide = dict(sro.reg_holiday_model((200,), (0.0, 1.0), cal), calendar=None)
    refused(lambda: eng.ss_set_state_models(level + [wide, wide]), "more than 256 regression holiday coefficients")
    bad = cal.copy()
    bad[7] = 2
    refused(lambda: eng.ss_set_state_models(level + [model(calendar=bad)]),
            "regression holiday calendar entry 7 is 2: it must be -1 (inactive) or a coefficient index in [0, 2)")
    bad[7] = -2
    refused(lambda: eng.ss_set_state_models(level + [model(calendar=bad)]), "regression holiday calendar entry 7 is -2")
    # the model is no block: the state dimension and the list's blocks do not count it
    eng.ss_set_state_models(level + [model(coefficients=[0.5, -0.25])])
    assert eng._ssm_dim == 1 and len(eng._blocks) == 1
    refused(lambda: eng.ss_set_regression_holiday_calendar(1, cal), "regression holiday model index out of range")
    refused(lambda: eng.ss_get_regression_holiday_calendar(1), "regression holiday model index out of range")
    assert np.array_equal(eng.ss_get_regression_holiday_calendar(0), cal)
    # no calendar, a calendar shorter than the series: every call that launches
    eng = engine(2, 1, y, X, None, level + [model(calendar=None, coefficients=[0.5, -0.25])], g0)
    for fn in (lambda: eng.ss_sweep(1), eng.ss_impute_state, eng.ss_draw_next, eng.ss_prediction_errors):
        refused(fn, "regression holiday model 0 has no calendar: call ba_ss_set_regression_holiday_calendar first")
    eng.ss_set_regression_holiday_calendar(0, cal[:T - 1])
    for fn in (lambda: eng.ss_sweep(1), eng.ss_impute_state, eng.ss_draw_next, eng.ss_prediction_errors):
        refused(fn, "the calendar of regression holiday model 0 has 29 entries, the series has 30 time points")
    eng.ss_set_regression_holiday_calendar(0, cal)
    # getters and setters round-trip; before the first state draw the totals are empty
    got = eng.ss_get_regression_holiday(1, 0)
    assert np.array_equal(got["coefficients"], [0.5, -0.25]) and np.array_equal(got["totals"], [0, 0])
    assert np.array_equal(got["counts"], [2, 1])
    eng.ss_set_regression_holiday(1, 0, [1.5, 2.5])
    assert np.array_equal(eng.ss_get_regression_holiday(1, 0)["coefficients"], [1.5, 2.5])
    assert np.array_equal(eng.ss_get_regression_holiday(0, 0)["coefficients"], [0.5, -0.25])
    eng.ss_set_regression_holiday(-1, 0, [3.0, 4.0])
    assert all(np.array_equal(eng.ss_get_regression_holiday(c, 0)["coefficients"], [3.0, 4.0]) for c in range(2))
    refused(lambda: eng.ss_set_regression_holiday(0, 0, [np.nan, 0.0]), "the coefficients must be finite")
    refused(lambda: eng.ss_get_regression_holiday(2, 0), "chain index out of range")
    eng.ss_sweep(2)
    assert np.all(eng.ss_get_regression_holiday(0, 0)["totals"] != 0)
    refused(lambda: eng.ss_forecast(np.zeros((1, src.P))), "a forecast of horizon 1 needs 31")
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
    # the list reset drops the models
    eng.ss_set_state_models(level)
    refused(lambda: eng.ss_get_regression_holiday_calendar(0), "regression holiday model index out of range")
    eng._rh_ncoef = [2]
    refused(lambda: eng.ss_get_regression_holiday(0, 0), "the list of state models holds no regression holiday model")
    # ... and the list runs as one that never had them: on the shared series, so with the template kernel's
    # draws (both engines below have the same history up to the reset)
    twins = []
    for with_model in (True, False):
        e6 = engine(2, 1, y, X, None, level + ([model()] if with_model else []), g0)
        e6.ss_set_state_models(level)
        e6.ss_sweep(1)
        twins.append(e6.ss_get_state_draw(0))
    assert np.array_equal(twins[0], twins[1])
    # the other observation families: the model added on such data ...
    text = "the regression holiday is built for the Gaussian observation model only (not the Student-t, Poisson and logit families)"
    from ss_family_cases import count_series, golden_mix
    Xc, counts, exposure, _ = count_series(T, src.P, 4)
    families = [
        (lambda e: e.ss_student_set_data(y, X, None), lambda e: e.ss_student_sweep(1), True),
        (lambda e: e.ss_poisson_set_data(counts, exposure, Xc, golden_mix(), None), lambda e: e.ss_poisson_sweep(1), False),
        (lambda e: e.ss_logit_set_data(np.minimum(counts, 3.0), np.full(T, 3.0), Xc), lambda e: e.ss_logit_sweep(1), False),
    ]
    for set_data, sweep, scales in families:
        e2 = boom_amd.Engine(2, seed=1)
        set_data(e2)
        refused(lambda: e2.ss_set_state_models(level + [model()]), text)
        # ... and the list first, the family's data and first call after it
        e3 = boom_amd.Engine(2, seed=1)
        e3.ss_set_data(y, X, None)
        e3.ss_set_state_models(level + [model()])
        set_data(e3)
        e3.sss_set_slab(np.zeros(src.P), 0.1 * np.eye(src.P), scales_with_sigsq=scales)
        e3.set_spike(np.full(src.P, 0.5))
        if scales:
            e3.set_sigma_prior(1.0, 1.0)
        e3.set_state(g0)
        refused(lambda: sweep(e3), text)


@gpu
def test_pybind_class_agrees_with_the_c_abi():
    """boom.RegressionHolidayStateModel(widths, prior_mean, prior_sd) with set_calendar in a
    StateSpaceRegressionModel: three rounds at the facade's default look-ahead (which it turns off for this
    model, as for the Student trend) == the engine's plain loop through the C-ABI on the same seed, bit for bit"""
    import boom_amd
    import boom_amd._boom as boom
    T, chains, seed = 70, 3, 24
    X, y, obs = src.data(T)
    base = src.list_small(y)
    models = src.models(T)
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
    for m in models:
        rh = boom.RegressionHolidayStateModel(m["widths"], m["prior"][0], m["prior"][1])
        assert rh.number_of_coefficients == sro.ncoef(m)
        rh.set_calendar(list(m["calendar"]))
        rh.set_coefficients(m["coefficients"])
        model.add_state(rh)
    sampler = boom.StateSpacePosteriorSampler(model, boom.MvnGivenScalarSigma(prior["b"], prior["ominv"]),
                                              boom.ChisqModel(prior["df"], prior["sigma_guess"]),
                                              boom.VariableSelectionPrior(prior["pi"]), sig_up)
    model.set_method(sampler)
    assert model.state_dimension == 4
    eng = engine(chains, seed, y, X, obs, base + models, np.zeros(src.P, np.uint8))
    for _ in range(3):
        model.sample_posterior()
        eng.ss_sweep(1)
    for u, v in zip(model.chain_states(), eng.get_states()):
        assert np.array_equal(u, v)
    for c in range(chains):
        assert np.array_equal(model.state(c), eng.ss_get_state_draw(c).T)
        for k in range(2):
            assert np.array_equal(model.regression_holiday_coefficients(c, k), eng.ss_get_regression_holiday(c, k)["coefficients"])
