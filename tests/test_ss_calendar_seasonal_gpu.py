"""The calendar seasonal state model on the device (ba_ss_add_state_model kind 11; bsts
AddMonthlyAnnualCycle is the one of 12 seasons that start on the first day of a month): a seasonal
block whose season starts are read from a table, served by the calendar instances of the general
structural kernel.

  identity      a regular calendar (t % d == ph) against the seasonal of that duration and phase on the
                general kernel: the state draw, the statistics, the variances after a round and every
                stream position, bit for bit; SMALL, LDC 33 and GLOB instances
  table edges   one impute_state against the restatement (tests/ss_calendar_seasonal_oracle.py):
                consecutive starts at the first step, at both edges of the kernel's 64-step time blocks
                and at T - 1 (the cursor wraps), month starts, a calendar without a start, a block of
                one component; missing observations; SMALL, LDC 33 and GLOB instances; a random-walk
                holiday beside the block (both tables live)
  whole rounds  ba_ss_sweep(1) x 12 against the restatement given the device's regression draw;
                ba_ss_sweep(12) and ba_ss_draw_next under a look-ahead of 4 the same draws, bit for bit
  distribution  4096 chains' state draws against the dense Gaussian posterior
  forecast      horizon 40 across a start inside the horizon; a horizon past the calendar is refused
  errors        ba_ss_prediction_errors, live and from the look-ahead's record, against the
                restatement's long-double filter and its own gate
  interface     refusals and their texts, the getter, the "monthly" block of capi and the pybind class
"""
import numpy as np
import pytest

import prediction_errors_ref as per
import ss_calendar_seasonal_cases as scc
import ss_calendar_seasonal_oracle as sco
import ss_holiday_oracle as sho
import ss_student_oracle as sso
from cases import bsts_priors, general_spec
from test_ss_holiday_gpu import check_state_models, close, engine, refused

gpu = pytest.mark.gpu


def set_chains(eng, gam, beta, sigsq):
    for c in range(eng.chains):
        eng.set_state(gam[c], beta[c], sigsq, chain=c)


# ---- 1. identity with the seasonal ---------------------------------------------------------------------
IDENTITY = [("small", 70, 4, 7, 1), ("small", 130, 12, 3, 0), ("ldc33", 70, 4, 3, 2), ("ldc33", 130, 4, 7, 6),
            ("glob", 70, 4, 1, 0), ("glob", 130, 12, 7, 0)]


@gpu
@pytest.mark.parametrize("shape,T,nseasons,duration,phase", IDENTITY)
def test_regular_calendar_equals_the_seasonal_bit_for_bit(shape, T, nseasons, duration, phase):
    chains, seed, sigsq = 4, 77, 0.5
    X, y, obs = scc.data(T, trig=[(12.0, [1.0, 2.0])] if shape == "glob" else None)
    cal, seas = scc.regular_pair(y, T, nseasons, duration, phase, shape)
    gam, beta = scc.chain_parameters(chains, 3)
    a = engine(chains, seed, y, X, obs, cal, gam[0])
    b = engine(chains, seed, y, X, obs, seas, gam[0], kernel=0)
    for e in (a, b):
        set_chains(e, gam, beta, sigsq)
        e.ss_impute_state()
    for c in range(chains):
        assert np.array_equal(a.ss_get_state_draw(c), b.ss_get_state_draw(c)), c
        for k in range(len(cal)):
            su, sv = a.ss_get_state_model(c, k), b.ss_get_state_model(c, k)
            assert all(np.array_equal(su[key], sv[key]) for key in sv), (c, k)
    # a whole round each: the variance draws (their sampler ids and positions), the regression, the next state draw
    for e in (a, b):
        e.ss_sweep(1)
    for u, v in zip(a.get_states(), b.get_states()):
        assert np.array_equal(u, v)
    for c in range(chains):
        assert np.array_equal(a.ss_get_state_draw(c), b.ss_get_state_draw(c)), c
        for k in range(len(cal)):
            su, sv = a.ss_get_state_model(c, k), b.ss_get_state_model(c, k)
            assert all(np.array_equal(su[key], sv[key]) for key in sv), (c, k)
    # every stream stands where the seasonal's does (the engine hands out no positions: what is read
    # next shows them): two more rounds -- the state stream, the variance samplers', the regression's --
    # and a forecast draw the same numbers
    newX = np.random.Generator(np.random.PCG64(4)).standard_normal((1, scc.P))
    for e in (a, b):
        e.ss_sweep(2)
    assert np.array_equal(a.ss_forecast(newX), b.ss_forecast(newX))
    for u, v in zip(a.get_states(), b.get_states()):
        assert np.array_equal(u, v)
    for c in range(chains):
        assert np.array_equal(a.ss_get_state_draw(c), b.ss_get_state_draw(c)), c


# ---- 2. one impute_state against the restatement -----------------------------------------------------------
EDGE_CASES = [(name, shape, T) for name in scc.CALENDARS for shape in scc.SHAPES for T in (70, 130)]
EDGE_CASES += [("edges", "holiday", 70), ("months", "holiday", 130)]


@gpu
@pytest.mark.parametrize("name,shape,T", EDGE_CASES)
def test_impute_state_matches_restatement(oracle, name, shape, T):
    chains, seed, sigsq = 2, 41, 0.8
    X, y, obs = scc.data(T, trig=[(12.0, [1.0, 2.0])] if shape == "glob" else None)
    blocks = scc.calendar_list(y, T, name, shape)
    gam, beta = scc.chain_parameters(chains, 8)
    eng = engine(chains, seed, y, X, obs, blocks, gam[0])
    set_chains(eng, gam, beta, sigsq)
    eng.ss_impute_state()
    worst = 0.0
    kb = [b["kind"] for b in blocks].index(sco.CALENDAR_SEASONAL)
    for c in range(chains):
        o = sco.CalendarOracle(oracle, T, obs, blocks, seed, c)
        inc = np.flatnonzero(gam[c])
        o.impute_state(y - X[:, inc] @ beta[c][inc], sigsq)
        worst = max(worst, check_state_models(eng, o, c, (name, shape, T, c)))
        if name == "never":
            # n = 0; the block is a constant; (no seasonal normal: the draw matches a restatement that reads none)
            st = eng.ss_get_state_draw(c)
            f, n = int(o.S.first[kb]), blocks[kb]["dim"]
            assert eng.ss_get_state_model(c, kb)["suf_n"][0] == 0
            assert np.all(st[:, f:f + n] == st[0, f:f + n])
    print("%s / %s / T=%d: state draw, worst error / max |state| %.3e" % (name, shape, T, worst))


@gpu
def test_never_started_block_draws_its_variance_from_the_prior(oracle):
    T, chains, seed = 70, 2, 43
    X, y, obs = scc.data(T)
    blocks = scc.calendar_list(y, T, "never", "small")
    g0 = np.zeros(scc.P, np.uint8)
    eng = engine(chains, seed, y, X, obs, blocks, g0)
    eng.set_state(g0, np.zeros(scc.P), 0.7)
    eng.ss_sweep(1)
    b = blocks[1]
    df, guess, smax = b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0]
    for c in range(chains):
        rng = oracle.rng_philox(seed, c, 7, 0)
        prior_draw = 1.0 / oracle.trun_gammas(rng, df / 2, df * guess * guess / 2, 1.0 / (smax * smax), 1)[0]
        assert close(eng.ss_get_state_model(c, 1)["variances"][0], prior_draw), c


# ---- 3. whole rounds ---------------------------------------------------------------------------------------
@gpu
def test_whole_rounds_match_restatement(oracle):
    c = scc.loop_case()
    T, X, y, obs, blocks, rounds = c["T"], c["X"], c["y"], c["obs"], c["blocks"], c["rounds"]

    def fresh():
        e = engine(c["chains"], c["seed"], y, X, obs, blocks, c["g0"])
        e.set_state(c["g0"], c["b0"], c["sig0"])
        return e

    eng = fresh()
    ora = {ch: sco.CalendarOracle(oracle, T, obs, blocks, c["seed"], ch) for ch in c["check"]}
    for o in ora.values():
        o.impute_state(y - X @ c["b0"], c["sig0"])
    record = []
    for r in range(rounds):
        eng.ss_sweep(1)
        gam, beta, sig = eng.get_states()
        for ch, o in ora.items():
            o.draw_state_models()
            o.impute_state(y - X @ (beta[ch] * gam[ch]), sig[ch])
            check_state_models(eng, o, ch, (ch, r))
        record.append(dict(states=(gam.copy(), beta.copy(), sig.copy()), path=eng.ss_get_state_draw(0),
                           var=[eng.ss_get_state_model(0, k, suf=False)["variances"] for k in range(len(blocks))]))
    for o in ora.values():
        assert o.margin > 1e-9
    final = [[eng.ss_get_state_model(ch, k) for k in range(len(blocks))] for ch in range(c["chains"])]
    eng2 = fresh()
    eng2.ss_sweep(rounds)
    for u, v in zip(eng.get_states(), eng2.get_states()):
        assert np.array_equal(u, v)
    for ch in range(c["chains"]):
        assert np.array_equal(eng.ss_get_state_draw(ch), eng2.ss_get_state_draw(ch))
        for k in range(len(blocks)):
            v = eng2.ss_get_state_model(ch, k)
            assert all(np.array_equal(final[ch][k][key], v[key]) for key in v), (ch, k)
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


# ---- 4. distribution -----------------------------------------------------------------------------------------
@gpu
def test_state_draws_have_the_dense_posterior_moments():
    """the edges pattern cut to T = 30, variances fixed (the seed: test_ss_calendar_seasonal_cpu.py runs the
    restatement's own 4096 draws against the same bound)"""
    c = scc.dense_case()
    T, y, X, obs, blocks = c["T"], c["y"], c["X"], c["obs"], c["blocks"]
    g0 = np.zeros(scc.P, np.uint8)
    eng = engine(c["chains"], c["seed"], y, X, obs, blocks, g0)
    eng.set_state(g0, np.zeros(scc.P), c["sigsq"])
    eng.ss_impute_state()
    draws = np.stack([eng.ss_get_state_draw(ch).reshape(-1) for ch in range(c["chains"])])
    S = sco.Structure(blocks)
    var = [b["initial_sigma"] ** 2 for b in blocks]
    mean, cov = sho.dense_posterior(S, var, y, obs.astype(bool), np.full(T, c["sigsq"]))
    d = len(mean)
    bound = sso.bonferroni_bound(d + d * (d + 1) // 2)   # (level 1e-3, fixed with the seed before any run)
    zm, zc = sso.moment_z(draws, mean, cov)
    print("largest |z|: mean %.3f covariance %.3f, bound %.3f" % (np.abs(zm).max(), np.abs(zc).max(), bound))
    assert np.abs(zm).max() < bound
    assert np.abs(zc).max() < bound


# ---- 5. forecast -----------------------------------------------------------------------------------------------
def swept_engine(chains=4, seed=53, sweeps=3, extra=scc.HORIZON, lookahead=0):
    """level + 7 seasons + months, T = 130, `extra` calendar entries past T"""
    T = 130
    X, y, obs = scc.data(T)
    sdy = float(np.std(y, ddof=1))
    ns, cal = scc.calendar("months", T, extra)
    blocks = general_spec(y, [("level",), ("seasonal", 7, 1)]) + [sco.calendar_block(ns, cal, sdy)]
    g0 = np.zeros(scc.P, np.uint8)
    g0[0] = 1
    eng = engine(chains, seed, y, X, obs, blocks, g0)
    if lookahead:
        eng.ss_set_lookahead(lookahead)
        for _ in range(sweeps):
            eng.ss_draw_next()
    else:
        eng.ss_sweep(sweeps)
    return eng, T, X, y, obs, blocks, seed


@gpu
def test_forecast_matches_restatement(oracle):
    """horizon 40 from T = 130: the entries past T, with the July 1 start (t = 152) inside the horizon; the
    series itself crosses the June 1 start at t = 122"""
    eng, T, X, y, obs, blocks, seed = swept_engine()
    cal = blocks[2]["calendar"]
    assert list(np.flatnonzero(cal)) == [2, 30, 61, 91, 122, 152]
    newX = np.random.Generator(np.random.PCG64(9)).standard_normal((scc.HORIZON, scc.P))
    fc = eng.ss_forecast(newX)
    gam, beta, sig = eng.get_states()
    for c in range(eng.chains):
        o = sco.CalendarOracle(oracle, T, obs, blocks, seed, c)
        o.var = [eng.ss_get_state_model(c, k, suf=False)["variances"] for k in range(len(blocks))]
        want = o.forecast(eng.ss_get_state_draw(c)[-1], sig[c], newX @ (beta[c] * gam[c]))
        assert np.max(np.abs(fc[c] - want)) < 1e-8 * max(1.0, np.abs(want).max()), c
    eng.ss_set_season_calendar(2, cal[:T])
    refused(lambda: eng.ss_forecast(np.zeros((1, scc.P))), "a forecast of horizon 1 needs 131")


# ---- 6. prediction errors ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lookahead", [0, 4])
def test_prediction_errors_match_restatement(oracle, lookahead):
    """live, and (look-ahead 4) served from the record of the draw ba_ss_draw_next handed out"""
    eng, T, X, y, obs, blocks, seed = swept_engine(seed=54, extra=0, lookahead=lookahead)
    full = eng.ss_prediction_errors(variances=True, log_likelihood=True)
    std = eng.ss_prediction_errors(standardize=True)
    S = sco.Structure(blocks)
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
    print("look-ahead %d: worst device / gate  v %.3f  std %.3f  F %.3f  loglik %.3f"
          % (lookahead, worst["v"], worst["std"], worst["F"], worst["loglik"]))


# ---- 7. interface ------------------------------------------------------------------------------------------------
@gpu
def test_refusals_and_their_texts():
    import boom_amd
    T = 30
    X, y, obs = scc.data(T, missing=())
    sdy = float(np.std(y, ddof=1))
    _, cal = scc.calendar("edges", T)
    g0 = np.zeros(scc.P, np.uint8)

    def blocks(nseasons=4, calendar=cal):
        return general_spec(y, [("level",)]) + [sco.calendar_block(nseasons, calendar, sdy)]

    eng = boom_amd.Engine(2, seed=1)
    eng.ss_set_data(y, X, None)
    # nseasons, the state dimension, the number of blocks
    refused(lambda: eng.ss_set_state_models(blocks(1, None)), "nseasons must be at least 2")
    refused(lambda: eng.ss_set_state_models(blocks(65, None)), "state dimension exceeds 64")
    refused(lambda: eng.ss_set_state_models([sco.calendar_block(2, None, sdy) for _ in range(9)]), "more than 8 state models")
    refused(lambda: eng.ss_set_state_models([dict(blocks(4, None)[1], kind=12)]), "10 (random-walk holiday) or 11 (calendar seasonal)")
    # an entry that is neither 0 nor 1
    wrong = cal.copy()
    wrong[5] = 2
    refused(lambda: eng.ss_set_state_models(blocks(4, wrong)), "season calendar entry 5 is 2: it must be 0 or 1")
    # a calendar on a block of another kind; the holiday's setter on this one
    hol = sho.holiday_block(2, np.zeros(0, np.int32), sdy)
    hol["calendar"] = None
    eng.ss_set_state_models(blocks(4, None) + [hol])
    refused(lambda: eng.ss_set_season_calendar(0, cal), "not a calendar seasonal state model")
    refused(lambda: eng.ss_set_season_calendar(2, cal), "not a calendar seasonal state model")
    refused(lambda: eng.ss_get_season_calendar(2), "not a calendar seasonal state model")
    refused(lambda: eng.ss_set_holiday_calendar(1, np.zeros(T, np.int32)), "not a random-walk holiday state model")
    refused(lambda: eng.ss_set_season_calendar(3, cal), "state model index out of range")
    # no calendar, a short one: every call that launches
    eng = engine(2, 1, y, X, None, blocks(4, None), g0)
    assert eng.ss_get_season_calendar(1).size == 0
    for fn in (lambda: eng.ss_sweep(1), eng.ss_impute_state, eng.ss_draw_next, eng.ss_prediction_errors):
        refused(fn, "state model 1 is a calendar seasonal without a calendar: call ba_ss_set_season_calendar first")
    eng.ss_set_season_calendar(1, cal[:T - 1])
    for fn in (lambda: eng.ss_sweep(1), eng.ss_impute_state, eng.ss_draw_next, eng.ss_prediction_errors):
        refused(fn, "the season calendar of state model 1 has 29 entries, the series has 30 time points")
    eng.ss_set_season_calendar(1, cal)
    got = eng.ss_get_season_calendar(1)
    assert got.dtype == np.uint8 and np.array_equal(got, cal)
    eng.ss_sweep(2)
    sm = eng.ss_get_state_model(0, 1)
    assert sm["suf_n"][0] == 3 and sm["suf_ss"][0] > 0   # (starts at 1, 2, 3)
    m = eng.ss_get_state_draw(0).shape[1]
    assert m == 4
    refused(lambda: eng.ss_forecast(np.zeros((1, scc.P))), "a forecast of horizon 1 needs 31")
    # under a look-ahead the setter is a mutator: the draws after it are those of a run without the look-ahead
    eng.ss_set_lookahead(4)
    eng.ss_draw_next()
    eng.ss_set_season_calendar(1, np.concatenate([cal, [0, 1]]).astype(np.uint8))
    eng.ss_draw_next()
    plain = engine(2, 1, y, X, None, blocks(), g0)
    plain.ss_sweep(4)
    for u, v in zip(eng.get_states(), plain.get_states()):
        assert np.array_equal(u, v)
    assert eng.ss_forecast(np.zeros((2, scc.P))).shape == (2, 2)
    # the other observation families: the block added on such data ...
    text = "the calendar seasonal is built for the Gaussian observation model only"
    from ss_family_cases import count_series, golden_mix
    Xc, counts, exposure, _ = count_series(T, scc.P, 4)
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
        e3.sss_set_slab(np.zeros(scc.P), 0.1 * np.eye(scc.P), scales_with_sigsq=scales)
        e3.set_spike(np.full(scc.P, 0.5))
        if scales:
            e3.set_sigma_prior(1.0, 1.0)
        e3.set_state(g0)
        refused(lambda: sweep(e3), text)
    # a Student local linear trend in the same list, in both orders
    import student_trend_cases as stc
    text = "a list that holds both a calendar seasonal and a Student local linear trend is not built"
    st = stc.student_trend_spec(y, [("student_trend",)])
    e4 = boom_amd.Engine(2, seed=1)
    e4.ss_set_data(y, X, None)
    refused(lambda: e4.ss_set_state_models(st + blocks()[1:]), text)
    refused(lambda: e4.ss_set_state_models(blocks()[1:] + st), text)


@gpu
def test_monthly_block_and_pybind_class_draw_the_months_calendar_from_a_date():
    """capi's "monthly" block and boom.MonthlyAnnualCycle(2023, 1, 30) in a StateSpaceRegressionModel: three
    rounds == the engine with the months calendar given entry by entry, bit for bit"""
    import boom_amd
    import boom_amd._boom as boom
    T, chains, seed = 130, 3, 23
    X, y, obs = scc.data(T)
    sdy = float(np.std(y, ddof=1))
    ns, cal = scc.calendar("months", T)
    blocks = general_spec(y, [("level",)]) + [sco.calendar_block(ns, cal, sdy)]
    prior, _, sig_up = bsts_priors(X, y, 2)
    g0 = np.zeros(scc.P, np.uint8)
    eng = engine(chains, seed, y, X, obs, blocks, g0)
    by_date = dict(blocks[1], kind="monthly", first_date=scc.FIRST_DATE, calendar=None)
    del by_date["nseasons"]
    eng2 = engine(chains, seed, y, X, obs, [blocks[0], by_date], g0)
    assert np.array_equal(eng2.ss_get_season_calendar(1)[:T], cal) and eng2.ss_get_season_calendar(1).size == T + 366
    general = dict(blocks[1], kind="calendar_seasonal")
    eng3 = engine(chains, seed, y, X, obs, [blocks[0], general], g0)
    model = boom.StateSpaceRegressionModel(y, X, [bool(o) for o in obs], chains=chains, seed=seed)
    b = blocks[0]
    level = boom.LocalLevelStateModel(float(b["initial_sigma"][0]))
    level.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    level.set_initial_state_mean(float(b["a0"][0]))
    level.set_initial_state_variance(float(b["P0"][0]))
    b = blocks[1]
    mac = boom.MonthlyAnnualCycle(*scc.FIRST_DATE)
    assert mac.state_dimension == 11 and mac.nseasons == 12
    assert np.array_equal(np.asarray(mac.calendar(T))[:T], cal)
    mac.set_sigsq(b["initial_sigma"][0] ** 2)
    mac.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    mac.set_initial_state_mean(b["a0"])
    mac.set_initial_state_variance(b["P0"][0])
    model.add_state(level)
    model.add_state(mac)
    sampler = boom.StateSpacePosteriorSampler(model, boom.MvnGivenScalarSigma(prior["b"], prior["ominv"]),
                                              boom.ChisqModel(prior["df"], prior["sigma_guess"]),
                                              boom.VariableSelectionPrior(prior["pi"]), sig_up)
    model.set_method(sampler)
    assert model.state_dimension == 12
    for _ in range(3):
        model.sample_posterior()
        for e in (eng, eng2, eng3):
            e.ss_sweep(1)
    for e in (eng2, eng3):
        for u, v in zip(eng.get_states(), e.get_states()):
            assert np.array_equal(u, v)
        for c in range(chains):
            assert np.array_equal(eng.ss_get_state_draw(c), e.ss_get_state_draw(c))
    for u, v in zip(model.chain_states(), eng.get_states()):
        assert np.array_equal(u, v)
    for c in range(chains):
        sm = eng.ss_get_state_model(c, 1)
        assert np.array_equal(model.state_variances(c)[1:2], sm["variances"])
        assert np.array_equal(model.state(c), eng.ss_get_state_draw(c).T)
