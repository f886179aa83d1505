"""The random-walk holiday state model on the device (ba_ss_add_state_model kind 10, bsts
AddRandomWalkHoliday): the holiday instances of the general structural kernel (a calendar-selected
observation row and state-error row), its variance draw, forecast, prediction errors and look-ahead.

  identity      a width-1 block active at every step against a local level in its place
  filter edges  one impute_state against the restatement (tests/ss_holiday_oracle.py): windows across
                the kernel's 64-step time-block edges, active at t = 0 and T - 1, two holidays on one
                day, recurring positions, missing observations on active days; SMALL, LDC 33 and GLOB
                instances; a never-active block
  whole rounds  ba_ss_sweep(1) x 12 against the restatement given the device's regression draw;
                ba_ss_sweep(12) and ba_ss_draw_next under a look-ahead of 4 the same draws, bit for bit
  distribution  4096 chains' state draws against the dense Gaussian posterior
  forecast      against the restatement on the forecast stream; a horizon past the calendar is refused
  errors        ba_ss_prediction_errors against the restatement's filter
  interface     refusals and their texts, the pybind class
"""
import numpy as np
import pytest

import prediction_errors_ref as per
import ss_holiday_cases as shc
import ss_holiday_oracle as sho
import ss_student_oracle as sso
from cases import bsts_priors, general_spec
from ss_gpu_helpers import RTOL, close, engine, refused

gpu = pytest.mark.gpu


# ---- 1. identity ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pad", [False, True])
def test_always_active_width_one_equals_a_local_level(pad):
    """[holiday (1), always active + 4 seasons (+ 20 seasons: state dimension 23, not SMALL)] against
    the same list with a local level, both through the general kernel; variances as given"""
    T, chains, seed, sigsq = 70, 4, 77, 0.5
    seas = [("seasonal", 4, 1)] + ([("seasonal", 20, 1)] if pad else [])
    X, y, obs = shc.data(T, seasonal=((4, 1),))
    sdy = float(np.std(y, ddof=1))
    plain = general_spec(y, [("level",)] + seas)
    plain[0]["a0"] = np.zeros(1)
    hol = [sho.holiday_block(1, np.zeros(T, np.int32), sdy, plain[0]["initial_sigma"][0])] + plain[1:]
    assert sum(b["dim"] for b in hol) == (23 if pad else 4)
    gam, beta = shc.chain_parameters(chains, 3)
    a = engine(chains, seed, y, X, obs, hol, gam[0])
    b = engine(chains, seed, y, X, obs, plain, gam[0], kernel=0)
    for c in range(chains):
        a.set_state(gam[c], beta[c], sigsq, chain=c)
        b.set_state(gam[c], beta[c], sigsq, chain=c)
    a.ss_impute_state()
    b.ss_impute_state()
    same = True
    for c in range(chains):
        u, v = a.ss_get_state_draw(c), b.ss_get_state_draw(c)
        same = same and np.array_equal(u, v)
        assert np.max(np.abs(u - v)) <= 1e-12 * np.abs(v).max(), c
        for k in range(len(hol)):
            su, sv = a.ss_get_state_model(c, k), b.ss_get_state_model(c, k)
            assert np.array_equal(su["suf_n"], sv["suf_n"]), (c, k)
            assert close(su["suf_ss"], sv["suf_ss"], 1e-12), (c, k)
            same = same and np.array_equal(su["suf_ss"], sv["suf_ss"])
    print("width-1 holiday against the local level (pad=%s): bits coincide: %s" % (pad, same))


# ---- 2. one impute_state against the restatement ---------------------------------------------------------
EDGE_CASES = {
    "a, T=70": (70, lambda y, T: shc.list_a(y, T), {}),
    "a, T=130": (130, lambda y, T: shc.list_a(y, T), {}),
    "b (LDC 33), T=70": (70, lambda y, T: shc.list_a(y, T, pad=True), {}),
    "c (GLOB), T=70": (70, shc.list_c, dict(seasonal=(), trig=[(12.0, [1.0, 2.0])], missing=(31, 63))),
    "c (GLOB), T=130": (130, shc.list_c, dict(seasonal=(), trig=[(12.0, [1.0, 2.0])], missing=(31, 64, 128))),
    "d (never active), T=70": (70, shc.list_d, dict(seasonal=())),
    # the calendar instances no list above reaches (2 chains, p = 2)
    "instance LDC 33, GLOB": shc.instance_case(18, True),
    "instance LDC 61": shc.instance_case(34, False),
    "instance LDC 61, GLOB": shc.instance_case(34, True),
    "instance LDC 65": shc.instance_case(61, False),
    "instance LDC 65, GLOB": shc.instance_case(61, True),
}


def check_state_models(eng, o, ch, tag):
    for j in range(len(o.blocks)):
        sm = eng.ss_get_state_model(ch, j)
        nv = len(sm["variances"])
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
    chains, seed, sigsq = (2 if name.startswith("instance") else 4), 41, 0.8
    X, y, obs = shc.data(T, **kw)
    blocks = make(y, T)
    gam, beta = shc.chain_parameters(chains, 8, X.shape[1])
    eng = engine(chains, seed, y, X, obs, blocks, gam[0])
    for c in range(chains):
        eng.set_state(gam[c], beta[c], sigsq, chain=c)
    eng.ss_impute_state()
    worst = 0.0
    for c in range(chains):
        o = sho.HolidayOracle(oracle, T, obs, blocks, seed, c)
        inc = np.flatnonzero(gam[c])
        o.impute_state(y - X[:, inc] @ beta[c][inc], sigsq)
        worst = max(worst, check_state_models(eng, o, c, (name, c)))
    print("%s: state draw, worst error / max |state| %.3e" % (name, worst))


# ---- 3. whole rounds ---------------------------------------------------------------------------------------
@gpu
def test_whole_rounds_match_restatement(oracle):
    c = shc.loop_case()
    T, X, y, obs, blocks, rounds = c["T"], c["X"], c["y"], c["obs"], c["blocks"], c["rounds"]

    def fresh():
        e = engine(c["chains"], c["seed"], y, X, obs, blocks, c["g0"])
        e.set_state(c["g0"], c["b0"], c["sig0"])
        return e

    eng = fresh()
    ora = {ch: sho.HolidayOracle(oracle, T, obs, blocks, c["seed"], ch) for ch in c["check"]}
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
    # ... and the same 12 draws handed out under a look-ahead of 4
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
    """list (a) cut to T = 12: level + 4 seasons + holiday (3) + holiday (2), variances fixed"""
    T, chains, sigsq = 12, 4096, 0.6
    X, y, obs = shc.data(T, seasonal=((4, 1),), missing=(7,))
    sdy = float(np.std(y, ddof=1))
    c1 = shc.calendar(3, T, [(0, 1, 2), (5, 0, 3), (T - 1, 0, 1)])
    c2 = shc.calendar(2, T, [(6, 0, 2), (9, 0, 2)])   # days 6 and 7: both active, 7 is missing
    blocks = general_spec(y, [("level",), ("seasonal", 4, 1)])
    blocks += [sho.holiday_block(3, c1, sdy, 0.6), sho.holiday_block(2, c2, sdy, 0.4)]
    g0 = np.zeros(shc.P, np.uint8)
    eng = engine(chains, 20264, y, X, obs, blocks, g0)
    eng.set_state(g0, np.zeros(shc.P), sigsq)
    eng.ss_impute_state()
    draws = np.stack([eng.ss_get_state_draw(c).reshape(-1) for c in range(chains)])
    S = sho.Structure(blocks)
    var = [b["initial_sigma"] ** 2 for b in blocks]
    mean, cov = sho.dense_posterior(S, var, y, obs.astype(bool), np.full(T, sigsq))
    d = len(mean)
    bound = sso.bonferroni_bound(d + d * (d + 1) // 2)   # (level 1e-3, fixed with the seed before any run)
    zm, zc = sso.moment_z(draws, mean, cov)
    print("largest |z|: mean %.3f covariance %.3f, bound %.3f" % (np.abs(zm).max(), np.abs(zc).max(), bound))
    assert np.abs(zm).max() < bound
    assert np.abs(zc).max() < bound


# ---- 5. forecast -----------------------------------------------------------------------------------------------
def swept_engine(chains=4, seed=53, sweeps=3):
    T = 70
    X, y, obs = shc.data(T)
    blocks = shc.list_a(y, T)
    g0 = np.zeros(shc.P, np.uint8)
    g0[0] = 1
    eng = engine(chains, seed, y, X, obs, blocks, g0)
    eng.ss_sweep(sweeps)
    return eng, T, X, y, obs, blocks, seed


@gpu
def test_forecast_matches_restatement(oracle):
    """horizon 10: the window open at T - 1 goes on into the horizon and another opens inside it"""
    import boom_amd
    eng, T, X, y, obs, blocks, seed = swept_engine()
    rs = np.random.Generator(np.random.PCG64(9))
    newX = rs.standard_normal((shc.HORIZON, shc.P))
    fc = eng.ss_forecast(newX)
    gam, beta, sig = eng.get_states()
    for c in range(eng.chains):
        o = sho.HolidayOracle(oracle, T, obs, blocks, seed, c)
        o.var = [eng.ss_get_state_model(c, k, suf=False)["variances"] for k in range(len(blocks))]
        want = o.forecast(eng.ss_get_state_draw(c)[-1], sig[c], newX @ (beta[c] * gam[c]))
        assert np.max(np.abs(fc[c] - want)) < 1e-8 * max(1.0, np.abs(want).max()), c
    with pytest.raises(boom_amd.BoomAmdError) as e:
        eng.ss_forecast(np.zeros((shc.HORIZON + 1, shc.P)))
    assert "a forecast of horizon 11 needs 81" in str(e.value), str(e.value)


# ---- 6. prediction errors ----------------------------------------------------------------------------------------
@gpu
def test_prediction_errors_match_restatement(oracle):
    eng, T, X, y, obs, blocks, seed = swept_engine(seed=54)
    full = eng.ss_prediction_errors(variances=True, log_likelihood=True)
    std = eng.ss_prediction_errors(standardize=True)
    S = sho.Structure(blocks)
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
        # (the restatement's own two-part filter is the same filter)
        o = sho.HolidayOracle(oracle, T, obs, blocks, seed, c)
        o.var = var
        inc = np.flatnonzero(gam[c])
        v2, F2, ll2 = o.prediction_errors(y - X[:, inc] @ beta[c][inc], sig[c])
        assert np.max(np.abs(v2 - ref["v"]) / np.sqrt(ref["F"])) <= gate["v"] and abs(ll2 - ref["loglik"]) <= gate["loglik"] * abs(ref["loglik"])
    print("worst device / gate  v %.3f  std %.3f  F %.3f  loglik %.3f" % (worst["v"], worst["std"], worst["F"], worst["loglik"]))


# ---- 7. interface ------------------------------------------------------------------------------------------------
@gpu
def test_refusals_and_their_texts():
    import boom_amd
    T = 30
    X, y, obs = shc.data(T, seasonal=(), missing=())
    sdy = float(np.std(y, ddof=1))
    cal = shc.calendar(3, T, [(3, 0, 3), (20, 0, 3)])
    g0 = np.zeros(shc.P, np.uint8)

    def blocks(width=3, calendar=cal):
        b = sho.holiday_block(width, np.zeros(0, np.int32), sdy)
        b["calendar"] = calendar
        return general_spec(y, [("level",)]) + [b]

    # the width
    eng = boom_amd.Engine(2, seed=1)
    eng.ss_set_data(y, X, None)
    for w in (0, 64):
        refused(lambda: eng.ss_set_state_models(blocks(w, None)), "a random-walk holiday's width must lie in [1, 63]")
    # a position outside [0, width)
    for bad in (3, -2):
        wrong = cal.copy()
        wrong[5] = bad
        refused(lambda: eng.ss_set_state_models(blocks(3, wrong)),
                "holiday calendar entry 5 is %d: it must be -1 (inactive) or a position in [0, 3)" % bad)
    # a calendar on a block that is none
    eng.ss_set_state_models(blocks(3, None))
    refused(lambda: eng.ss_set_holiday_calendar(0, cal), "not a random-walk holiday state model")
    # no calendar, a short one: every call that launches
    eng = engine(2, 1, y, X, None, blocks(3, None), g0)
    for fn in (lambda: eng.ss_sweep(1), eng.ss_impute_state, eng.ss_draw_next, eng.ss_prediction_errors):
        refused(fn, "state model 1 is a random-walk holiday without a calendar")
    eng.ss_set_holiday_calendar(1, cal[:T - 1])
    for fn in (lambda: eng.ss_sweep(1), eng.ss_impute_state, eng.ss_draw_next, eng.ss_prediction_errors):
        refused(fn, "the holiday calendar of state model 1 has 29 entries, the series has 30 time points")
    eng.ss_set_holiday_calendar(1, cal)
    assert np.array_equal(eng.ss_get_holiday_calendar(1), cal)
    eng.ss_sweep(2)
    sm = eng.ss_get_state_model(0, 1)
    assert sm["suf_n"][0] == 6 and sm["suf_ss"][0] > 0
    refused(lambda: eng.ss_forecast(np.zeros((1, shc.P))), "a forecast of horizon 1 needs 31")
    # under a look-ahead the setter is a mutator: the draws after it are those of a run without the look-ahead
    eng.ss_set_lookahead(4)
    eng.ss_draw_next()
    eng.ss_set_holiday_calendar(1, np.concatenate([cal, [-1, 0]]))
    eng.ss_draw_next()
    plain = engine(2, 1, y, X, None, blocks(), g0)
    plain.ss_sweep(4)
    for u, v in zip(eng.get_states(), plain.get_states()):
        assert np.array_equal(u, v)
    assert eng.ss_forecast(np.zeros((2, shc.P))).shape == (2, 2)
    # the other observation families: the block added on such data ...
    text = "the random-walk holiday is built for the Gaussian observation model only"
    from ss_family_cases import count_series, golden_mix
    Xc, counts, exposure, _ = count_series(T, shc.P, 4)
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
        e3.sss_set_slab(np.zeros(shc.P), 0.1 * np.eye(shc.P), scales_with_sigsq=scales)
        e3.set_spike(np.full(shc.P, 0.5))
        if scales:
            e3.set_sigma_prior(1.0, 1.0)
        e3.set_state(g0)
        refused(lambda: sweep(e3), text)
    # a Student local linear trend in the same list, in both orders
    import student_trend_cases as stc
    text = "a list that holds both a random-walk holiday and a Student local linear trend is not built"
    st = stc.student_trend_spec(y, [("student_trend",)])
    e4 = boom_amd.Engine(2, seed=1)
    e4.ss_set_data(y, X, None)
    refused(lambda: e4.ss_set_state_models(st + blocks()[1:]), text)
    refused(lambda: e4.ss_set_state_models(blocks()[1:] + st), text)


@gpu
def test_pybind_class_agrees_with_the_c_abi():
    """boom.RandomWalkHolidayStateModel(positions, width) in a StateSpaceRegressionModel: three rounds ==
    the engine through the C-ABI on the same seed, bit for bit"""
    import boom_amd
    import boom_amd._boom as boom
    T, chains, seed = 70, 3, 23
    X, y, obs = shc.data(T)
    blocks = shc.list_a(y, T)[:3]   # level + 7 seasons + holiday (3)
    prior, _, sig_up = bsts_priors(X, y, 2)
    model = boom.StateSpaceRegressionModel(y, X, [bool(o) for o in obs], chains=chains, seed=seed)
    b = blocks[0]
    level = boom.LocalLevelStateModel(float(b["initial_sigma"][0]))
    level.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    level.set_initial_state_mean(float(b["a0"][0]))
    level.set_initial_state_variance(float(b["P0"][0]))
    b = blocks[1]
    seas = boom.SeasonalStateModel(7)
    seas.set_sigsq(b["initial_sigma"][0] ** 2)
    seas.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    seas.set_initial_state_mean(b["a0"])
    seas.set_initial_state_variance(b["P0"][0])
    b = blocks[2]
    hol = boom.RandomWalkHolidayStateModel([int(k) for k in b["calendar"]], 3)
    hol.set_sigsq(b["initial_sigma"][0] ** 2)
    hol.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    hol.set_initial_state_mean(b["a0"])
    hol.set_initial_state_variance(b["P0"])
    for s in (level, seas, hol):
        model.add_state(s)
    sampler = boom.StateSpacePosteriorSampler(model, boom.MvnGivenScalarSigma(prior["b"], prior["ominv"]),
                                              boom.ChisqModel(prior["df"], prior["sigma_guess"]),
                                              boom.VariableSelectionPrior(prior["pi"]), sig_up)
    model.set_method(sampler)
    assert model.state_dimension == 10
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_set_data(y, X, obs)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"], sigma_upper_limit=sig_up)
    eng.ss_set_state_models(blocks)
    eng.set_state(np.zeros(shc.P, np.uint8))
    for _ in range(3):
        model.sample_posterior()
        eng.ss_sweep(1)
    for u, v in zip(model.chain_states(), eng.get_states()):
        assert np.array_equal(u, v)
    for c in range(chains):
        sm = eng.ss_get_state_model(c, 2)
        assert np.array_equal(model.state_variances(c)[2:3], sm["variances"])
        assert np.array_equal(model.state(c), eng.ss_get_state_draw(c).T)
