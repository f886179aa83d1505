"""Forecasts of the Student-t, Poisson and logit state space families on the device
(ba_ss_student_forecast, ba_ss_poisson_forecast, ba_ss_logit_forecast) against the restatement
(tests/family_forecast_ref.py) at every chain's own parameters and final state, read back through
the getters after a few sweeps.

  1  Student: two consecutive calls within 1e-9 max|want| of the restatement
  2  Poisson, logit: cell by cell equal to the restatement (a chain is compared up to its first
     close draw, at most 2 of 64 chains are cut short)
  3  every branch of the count samplers through the public path (a static intercept, newX = 0)
  4  large means: finite, integer-valued, within 8 standard deviations
  5  repeatability; a forecast leaves the next sweep's draws alone
  6  the interface: refusals by text, NULL exposure / trials, the pybind methods
"""
import math

import numpy as np
import pytest

import family_forecast_ref as ffr
from cases import general_data, general_spec
from ss_family_cases import (count_series, golden_mix, logit_engine, poisson_engine, slab_of, student_engine,
                             student_slab_of)
from ss_gpu_helpers import refused

gpu = pytest.mark.gpu
T, P, CHAINS, WARMUP, HORIZON = 40, 3, 64, 5, 6
LISTS = {"level": [("level",)], "trend+seasonal": [("trend",), ("seasonal", 4, 1)], "intercept": [("intercept",)]}


def fair_coin_series(seed):
    """one trial per step at probability 1/2: the chains' intercepts fall on both sides of 0"""
    rs = np.random.Generator(np.random.PCG64(seed))
    X = rs.standard_normal((T, P))
    trials = np.ones(T)
    successes = rs.binomial(1, 0.5, T).astype(float)
    return X, successes, trials, np.log((successes + 0.5) / (trials - successes + 0.5))


def family_engine(family, desc, seed, chains=CHAINS, warmup=WARMUP):
    """the family's engine on a small series after `warmup` sweeps; returns it with its block list"""
    g0 = np.zeros(P, np.uint8)
    g0[0] = 1
    if family == "student":
        X, y, _, _ = general_data(T, P, 2, [(4, 1)] if len(desc) > 1 else [], seed=3)
        blocks = general_spec(y, desc)
        eng = student_engine(chains, seed, y, X, None, blocks, g0)
    elif family == "poisson":
        X, counts, exposure, series = count_series(T, P, 4, seasons=4 if len(desc) > 1 else 0)
        blocks = general_spec(series, desc)
        eng = poisson_engine(chains, seed, counts, exposure, X, None, blocks, g0)
    else:
        X, successes, trials, series = fair_coin_series(5)
        blocks = general_spec(series, desc)
        eng = logit_engine(chains, seed, successes, trials, X, None, blocks, g0)
    sweep(eng, family, warmup)
    return eng, blocks


def sweep(eng, family, n):
    if n:
        {"student": eng.ss_student_sweep, "poisson": eng.ss_poisson_sweep, "logit": eng.ss_logit_sweep}[family](n)


def forecast(eng, family, newX, scale=None):
    if family == "student":
        return eng.ss_student_forecast(newX)
    return eng.ss_poisson_forecast(newX, scale) if family == "poisson" else eng.ss_logit_forecast(newX, scale)


def chain_inputs(eng, family, blocks):
    """what the restatement needs of every chain, through the getters"""
    _, beta, sig = eng.get_states()
    nu = eng.student_get_nu() if family == "student" else np.zeros(eng.chains)
    var = [[eng.ss_get_state_model(c, k, suf=False)["variances"] for k in range(len(blocks))] for c in range(eng.chains)]
    final = [eng.ss_get_state_draw(c)[-1] for c in range(eng.chains)]
    return beta, sig, nu, var, final


def new_predictors(seed, h=HORIZON):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((h, P))


def check_counts(oracle, eng, family, blocks, seed, calls):
    """calls: [(newX, scale)], consecutive.  Equality with the restatement, a chain up to its first close
    draw; returns the draws compared and the number of chains cut short"""
    beta, _, _, var, final = chain_inputs(eng, family, blocks)
    got = [forecast(eng, family, newX, scale) for newX, scale in calls]
    used, cut = [], 0
    for c in range(eng.chains):
        s = ffr.Stream(oracle, seed, c)
        alive = True
        for (newX, scale), out in zip(calls, got):
            if not alive:
                break
            want, draws = ffr.forecast(s, family, T, newX, beta[c], blocks, var[c], final[c], scale=scale)
            for i, d in enumerate(draws):
                if d.close:
                    alive = False
                    cut += 1
                    break
                assert out[c, i] == want[i] or (math.isnan(want[i]) and math.isnan(out[c, i])), (family, c, i, out[c, i], want[i])
                used.append(d)
    return used, cut


# ---- 1 -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("key", ["level", "trend+seasonal"])
def test_student_forecast_matches_restatement(oracle, key):
    seed = 101
    eng, blocks = family_engine("student", LISTS[key], seed)
    beta, sig, nu, var, final = chain_inputs(eng, "student", blocks)
    calls = [new_predictors(7), new_predictors(7)]     # (the same predictors: the second call differs by its stream alone)
    got = [eng.ss_student_forecast(x) for x in calls]
    assert not np.any(got[0] == got[1])
    worst = 0.0
    for c in range(CHAINS):
        s = ffr.Stream(oracle, seed, c)
        for newX, out in zip(calls, got):
            want = ffr.forecast(s, "student", T, newX, beta[c], blocks, var[c], final[c], sigsq_obs=sig[c], nu=nu[c])
            err = np.max(np.abs(out[c] - want)) / np.abs(want).max()
            worst = max(worst, err)
            assert err < 1e-9, (key, c, err)
    print("Student forecast, %s: largest error / max|want| %.2e" % (key, worst))


# ---- 2 -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("family", ["poisson", "logit"])
@pytest.mark.parametrize("key", ["level", "trend+seasonal"])
def test_count_forecasts_equal_restatement_draw_for_draw(oracle, family, key):
    seed = 202
    eng, blocks = family_engine(family, LISTS[key], seed)
    scale = [np.array([0.5, 2.0, 30.0, 1.0, 400.0, 7.5]), np.array([3.0, 0.25, 1.0, 90.0, 12.0, 2500.0])]
    if family == "logit":
        scale = [np.array([1.0, 12.0, 300.0, 0.0, 45.0, 7.0]), np.array([2.0, 64.0, 1.0, 5000.0, 30.0, 9.4])]
    calls = [(new_predictors(11), scale[0]), (new_predictors(12), scale[1])]
    used, cut = check_counts(oracle, eng, family, blocks, seed, calls)
    print("%s, %s: %d draws compared, %d chains cut short" % (family, key, len(used), cut))
    assert cut <= 2 and len(used) >= (CHAINS - 2) * HORIZON


# ---- 3 -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("family", ["poisson", "logit"])
def test_every_branch_of_the_count_samplers_on_the_device(oracle, family):
    seed, h = 303, 48
    eng, blocks = family_engine(family, LISTS["intercept"], seed)
    intercept = np.array([eng.ss_get_state_draw(c)[-1][0] for c in range(CHAINS)])
    rs = np.random.Generator(np.random.PCG64(31))
    if family == "poisson":
        # log-uniform over 1e-3 .. 1e6, and for six chains the two exposures 3 % either side of a mean of 10
        around = np.concatenate([10.0 * np.exp(-intercept[c]) * np.array([0.97, 1.03]) for c in range(6)])
        scale = np.concatenate([np.exp(rs.uniform(np.log(1e-3), np.log(1e6), h - len(around))), around])
    else:
        scale = rs.choice([0.0, 1.0, 7.0, 40.0, 1000.0, 1e5], h)
    used, cut = check_counts(oracle, eng, family, blocks, seed, [(np.zeros((h, P)), scale)])
    taken = {}
    for d in used:
        for part in d.branch.split("+"):
            taken[part] = taken.get(part, 0) + 1
    print(family, "intercepts %.3f .. %.3f" % (intercept.min(), intercept.max()), taken, "cut short:", cut)
    assert cut <= 2
    if family == "poisson":
        lam = scale[None, :] * np.exp(intercept[:, None])
        assert np.sum((lam[:6, -12:] < 10.0).any(axis=1) & (lam[:6, -12:] >= 10.0).any(axis=1)) >= 3
        assert taken.get("inversion", 0) >= 100 and taken.get("ptrs", 0) >= 100
    else:
        assert taken.get("inversion", 0) >= 100 and taken.get("btrs", 0) >= 100 and taken.get("mirror", 0) >= 100
        assert taken.get("edge", 0) >= 1     # (no trials)


# ---- 4 -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("family", ["poisson", "logit"])
def test_large_means_are_sane(family):
    eng, _ = family_engine(family, LISTS["intercept"], 404)
    intercept = np.array([eng.ss_get_state_draw(c)[-1][0] for c in range(CHAINS)])
    scale = np.array([1e9, 1e12, 1e9, 1e12]) if family == "poisson" else np.full(4, 1e8)
    out = forecast(eng, family, np.zeros((4, P)), scale)
    assert np.all(np.isfinite(out)) and np.array_equal(out, np.floor(out))
    if family == "poisson":
        mean = scale[None, :] * np.exp(intercept[:, None])
        sd = np.sqrt(mean)
    else:
        pr = 1.0 / (1.0 + np.exp(-intercept[:, None]))
        mean = scale[None, :] * pr
        sd = np.sqrt(mean * (1.0 - pr))
    z = np.abs(out - mean) / sd
    print("%s: largest |k - mean| / sd %.2f" % (family, z.max()))
    assert z.max() < 8.0


# ---- 5 -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("family", ["student", "poisson", "logit"])
def test_forecasts_repeat_and_leave_the_sampler_alone(family):
    seed, desc = 505, LISTS["trend+seasonal"]
    newX = new_predictors(21)
    scale = None if family == "student" else np.array([1.0, 20.0, 3.0, 150.0, 2.0, 40.0])
    a, _ = family_engine(family, desc, seed, chains=8)
    b, _ = family_engine(family, desc, seed, chains=8)
    plain, _ = family_engine(family, desc, seed, chains=8)
    fa, fb = forecast(a, family, newX, scale), forecast(b, family, newX, scale)
    assert fa.tobytes() == fb.tobytes()
    sweep(a, family, 1)
    sweep(plain, family, 1)
    for u, w in zip(a.get_states(), plain.get_states()):
        assert np.array_equal(u, w)
    for c in (0, 7):
        assert np.array_equal(a.ss_get_state_draw(c), plain.ss_get_state_draw(c))


# ---- 6 -----------------------------------------------------------------------------------------------
@gpu
def test_refusals_and_their_texts():
    import boom_amd
    from boom_amd.capi import _fcol, _p
    newX = new_predictors(1)
    engines = {f: family_engine(f, LISTS["level"], 606, chains=4, warmup=0)[0] for f in ("student", "poisson", "logit")}
    # another data kind
    for f, eng in engines.items():
        for g in engines:
            if g != f:
                refused(lambda: forecast(eng, g, newX), "call ba_ss_%s_set_data first" % g)
    X, y, _, _ = general_data(T, P, 2, [], seed=3)
    plain = boom_amd.Engine(2, seed=1)
    plain.ss_set_data(y, X, None)
    for g in engines:
        refused(lambda: forecast(plain, g, newX), "call ba_ss_%s_set_data first" % g)
    # no state draw yet
    for f, eng in engines.items():
        refused(lambda: forecast(eng, f, newX), "no state draw yet: run ba_ss_%s_sweep or ba_ss_%s_impute_state first" % (f, f))
        sweep(eng, f, 1)
        forecast(eng, f, newX)
    # horizon and null pointers
    out = np.zeros((4, HORIZON))
    st, po, lo = engines["student"], engines["poisson"], engines["logit"]
    x = _fcol(newX)
    for call in (lambda: st._check(st.lib.ba_ss_student_forecast(st._h, 0, _p(x), _p(out))),
                 lambda: st._check(st.lib.ba_ss_student_forecast(st._h, HORIZON, None, _p(out))),
                 lambda: st._check(st.lib.ba_ss_student_forecast(st._h, HORIZON, _p(x), None)),
                 lambda: po._check(po.lib.ba_ss_poisson_forecast(po._h, -1, _p(x), None, _p(out))),
                 lambda: po._check(po.lib.ba_ss_poisson_forecast(po._h, HORIZON, None, None, _p(out))),
                 lambda: lo._check(lo.lib.ba_ss_logit_forecast(lo._h, HORIZON, _p(x), None, None)),
                 lambda: lo._check(lo.lib.ba_ss_logit_forecast(lo._h, 0, _p(x), None, _p(out)))):
        refused(call, "bad argument")
    # exposures and trial counts
    for bad in (-1.0, np.nan, np.inf):
        scale = np.ones(HORIZON)
        scale[2] = bad
        refused(lambda: po.ss_poisson_forecast(newX, scale), "exposures of a forecast must be non-negative and finite")
        refused(lambda: lo.ss_logit_forecast(newX, scale), "trial counts of a forecast must be non-negative and finite")
    # an exposure of 0 and no trials are served: the cell is 0
    scale = np.ones(HORIZON)
    scale[3] = 0.0
    assert np.all(po.ss_poisson_forecast(newX, scale)[:, 3] == 0.0) and np.all(lo.ss_logit_forecast(newX, scale)[:, 3] == 0.0)
    # a mean that overflows is NaN (eta = +inf), a rate of 0 gives 0 (eta = -inf); no chain stops
    g1 = np.array([1, 0, 0], np.uint8)
    po.set_state(g1, np.array([1.0, 0.0, 0.0]))
    po.ss_poisson_impute_state()
    huge = np.zeros((HORIZON, P))
    huge[:, 0] = [1e300, -1e300] * (HORIZON // 2)
    cells = po.ss_poisson_forecast(huge)
    assert np.all(np.isnan(cells[:, 0::2])) and np.all(cells[:, 1::2] == 0.0)
    lo.set_state(g1, np.array([1.0, 0.0, 0.0]))
    lo.ss_logit_impute_state()
    cells = lo.ss_logit_forecast(huge, np.full(HORIZON, 9.0))
    assert np.all(cells[:, 0::2] == 9.0) and np.all(cells[:, 1::2] == 0.0)     # (plogis saturates to exactly 1 and 0)
    po.ss_poisson_sweep(1)
    lo.ss_logit_sweep(1)


@gpu
@pytest.mark.parametrize("family", ["poisson", "logit"])
def test_null_scale_is_ones(family):
    a, _ = family_engine(family, LISTS["level"], 707, chains=8)
    b, _ = family_engine(family, LISTS["level"], 707, chains=8)
    newX = new_predictors(2)
    assert np.array_equal(forecast(a, family, newX, None), forecast(b, family, newX, np.ones(HORIZON)))


def level_model(boom, blocks):
    b = blocks[0]
    level = boom.LocalLevelStateModel(float(b["initial_sigma"][0]))
    level.set_initial_state_mean(float(b["a0"][0]))
    level.set_initial_state_variance(float(b["P0"][0]))
    level.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    return level


@gpu
@pytest.mark.parametrize("family", ["student", "poisson", "logit"])
def test_pybind_methods_return_what_capi_returns(family):
    import boom_amd._boom as boom
    chains, seed, rounds = 3, 808, 3
    g0 = np.zeros(P, np.uint8)
    newX = new_predictors(3)
    scale = np.array([2.0, 1.0, 25.0, 3.0, 1.0, 60.0])
    if family == "student":
        X, y, _, _ = general_data(T, P, 2, [], seed=3)
        blocks = general_spec(y, LISTS["level"])
        mu, prec, pi = student_slab_of(P)
        model = boom.StateSpaceStudentRegressionModel(y, X, [], chains=chains, seed=seed)
        model.add_state(level_model(boom, blocks))
        sampler = boom.StateSpaceStudentPosteriorSampler(model, boom.MvnGivenScalarSigma(mu, prec), boom.VariableSelectionPrior(pi),
                                                         boom.ChisqModel(1.0, 1.0), boom.UniformModel(0.1, 100.0))
        eng = student_engine(chains, seed, y, X, None, blocks, g0)
    elif family == "poisson":
        X, counts, exposure, series = count_series(T, P, 4)
        blocks = general_spec(series, LISTS["level"])
        mu, prec, pi = slab_of(P)
        mix = golden_mix()
        model = boom.StateSpacePoissonModel(counts, exposure, X, [], chains=chains, seed=seed)
        model.set_mixture_table([int(c) for c in mix["counts"]], [int(c) for c in mix["ncomp"]], mix["mu"], mix["sigma"],
                                mix["weight"], mix["largest_index"])
        model.add_state(level_model(boom, blocks))
        sampler = boom.StateSpacePoissonPosteriorSampler(model, boom.MvnModel(mu, prec, True), boom.VariableSelectionPrior(pi))
        eng = poisson_engine(chains, seed, counts, exposure, X, None, blocks, g0)
    else:
        X, successes, trials, series = fair_coin_series(5)
        blocks = general_spec(series, LISTS["level"])
        mu, prec, pi = slab_of(P)
        model = boom.StateSpaceLogitModel(successes, trials, X, [], chains=chains, seed=seed)
        model.add_state(level_model(boom, blocks))
        sampler = boom.StateSpaceLogitPosteriorSampler(model, boom.MvnModel(mu, prec, True), boom.VariableSelectionPrior(pi))
        eng = logit_engine(chains, seed, successes, trials, X, None, blocks, g0)
    model.set_method(sampler)
    for _ in range(rounds):
        model.sample_posterior()
    sweep(eng, family, rounds)
    for u, w in zip(model.chain_states(), eng.get_states()):
        assert np.array_equal(u, w)
    if family == "student":
        got = [model.simulate_forecast(newX), model.simulate_forecast(newX)]
        want = [eng.ss_student_forecast(newX), eng.ss_student_forecast(newX)]
    else:
        got = [model.simulate_forecast(newX), model.simulate_forecast(newX, scale)]
        want = [forecast(eng, family, newX), forecast(eng, family, newX, scale)]
    for u, w in zip(got, want):
        assert u.shape == (chains, HORIZON) and np.array_equal(u, w)
    with pytest.raises(Exception, match="do not match the model dimension"):
        model.simulate_forecast(np.zeros((HORIZON, P + 1)))
