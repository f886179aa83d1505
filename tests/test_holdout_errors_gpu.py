"""ba_ss_holdout_prediction_errors (bsts.prediction.errors' holdout part) on the device against the dense
long-double filter of tests/holdout_errors_ref.py, at exactly the parameters and the final state the accessors
report after three sweeps: the local-level path and every kind of Gaussian state model, T = 40, at the horizons
that are the kernel's 64-step block edges.  The gate of each comparison comes from the reference alone
(holdout_errors_ref.reference_and_gate: float64 against long double in both algebraic forms, times 8, at least
64 u); the worst device-to-gate ratio of each case is printed.  Then horizon 1 in closed form, what makes the call
an observer -- prefixes, sub-ranges and repeats to the bit, purity against a twin that never asks, the look-ahead
--, the forecast variance that is not positive, the refusals and the pybind facade.

Worst device / gate ratios measured on an MI355X (v, v / sqrt F, F): see DESIGN.md section 3.28."""
import ctypes as C

import numpy as np
import pytest

import holdout_errors_ref as her
import prediction_errors_ref as per
import ss_dynreg_ar_oracle as sda
import ss_dynreg_cases as sdc
import ss_dynreg_oracle as sdo
import ss_state_models_oracle as ssm
from cases import bsts_priors, general_data, general_spec
from ss_calendar_seasonal_oracle import calendar_block, starts_calendar
from ss_gpu_helpers import refused
from ss_holiday_oracle import holiday_block

pytestmark = pytest.mark.gpu
CHAINS, P, T0, HMAX = 4, 3, 40, 130
HORIZONS = (1, 2, 63, 64, 65, 130)
U = her.U
DP = C.POINTER(C.c_double)


def series(T, seed, seasonals=(), **kw):
    """T steps of a series and the HMAX rows that follow it; the priors come from the series alone"""
    X, y, _, _ = general_data(T + HMAX, P, 2, list(seasonals), seed=seed, **kw)
    prior, ss, sig_up = bsts_priors(X[:T], y[:T], 2)
    obs = np.ones(T, np.uint8)
    obs[7] = 0
    return dict(T=T, X=np.ascontiguousarray(X[:T]), y=np.ascontiguousarray(y[:T]), obs=obs, prior=prior, ss=ss, sig_up=sig_up,
                newX=np.ascontiguousarray(X[T:]), newY=np.ascontiguousarray(y[T:]), sdy=float(np.std(y[:T], ddof=1)))


def engine(d, blocks, seed, chains=CHAINS):
    """blocks None: the local level through ba_ss_set_local_level"""
    import boom_amd
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_set_data(d["y"], d["X"], d["obs"])
    pr = d["prior"]
    eng.set_priors(pr["b"], pr["ominv"], pr["pi"], pr["df"], pr["sigma_guess"], sigma_upper_limit=d["sig_up"])
    if blocks is None:
        ss = d["ss"]
        eng.ss_set_local_level(ss["level_df"], ss["level_sigma_guess"], ss["level_sigma_upper_limit"],
                               ss["initial_state_mean"], ss["initial_state_variance"], ss["initial_level_sigma"])
    else:
        eng.ss_set_state_models(sda.engine_blocks(blocks))
    g0 = np.ones(P, np.uint8)
    eng.set_state(g0)
    return eng


def swept(d, blocks, seed, chains=CHAINS):
    """three sweeps, so that every parameter has moved; then the regression of chains 1 - 3 is set by hand: none
    included, one, two (chain 0 keeps what it drew)"""
    eng = engine(d, blocks, seed, chains)
    eng.ss_sweep(3)
    rs = np.random.Generator(np.random.PCG64(seed + 1))
    for c, g in [(1, [0, 0, 0]), (2, [1, 0, 0]), (3, [1, 0, 1])]:
        if c < chains:
            g = np.array(g, np.uint8)
            eng.set_state(g, rs.standard_normal(P) * g, float(eng.get_state(c)[2]), chain=c)
    return eng


def is_structure(blocks):
    return blocks is not None and any(b["kind"] not in (1, 2, 3, 4, 5, 6, 7) for b in blocks)


def chain_view(eng, blocks, d, c):
    """what the accessors report for chain c: (view, final state, sigma^2, gamma, beta)"""
    g, b, s = eng.get_state(c)
    if blocks is None:
        ss = d["ss"]
        rb = [dict(kind=1, a0=[ss["initial_state_mean"]], P0=[ss["initial_state_variance"]], initial_sigma=[ss["initial_level_sigma"]])]
        st = eng.ss_get_state(c)
        return her.model_view(rb, [dict(var=np.array([st["level_sigsq"]]), phi=None)]), st["state"][-1:], s, g, b
    alpha = eng.ss_get_state_draw(c)[-1]
    sm = [eng.ss_get_state_model(c, k, suf=False) for k in range(len(blocks))]
    if is_structure(blocks):
        at = [dict(blk, phi=m["phi"]) if blk["kind"] == sda.DYNREG_AR else blk for blk, m in zip(blocks, sm)]
        return her.structure_view(ssm.Structure(at), [m["variances"] for m in sm]), alpha, s, g, b
    return her.model_view(blocks, [dict(var=m["variances"], phi=m.get("phi")) for m in sm]), alpha, s, g, b


def holdout(eng, d, h, **kw):
    return eng.ss_holdout_prediction_errors(d["newX"][:h], d["newY"][:h], **kw)


def check(eng, blocks, d, label, horizons=HORIZONS):
    """every output of every chain within the gate at every horizon; the runs of the reference are made once per
    chain, at the longest horizon"""
    hmax = max(horizons)
    chains = eng.chains
    runs = []
    for c in range(chains):
        view, alpha, s, g, b = chain_view(eng, blocks, d, c)
        runs.append(her.reference_runs(view, alpha, d["T"], s, d["newY"][:hmax], d["newX"][:hmax], g, b))
    for h in horizons:
        full = holdout(eng, d, h, variances=True)
        std = holdout(eng, d, h, standardize=True)
        assert full["errors"].shape == (chains, h) and full["variances"].shape == (chains, h) and std.shape == (chains, h)
        worst = {}
        for c in range(chains):
            ref, gate = her.gate_of(runs[c], h)
            dev = her.device_deviation(ref, full["errors"][c], full["variances"][c], std[c])
            for k, v in dev.items():
                r = v / gate["v" if k == "std" else k]
                worst[k] = max(worst.get(k, 0.0), r)
                assert r <= 1.0, (label, h, c, k, v, gate)
        print("%s, h=%d: worst device / gate  v %.3f  std %.3f  F %.3f" % (label, h, worst["v"], worst["std"], worst["F"]))


# ---- the lists
def holiday_calendar(T, windows, width=3):
    cal = np.full(T + HMAX, -1, np.int32)
    for first in windows:
        cal[first:first + width] = np.arange(width)
    return cal


def kinds_list(name, d):
    y, T, sdy = d["y"], d["T"], d["sdy"]
    level = general_spec(y, [("level",)])
    if name.startswith("holiday"):
        windows = {"holiday covers T": (10, T - 1, T + 62), "holiday straddles later steps": (10, T + 5, T + 63),
                   "holiday never active": ()}[name]
        return level + [holiday_block(3, holiday_calendar(T, windows), sdy)]
    if name == "calendar seasonal":
        starts = (3, 9, 14, 22, 27, 35, T, T + 7, T + 12, T + 21, T + 30, T + 42, T + 55, T + 63, T + 64, T + 70, T + 85, T + 100, T + 128)
        return level + [calendar_block(4, starts_calendar(T + HMAX, starts), sdy)]
    if name == "dynamic regression d=2":
        return level + [sdo.dynreg_block(sdc.predictors(T + HMAX, 2, 71, hard=T), sdy, [0.3, 0.5])]
    if name == "AR dynamic regression 2x2":
        return level + sda.dynreg_ar_blocks(sdc.predictors(T + HMAX, 2, 72, hard=T), 2, sdy, [0.3, 0.5], [[0.5, -0.2], [0.3, 0.2]])
    raise KeyError(name)


LISTS = {
    "local level path": (None, T0, {}),
    "level": ([("level",)], T0, {}),
    "trend+seasonal(4,3,t0=1), T on a boundary": ([("trend",), ("seasonal", 4, 3, 1)], 40, dict(seasonals=[(4, 3)])),
    "trend+seasonal(4,3,t0=1), T off a boundary": ([("trend",), ("seasonal", 4, 3, 1)], 41, dict(seasonals=[(4, 3)])),
    "ar3": ([("ar", 3, [0.5, -0.2, 0.1])], T0, dict(level=False, ar_coef=[0.5, -0.2, 0.1])),
    "intercept+trig x2": ([("intercept",), ("trig", 7.0, [1.0, 2.0])], T0, dict(level=False, trig=[(7.0, [1.0, 2.0])], intercept=2.0)),
    "semilocal+seasonal7": ([("semilocal",), ("seasonal", 7, 1)], T0, dict(seasonals=[(7, 1)])),
    "holiday covers T": ("kinds", T0, {}),
    "holiday straddles later steps": ("kinds", T0, {}),
    "holiday never active": ("kinds", T0, {}),
    "calendar seasonal": ("kinds", T0, {}),
    "dynamic regression d=2": ("kinds", T0, {}),
    "AR dynamic regression 2x2": ("kinds", T0, {}),
    "m=33": ([("trend",), ("seasonal", 32, 1)], T0, dict(seasonals=[(32, 1)])),
    "m=64": ([("trend",), ("seasonal", 53, 1), ("ar", 10, [0.3, 0.1] + [0.0] * 8)], T0, dict(seasonals=[(53, 1)], ar_coef=[0.3, 0.1])),
}


def case(name, seed=31):
    desc, T, kw = LISTS[name]
    d = series(T, seed, **kw)
    if desc is None:
        return d, None
    return d, kinds_list(name, d) if desc == "kinds" else general_spec(d["y"], desc)


@pytest.mark.parametrize("name", list(LISTS))
def test_every_list_at_the_block_edges(name):
    d, blocks = case(name)
    if name.startswith("trend+seasonal"):
        assert ((d["T"] - 1) % 3 == 0) == ("on a boundary" in name)   # (time t starts a season where (t - 1) % 3 == 0)
    if name.startswith("m="):
        assert sum(per.block_dim(b) for b in blocks) == int(name[2:])
    eng = swept(d, blocks, 41)
    assert any(eng.get_state(c)[0].sum() == 0 for c in range(CHAINS)) and any(eng.get_state(c)[0].sum() in (1, 2) for c in range(CHAINS))
    check(eng, blocks, d, name)


# ---- horizon 1 in closed form
@pytest.mark.parametrize("name", ["local level path", "trend+seasonal(4,3,t0=1), T on a boundary",
                                  "trend+seasonal(4,3,t0=1), T off a boundary", "semilocal+seasonal7", "holiday covers T",
                                  "holiday straddles later steps", "calendar seasonal", "AR dynamic regression 2x2"])
def test_horizon_one_closed_form(name):
    """v_0 = y*_0 - Z_T'T_{T-1} alpha and F_0 = Z_T'RQR_{T-1} Z_T + sigma^2, at 64 u sqrt F (F: 64 u F)"""
    d, blocks = case(name)
    eng = swept(d, blocks, 43)
    got = holdout(eng, d, 1, variances=True)
    L = np.longdouble
    for c in range(CHAINS):
        view, alpha, s, g, b = chain_view(eng, blocks, d, c)
        V = view(L)
        Z = V.Z(d["T"])
        v0 = her.ystar(d["newY"][:1], d["newX"][:1], g, b)[0] - Z @ (V.Tmat(d["T"] - 1) @ np.asarray(alpha, L))
        F0 = Z @ (V.rqr(d["T"] - 1) * Z) + L(s)
        assert abs(L(got["errors"][c, 0]) - v0) <= 64 * U * np.sqrt(F0), (name, c)
        assert abs(L(got["variances"][c, 0]) - F0) <= 64 * U * F0, (name, c)


# ---- the call observes
@pytest.mark.parametrize("name", ["local level path", "trend+seasonal(4,3,t0=1), T on a boundary", "holiday straddles later steps",
                                  "dynamic regression d=2"])
def test_prefixes_subranges_and_repeats_to_the_bit(name):
    d, blocks = case(name)
    eng = swept(d, blocks, 45)
    full = holdout(eng, d, 130, variances=True)
    std = holdout(eng, d, 130, standardize=True)
    for k in (1, 64):
        part = holdout(eng, d, k, variances=True)
        assert np.array_equal(part["errors"], full["errors"][:, :k]) and np.array_equal(part["variances"], full["variances"][:, :k]), k
        assert np.array_equal(holdout(eng, d, k, standardize=True), std[:, :k]), k
    again = holdout(eng, d, 130, variances=True)
    assert np.array_equal(again["errors"], full["errors"]) and np.array_equal(again["variances"], full["variances"])
    sub = holdout(eng, d, 130, variances=True, chains=(1, 2))
    assert np.array_equal(sub["errors"], full["errors"][1:3]) and np.array_equal(sub["variances"], full["variances"][1:3])
    assert np.array_equal(holdout(eng, d, 130, standardize=True, chains=range(3, 4)), std[3:4])


def chain_image(eng, blocks):
    out = list(eng.get_states())
    for c in range(eng.chains):
        if blocks is None:
            st = eng.ss_get_state(c)
            out += [st["state"], np.array([st["level_sigsq"], st["level_n"], st["level_sumsq"]])]
        else:
            out.append(eng.ss_get_state_draw(c))
            for k in range(len(blocks)):
                m = eng.ss_get_state_model(c, k, suf=False)
                out += [m["variances"]] + ([m["phi"]] if m.get("phi") is not None else [])
    return out


@pytest.mark.parametrize("name", ["local level path", "trend+seasonal(4,3,t0=1), T on a boundary", "dynamic regression d=2"])
def test_purity_against_a_twin_that_never_asks(name):
    d, blocks = case(name)
    a, b = engine(d, blocks, 51), engine(d, blocks, 51)
    a.ss_sweep(3)
    b.ss_sweep(3)
    holdout(a, d, 65, variances=True)
    holdout(a, d, 7, standardize=True, chains=(2, 2))
    for u, v in zip(chain_image(a, blocks), chain_image(b, blocks)):
        assert np.array_equal(u, v)
    assert np.array_equal(a.ss_forecast(d["newX"][:10]), b.ss_forecast(d["newX"][:10]))
    ea, eb = a.ss_prediction_errors(variances=True, log_likelihood=True), b.ss_prediction_errors(variances=True, log_likelihood=True)
    for k in ea:
        assert np.array_equal(ea[k], eb[k]), k
    holdout(a, d, 2)
    a.ss_sweep(1)
    b.ss_sweep(1)
    for u, v in zip(chain_image(a, blocks), chain_image(b, blocks)):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("name", ["local level path", "trend+seasonal(4,3,t0=1), T on a boundary"])
def test_lookahead_8_against_lookahead_1(name):
    d, blocks = case(name)
    a, b = engine(d, blocks, 53), engine(d, blocks, 53)
    a.ss_set_lookahead(8)
    b.ss_set_lookahead(1)
    for _ in range(12):
        a.ss_draw_next()
        b.ss_draw_next()
    ea, eb = holdout(a, d, 65, variances=True), holdout(b, d, 65, variances=True)
    assert np.array_equal(ea["errors"], eb["errors"]) and np.array_equal(ea["variances"], eb["variances"])
    assert np.array_equal(holdout(a, d, 65, standardize=True), holdout(b, d, 65, standardize=True))
    check(a, blocks, d, name + ", look-ahead 8, draw 12", horizons=(65,))


def test_forecast_variance_not_positive():
    """a static intercept (RQR = 0) under sigma^2 = 0: F_0 = 0 on that chain alone"""
    d = series(T0, 37, level=False, intercept=2.0)
    blocks = general_spec(d["y"], [("intercept",)])
    eng = engine(d, blocks, 63)
    eng.ss_sweep(2)
    g, b, s = eng.get_state(2)
    eng.set_state(g, b, 0.0, chain=2)
    before = chain_image(eng, blocks)
    h = 70
    err, var = np.zeros((CHAINS, h)), np.zeros((CHAINS, h))
    nx, ny = np.ascontiguousarray(d["newX"][:h].T).ravel(), d["newY"][:h].copy()
    rc = eng.lib.ba_ss_holdout_prediction_errors(eng._h, 0, CHAINS, 0, h, nx.ctypes.data_as(DP), ny.ctypes.data_as(DP),
                                                 err.ctypes.data_as(DP), var.ctypes.data_as(DP))
    assert rc == -7   # BA_E_FORECAST_VARIANCE
    msg = eng.lib.ba_last_error().decode()
    assert "Found a zero (or negative) forecast variance!" in msg and "(chain 2)" in msg, msg
    assert np.all(np.isnan(err[2])) and np.all(np.isnan(var[2]))
    others = [0, 1, 3]
    assert np.all(np.isfinite(err[others])) and np.all(var[others] > 0)
    for u, v in zip(chain_image(eng, blocks), before):
        assert np.array_equal(u, v)
    # the chain and its status are as they were: with a variance again the engine sweeps and the call serves
    eng.set_state(g, b, s, chain=2)
    eng.ss_sweep(1)
    assert np.all(np.isfinite(holdout(eng, d, h)))


def test_refusals_and_invalid_arguments():
    import student_trend_cases as stc
    import ss_hier_regholiday_cases as shc
    import ss_regholiday_cases as src
    from test_family_forecast_gpu import LISTS as FAMILY_LISTS, family_engine
    nx, ny = np.zeros((5, P)), np.zeros(5)
    for family in ("student", "poisson", "logit"):
        eng, _ = family_engine(family, FAMILY_LISTS["level"], 7, chains=2, warmup=0)
        refused(lambda: eng.ss_holdout_prediction_errors(nx[:, :eng.p], ny),
                "holdout prediction errors are built for the Gaussian observation model only")
    d = series(T0, 33, seasonals=[(4, 1)])
    eng = engine(d, stc.student_trend_spec(d["y"], [("student_trend",), ("seasonal", 4, 1)]), 65)
    refused(lambda: holdout(eng, d, 5), "holdout prediction errors with a Student local linear trend are not defined")
    X, y, obs = src.data(70)
    for extra in (src.models(70), [shc.hier(70)]):
        import boom_amd
        eng = boom_amd.Engine(2, seed=3)
        eng.ss_set_data(y, X, obs)
        pr, _, sig_up = bsts_priors(X, y, 2)
        eng.set_priors(pr["b"], pr["ominv"], pr["pi"], pr["df"], pr["sigma_guess"], sigma_upper_limit=sig_up)
        eng.ss_set_state_models(general_spec(y, [("level",)]) + extra)
        refused(lambda: eng.ss_holdout_prediction_errors(nx, ny), "holdout prediction errors with a regression holiday model are not built")
    # before any state draw
    d, blocks = case("level")
    eng = engine(d, blocks, 67)
    refused(lambda: holdout(eng, d, 5), "no state draw yet")
    eng.ss_sweep(1)
    assert holdout(eng, d, 5).shape == (CHAINS, 5)
    # invalid arguments
    for rng in [(-1, 2), (0, 0), (0, CHAINS + 1), (CHAINS, 1), (3, 2)]:
        refused(lambda: holdout(eng, d, 5, chains=rng), "chain range out of bounds")
    bad = d["newY"][:5].copy()
    bad[3] = np.nan
    refused(lambda: eng.ss_holdout_prediction_errors(d["newX"][:5], bad), "holdout response 3 is not finite")
    bad[3] = np.inf
    refused(lambda: eng.ss_holdout_prediction_errors(d["newX"][:5], bad), "holdout response 3 is not finite")
    out = np.zeros((CHAINS, 5))
    x, yy = np.ascontiguousarray(d["newX"][:5].T).ravel(), d["newY"][:5].copy()
    px, py, po = x.ctypes.data_as(DP), yy.ctypes.data_as(DP), out.ctypes.data_as(DP)
    call = eng.lib.ba_ss_holdout_prediction_errors
    for args, text in [((0, px, py, po), b"the horizon must be positive"), ((-3, px, py, po), b"the horizon must be positive"),
                       ((5, None, py, po), b"null argument"), ((5, px, None, po), b"null argument"), ((5, px, py, None), b"null argument")]:
        assert call(eng._h, 0, CHAINS, 0, *args, None) == -1 and text in eng.lib.ba_last_error(), (args[0], text)
    assert call(eng._h, 0, CHAINS, 0, 5, px, py, po, None) == 0 and np.array_equal(out, holdout(eng, d, 5))
    # a calendar or a predictor table that ends before T + h
    d, blocks = case("holiday covers T")
    blocks[1]["calendar"] = blocks[1]["calendar"][:T0 + 64]
    eng = swept(d, blocks, 69)
    assert holdout(eng, d, 64).shape == (CHAINS, 64)
    refused(lambda: holdout(eng, d, 65), "the holiday calendar of state model 1 has 104 entries: a forecast of horizon 65 needs 105")
    d, blocks = case("dynamic regression d=2")
    blocks[1]["predictors"] = blocks[1]["predictors"][:T0 + 64]
    eng = swept(d, blocks, 69)
    assert holdout(eng, d, 64).shape == (CHAINS, 64)
    refused(lambda: holdout(eng, d, 65), "the predictors of state model 1 have 104 rows: a forecast of horizon 65 needs 105")


def test_pybind_facade():
    import boom_amd
    import boom_amd._boom as boom
    d = series(T0, 17, seasonals=[(4, 1)])
    blocks = general_spec(d["y"], [("trend",), ("seasonal", 4, 1)])
    chains, seed = 3, 71
    pr = d["prior"]
    model = boom.StateSpaceRegressionModel(d["y"], d["X"], [bool(o) for o in d["obs"]], chains=chains, seed=seed)
    b = blocks[0]
    trend = boom.LocalLinearTrendStateModel()
    trend.set_initial_sigma(float(b["initial_sigma"][0]), float(b["initial_sigma"][1]))
    for i in range(2):
        trend.set_prior(i, b["df"][i], b["sigma_guess"][i], b["sigma_upper_limit"][i])
    trend.set_initial_state_mean(b["a0"])
    trend.set_initial_state_variance(b["P0"])
    b = blocks[1]
    seas = boom.SeasonalStateModel(4)
    seas.set_sigsq(float(b["initial_sigma"][0]) ** 2)
    seas.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    seas.set_initial_state_mean(b["a0"])
    seas.set_initial_state_variance(float(b["P0"][0]))
    model.add_state(trend)
    model.add_state(seas)
    model.set_method(boom.StateSpacePosteriorSampler(model, boom.MvnGivenScalarSigma(pr["b"], pr["ominv"]),
                                                     boom.ChisqModel(pr["df"], pr["sigma_guess"]),
                                                     boom.VariableSelectionPrior(pr["pi"]), d["sig_up"]))
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_set_data(d["y"], d["X"], d["obs"])
    eng.set_priors(pr["b"], pr["ominv"], pr["pi"], pr["df"], pr["sigma_guess"], sigma_upper_limit=d["sig_up"])
    eng.ss_set_state_models(blocks)
    eng.set_state(np.zeros(P, np.uint8))
    for _ in range(3):
        model.sample_posterior()
    eng.ss_sweep(3)
    for h in (1, 65):
        got = model.one_step_holdout_prediction_errors(d["newX"][:h], d["newY"][:h])
        assert got.shape == (chains, h) and np.array_equal(got, holdout(eng, d, h))
        assert np.array_equal(model.one_step_holdout_prediction_errors(d["newX"][:h], d["newY"][:h], True),
                              holdout(eng, d, h, standardize=True))
