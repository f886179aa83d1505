"""ba_ss_prediction_errors (bsts's one.step.prediction.errors and log.likelihood) on the device
against the dense long-double filter of tests/prediction_errors_ref.py, at exactly the
parameters the accessors report: before any sweep and after three, for every kind of state
model, the local-level path, the Student trend's per-step variances and the state-dimension
edges.  The gate of each comparison comes from the reference alone (reference_and_gate: float64
against long double in both algebraic forms, times 8, at least 64 u); the worst device-to-gate
ratio of each case is printed.  Then what makes the call an observer: sub-ranges and repeats to
the bit, purity, the look-ahead served from the record without a replay, the refusals and the
forecast variance that is not positive.

Worst device / gate ratios measured on an MI355X (v, v / sqrt F, F, log likelihood):
see DESIGN.md section 3.19."""
import ctypes as C

import numpy as np
import pytest

import prediction_errors_ref as per
import student_trend_cases as stc
from cases import bsts_priors, general_data, general_spec

pytestmark = pytest.mark.gpu
CHAINS, P = 5, 3


def series(T, seed, seasonals=(), missing=(), **kw):
    """T steps of a series whose priors come from 40 steps of it (a series of one or two steps has
    no standard deviation)"""
    X, y, _, _ = general_data(max(T, 40), P, 2, list(seasonals), seed=seed, **kw)
    prior, ss, sig_up = bsts_priors(X, y, 2)
    obs = np.ones(T, np.uint8)
    obs[list(missing)] = 0
    return dict(X=np.ascontiguousarray(X[:T]), y=np.ascontiguousarray(y[:T]), obs=obs, prior=prior, ss=ss, sig_up=sig_up,
                full_y=y)


def chain_start(seed):
    """chain 1 has all coefficients excluded, chain 2 one"""
    rs = np.random.Generator(np.random.PCG64(seed))
    gam = np.ones((CHAINS, P), np.uint8)
    gam[1] = 0
    gam[2, 1] = 0
    return gam, rs.standard_normal((CHAINS, P)) * gam, rs.uniform(0.3, 1.5, CHAINS)


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
        eng.ss_set_state_models(blocks)
    gam, beta, sig = chain_start(seed + 1)
    for c in range(chains):
        eng.set_state(gam[c % CHAINS], beta[c % CHAINS], float(sig[c % CHAINS]), chain=c)
    return eng


LEVEL_BLOCK = lambda ss: [dict(kind=1, a0=[ss["initial_state_mean"]], P0=[ss["initial_state_variance"]],
                               initial_sigma=[ss["initial_level_sigma"]])]


def chain_params(eng, blocks, d, c):
    """what the accessors report for chain c, in the reference's form: (blocks, params, sigsq, gamma, beta)"""
    g, b, s = eng.get_state(c)
    if blocks is None:
        ref_blocks = LEVEL_BLOCK(d["ss"])
        params = [dict(var=np.array([eng.ss_get_state(c, state=False, suf=False)["level_sigsq"]]), phi=None)]
        return ref_blocks, params, s, g, b
    params = []
    for k, blk in enumerate(blocks):
        m = eng.ss_get_state_model(c, k, suf=False)
        q = dict(var=m["variances"], phi=m.get("phi"))
        if blk["kind"] == per.STUDENT_TREND:
            q["weights"] = eng.ss_trend_get_weights(c)
        params.append(q)
    return blocks, params, s, g, b


def check(eng, blocks, d, label):
    """every output of every chain within the gate; sub-range and repeat to the bit; returns the worst ratio"""
    full = eng.ss_prediction_errors(variances=True, log_likelihood=True)
    std = eng.ss_prediction_errors(standardize=True)
    assert full["errors"].shape == (CHAINS, eng.T) and std.shape == (CHAINS, eng.T)
    worst = {}
    for c in range(CHAINS):
        rb, params, s, g, b = chain_params(eng, blocks, d, c)
        ref, gate = per.reference_and_gate(rb, params, s, d["y"], d["X"], g, b, d["obs"])
        dev = per.device_deviation(ref, full["errors"][c], full["variances"][c], std[c], full["log_likelihood"][c])
        miss = d["obs"] == 0
        assert np.all(full["errors"][c][miss] == 0) and np.all(std[c][miss] == 0)
        for k, v in dev.items():
            r = v / gate["v" if k == "std" else k]
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= 1.0, (label, c, k, v, gate)
    print("%s: worst device / gate  v %.3f  std %.3f  F %.3f  loglik %.3f" %
          (label, worst["v"], worst["std"], worst["F"], worst["loglik"]))
    again = eng.ss_prediction_errors(variances=True, log_likelihood=True)
    for k in full:
        assert np.array_equal(full[k], again[k]), (label, k)
    if CHAINS >= 4:
        sub = eng.ss_prediction_errors(chains=(1, 3), variances=True, log_likelihood=True)
        for k in full:
            assert np.array_equal(sub[k], full[k][1:4]), (label, k)
    return worst


def both_points(d, blocks, seed, label, prepare=None):
    eng = engine(d, blocks, seed)
    if prepare:
        prepare(eng)
    check(eng, blocks, d, label + ", before any sweep")
    eng.ss_sweep(3)
    check(eng, blocks, d, label + ", after 3 sweeps")


# ---- case 1: the local level through ba_ss_set_local_level
@pytest.mark.parametrize("T,missing", [(1, ()), (2, (0,)), (40, (0, 17, 18, 39))])
def test_local_level_path(T, missing):
    both_points(series(T, 11, missing=missing), None, 21, "local level path T=%d" % T)


# ---- cases 2-8: every kind of state model, T = 29
LISTS = {
    "level": ([("level",)], {}),
    "trend": ([("trend",)], {}),
    "trend+seasonal(4,3,t0=1)": ([("trend",), ("seasonal", 4, 3, 1)], dict(seasonals=[(4, 3)])),
    "ar3": ([("ar", 3, [0.5, -0.2, 0.1])], dict(level=False, ar_coef=[0.5, -0.2, 0.1])),
    "level+ar1": ([("level",), ("ar", 1, [0.6])], dict(ar_coef=[0.6])),
    "intercept+trig": ([("intercept",), ("trig", 7.0, [1.0, 2.0])], dict(level=False, trig=[(7.0, [1.0, 2.0])], intercept=2.0)),
    "semilocal+seasonal7": ([("semilocal",), ("seasonal", 7, 1)], dict(seasonals=[(7, 1)])),
}


@pytest.mark.parametrize("name", list(LISTS))
def test_every_state_model_kind(name):
    desc, kw = LISTS[name]
    d = series(29, 31, missing=(5, 6, 28), **kw)
    both_points(d, general_spec(d["full_y"], desc), 41, name)


# ---- case 9: the Student trend's per-step variances
def test_student_trend_weights():
    T = 29
    d = series(T, 33, seasonals=[(4, 1)], missing=(9,))
    blocks = stc.student_trend_spec(d["full_y"], [("student_trend",), ("seasonal", 4, 1)])

    def weights(eng):
        rs = np.random.Generator(np.random.PCG64(5))
        for c in range(CHAINS):
            eng.ss_trend_set_weights(10.0 ** rs.uniform(-2, 2, T), 10.0 ** rs.uniform(-2, 2, T), chain=c)
    both_points(d, blocks, 43, "student trend+seasonal4", prepare=weights)


# ---- cases 10, 11: the state-dimension edges
@pytest.mark.parametrize("m", [16, 17, 32, 33, 64])
def test_state_dimension_edges(m):
    if m == 64:
        desc = [("trend",), ("seasonal", 53, 1), ("ar", 10, [0.3, 0.1] + [0.0] * 8)]
        kw = dict(seasonals=[(53, 1)], ar_coef=[0.3, 0.1])
    else:
        desc = [("trend",), ("seasonal", m - 1, 1)]
        kw = dict(seasonals=[(m - 1, 1)])
    d = series(70, 35, missing=(0, 30, 31, 69), **kw)
    blocks = general_spec(d["full_y"], desc)
    assert sum(per.block_dim(b) for b in blocks) == m
    both_points(d, blocks, 45, "m=%d" % m)


# ---- the call observes
def chain_image(eng, blocks):
    out = list(eng.get_states())
    for c in range(CHAINS):
        if blocks is None:
            st = eng.ss_get_state(c)
            out += [st["state"], np.array([st["level_sigsq"], st["level_n"], st["level_sumsq"]])]
        else:
            out.append(eng.ss_get_state_draw(c))
            for k in range(len(blocks)):
                m = eng.ss_get_state_model(c, k, suf=False)
                out += [m["variances"]] + ([m["phi"]] if m.get("phi") is not None else [])
    return out


@pytest.mark.parametrize("which", ["local level path", "trend+seasonal+ar"])
def test_purity(which):
    d = series(40, 13, seasonals=[(4, 1)], missing=(7,), ar_coef=[0.5])
    blocks = None if which == "local level path" else general_spec(d["full_y"], [("trend",), ("seasonal", 4, 1), ("ar", 2)])
    a, b = engine(d, blocks, 51), engine(d, blocks, 51)
    a.ss_sweep(2)
    a.ss_prediction_errors(variances=True, log_likelihood=True)
    a.ss_prediction_errors(standardize=True, chains=(2, 2))
    a.ss_sweep(2)
    b.ss_sweep(4)
    for u, v in zip(chain_image(a, blocks), chain_image(b, blocks)):
        assert np.array_equal(u, v)


def lookahead_pair(which, seed):
    d = series(40, 15, seasonals=[(4, 1)], missing=(3,))
    blocks = None if which == "local level path" else general_spec(d["full_y"], [("trend",), ("seasonal", 4, 1)])
    return d, blocks, engine(d, blocks, seed), engine(d, blocks, seed)


@pytest.mark.parametrize("which", ["local level path", "trend+seasonal"])
def test_lookahead_serves_the_recorded_draw(which):
    d, blocks, a, b = lookahead_pair(which, 53)
    a.ss_set_lookahead(8)
    b.ss_set_lookahead(1)
    for it in range(12):
        a.ss_draw_next()
        b.ss_draw_next()
        ea = a.ss_prediction_errors(variances=True, log_likelihood=True)
        eb = b.ss_prediction_errors(variances=True, log_likelihood=True)
        for k in ea:
            assert np.array_equal(ea[k], eb[k]), (it, k)
        assert np.array_equal(a.ss_prediction_errors(standardize=True), b.ss_prediction_errors(standardize=True)), it
    # ... and it is the filter of what the accessors report at that draw
    check(a, blocks, d, which + ", look-ahead 8, draw 12")


def test_no_replay_under_the_lookahead():
    d, blocks, a, b = lookahead_pair("trend+seasonal", 55)
    for e in (a, b):
        e.ss_set_lookahead(8)
        e.set_kernel_timing(True, overlap=True)
    for it in range(12):
        a.ss_draw_next()
        a.ss_prediction_errors(log_likelihood=True)
        a.get_state(0)
        b.ss_draw_next()
        b.get_state(0)
    ta, tb = a.kernel_times(), b.kernel_times()
    assert ta.pop("ss_filter_kernel")[1] == 12 and "ss_filter_kernel" not in tb
    assert {k: v[1] for k, v in ta.items()} == {k: v[1] for k, v in tb.items()}
    assert sum(v[1] for v in tb.values()) > 0


def test_refusals():
    from test_family_forecast_gpu import LISTS as FAMILY_LISTS, family_engine
    from ss_gpu_helpers import refused
    text = "one-step prediction errors are built for the Gaussian observation model only"
    for family in ("student", "poisson", "logit"):
        eng, _ = family_engine(family, FAMILY_LISTS["level"], 7, chains=2, warmup=0)
        refused(lambda: eng.ss_prediction_errors(), text)
    d = series(29, 31)
    eng = engine(d, general_spec(d["full_y"], [("level",)]), 61)
    for rng in [(-1, 2), (0, 0), (0, CHAINS + 1), (CHAINS, 1), (3, 3)]:
        refused(lambda: eng.ss_prediction_errors(chains=rng), "chain range out of bounds")
    rc = eng.lib.ba_ss_prediction_errors(eng._h, 0, CHAINS, 0, None, None, None)
    assert rc == -1 and b"null argument" in eng.lib.ba_last_error()
    # (one output is enough)
    ll = np.zeros(CHAINS)
    assert eng.lib.ba_ss_prediction_errors(eng._h, 0, CHAINS, 0, None, None, ll.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert np.all(np.isfinite(ll)) and np.all(ll != 0)


def test_forecast_variance_not_positive():
    """a static intercept with initial variance 0 under sigma^2 = 0: F_0 = 0 on that chain alone"""
    d = series(29, 37, level=False, intercept=2.0)
    blocks = general_spec(d["full_y"], [("intercept",)])
    blocks[0]["P0"] = np.zeros(1)
    eng = engine(d, blocks, 63)
    g, b, _ = eng.get_state(2)
    eng.set_state(g, b, 0.0, chain=2)
    err, var, ll = np.zeros((CHAINS, eng.T)), np.zeros((CHAINS, eng.T)), np.zeros(CHAINS)
    dp = C.POINTER(C.c_double)
    rc = eng.lib.ba_ss_prediction_errors(eng._h, 0, CHAINS, 0, err.ctypes.data_as(dp), var.ctypes.data_as(dp), ll.ctypes.data_as(dp))
    assert rc == -7   # BA_E_FORECAST_VARIANCE
    msg = eng.lib.ba_last_error().decode()
    assert "Found a zero (or negative) forecast variance!" in msg and "(chain 2)" in msg, msg
    assert np.all(np.isnan(err[2])) and np.all(np.isnan(var[2])) and np.isnan(ll[2])
    others = [0, 1, 3, 4]
    assert np.all(np.isfinite(err[others])) and np.all(var[others] > 0) and np.all(np.isfinite(ll[others]))
    # the chain and its status are as they were: with a variance again the engine sweeps
    eng.set_state(g, b, 1.0, chain=2)
    eng.ss_sweep(2)
    assert np.all(np.isfinite(eng.ss_prediction_errors()))


def test_pybind_methods():
    import boom_amd._boom as boom
    d = series(40, 17, seasonals=[(4, 1)], missing=(4,))
    blocks = general_spec(d["full_y"], [("trend",), ("seasonal", 4, 1)])
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
    import boom_amd
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_set_data(d["y"], d["X"], d["obs"])
    eng.set_priors(pr["b"], pr["ominv"], pr["pi"], pr["df"], pr["sigma_guess"], sigma_upper_limit=d["sig_up"])
    eng.ss_set_state_models(blocks)
    eng.set_state(np.zeros(P, np.uint8))
    for _ in range(3):
        model.sample_posterior()
    eng.ss_sweep(3)
    want = eng.ss_prediction_errors(variances=True, log_likelihood=True)
    got = model.one_step_prediction_errors()
    assert got.shape == (eng.T, chains) and np.array_equal(got, want["errors"].T)
    assert np.array_equal(model.one_step_prediction_errors(True), eng.ss_prediction_errors(standardize=True).T)
    assert np.array_equal(model.log_likelihood(), want["log_likelihood"])
