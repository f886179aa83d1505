"""The Student local linear trend state model on the device (ba_ss_add_state_model kind 8, bsts
AddStudentLocalLinearTrend): the general structural kernel's per-step state variance Q_t (its QT
instances), the weights' kernel and the sampler's kernel (slt_kernel.hip), the round's order.

  identities    the QT instances against the scalar ones, bit for bit: constant weights w are a plain
                local linear trend at sigma^2 / w
  filter edges  one impute_state against the restatement (tests/ss_student_trend_oracle.py): weights
                over six decades, missing steps; the weights drawn after it and their statistics
  the loop      12 x (ba_ss_trend_draw_parameters; ba_ss_impute_state) against the restatement, both
                nu posteriors, a sigma upper limit, a gamma nu prior
  whole rounds  ba_ss_sweep(1) x 12: the state-model half against the restatement given the device's
                regression draw; the regression's statistics; ba_ss_sweep(12) the same draws
  distribution  4096 chains' state draws against the dense Gaussian posterior with Q_t
  interface     refusals and their texts, the accessors
"""
import ctypes as C

import numpy as np
import pytest

import ss_student_oracle as sso
import ss_student_trend_oracle as sto
import student_trend_cases as stc
from cases import bsts_priors, general_data, kernel_instance
from ss_gpu_helpers import refused

gpu = pytest.mark.gpu
RTOL = 1e-8


def relerr(a, b, floor=1e-300):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def engine(chains, seed, y, X, obs, blocks, g0, prior_data=None):
    """prior_data: the (X, y) the regression's bsts priors are made from (default: the data)"""
    import boom_amd
    prior, _, sig_up = bsts_priors(*(prior_data or (X, y)), 2)
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_set_data(y, X, obs)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"],
                   sigma_upper_limit=sig_up)
    eng.ss_set_state_models(blocks)
    eng.ss_set_tuning(kernel=0)   # the general kernel: the one the QT instances are instances of
    eng.set_state(g0)
    return eng


def state_stream(oracle, seed, chain):
    L = oracle.lib
    L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_rnorm.restype = C.c_double
    rng = oracle.rng_philox(seed, chain, 2, 0)
    return lambda mu, sd: L.bo_rnorm(C.byref(rng), float(mu), float(sd))


# ---- identities ------------------------------------------------------------------------------------
ST = ("student_trend",)
# (list, T or None = one step more than a time block, missing fraction, the expected leading dimension)
IDENTITY_LISTS = [
    ([ST], 1, 0.0, 17), ([ST], 2, 0.0, 17), ([ST], 64, 0.0, 17), ([ST], 65, 0.0, 17), ([ST], 131, 0.0, 17),
    ([("seasonal", 4, 1), ST], 70, 0.05, 17),         # the block is not the first
    ([ST, ("seasonal", 20, 1)], None, 0.0, 33),
    ([ST, ("seasonal", 40, 1)], None, 0.0, 61),
    ([ST, ("seasonal", 62, 1)], None, 0.0, 65),
]
TRIG = ("trig", 12.0, [1.0])


def identity_cases():
    out = []
    for desc, T, miss, ld in IDENTITY_LISTS:
        out.append((desc, T, miss, ld))
        g = list(desc) + [TRIG]   # the GLOB instances
        if desc[-1] == ("seasonal", 62, 1):
            # (63 + 2 components would pass the state's 64: two seasons fewer keep the leading dimension 65)
            g = [ST, ("seasonal", 60, 1), TRIG]
        out.append((g, T, miss, ld))
    return out


@gpu
@pytest.mark.parametrize("desc,T,missing,ld", identity_cases())
def test_constant_weights_equal_the_scalar_kernel(desc, T, missing, ld):
    """w = 1, w = 4 and (level 4, slope 1): the same list with a plain local linear trend at sigma^2,
    sigma^2 / 4 and (sigma_level^2 / 4, sigma_slope^2), all exact in binary"""
    p, chains, seed, sigsq = 3, 4, 77, 0.5
    seas = [(b[1], b[2]) for b in desc if b[0] == "seasonal"]
    probe = stc.student_trend_spec(np.arange(8.0), desc)
    m, ld_rule, bl, _ = kernel_instance(probe)
    assert ld_rule == ld
    if T is None:
        T = bl + 1
    n = max(T, 8)   # (the priors' scale is a standard deviation: from eight steps at least)
    X, y, _, obs = general_data(n, p, 2, seas, seed=n + m, missing_frac=missing)
    blocks = stc.student_trend_spec(y, desc)
    full = (X, y)
    X, y, obs = X[:T], y[:T], (None if obs is None else obs[:T])
    gam, beta = stc.chain_parameters(p, chains, 3)
    qt = [i for i, b in enumerate(blocks) if b["kind"] == 8][0]
    for wl, ws in [(1.0, 1.0), (4.0, 4.0), (4.0, 1.0)]:
        a = engine(chains, seed, y, X, obs, blocks, gam[0], full)
        b = engine(chains, seed, y, X, obs, stc.as_plain_trend(blocks, (wl, ws)), gam[0], full)
        for c in range(chains):
            a.set_state(gam[c], beta[c], sigsq, chain=c)
            b.set_state(gam[c], beta[c], sigsq, chain=c)
        a.ss_trend_set_weights(np.full(T, wl), np.full(T, ws))
        a.ss_impute_state()
        b.ss_impute_state()
        for c in range(chains):
            assert np.array_equal(a.ss_get_state_draw(c), b.ss_get_state_draw(c)), (wl, ws, c)
            for k in range(len(blocks)):
                u, v = a.ss_get_state_model(c, k), b.ss_get_state_model(c, k)
                assert np.array_equal(u["suf_n"], v["suf_n"]), (wl, ws, c, k)
                if k != qt:
                    assert np.array_equal(u["suf_ss"], v["suf_ss"]), (wl, ws, c, k)
                elif T > 1:
                    # (the weighted sum against MvnSuf's running form)
                    assert relerr(u["suf_ss"], np.array([wl, ws]) * v["suf_ss"]) < 1e-12, (wl, ws, c)


# ---- filter edges ----------------------------------------------------------------------------------
@gpu
def test_impute_state_matches_restatement_at_the_edges(oracle):
    """weights from 1e-3 to 1e3, different per chain and series; the first step missing and one in the
    second block of 64; then the weights observe_state draws and their statistics (stream 161)"""
    desc, T, p, chains, seed, sigsq = [ST, ("seasonal", 4, 1)], 70, 3, 4, 41, 0.8
    X, y, _, _ = general_data(T, p, 2, [(4, 1)], seed=12)
    obs = np.ones(T, np.uint8)
    obs[[0, 66]] = 0
    blocks = stc.student_trend_spec(y, desc)
    gam, beta = stc.chain_parameters(p, chains, 8)
    eng = engine(chains, seed, y, X, obs, blocks, gam[0])
    rs = np.random.Generator(np.random.PCG64(2))
    W = np.exp(rs.uniform(np.log(1e-3), np.log(1e3), (chains, 2, T)))
    W[:, 0, [1, 65]] = [1e-3, 1e3]
    W[:, 1, [1, 65]] = [1e3, 1e-3]
    for c in range(chains):
        eng.set_state(gam[c], beta[c], sigsq, chain=c)
        eng.ss_trend_set_weights(W[c, 0], W[c, 1], chain=c)
    eng.ss_impute_state()
    for c in range(chains):
        o = sto.StudentTrendOracle(oracle, T, obs, blocks, seed, c)
        o.set_weights(W[c, 0], W[c, 1])
        inc = np.flatnonzero(gam[c])
        want = o.impute_state(y - X[:, inc] @ beta[c][inc], sigsq)
        got = eng.ss_get_state_draw(c)
        err = np.max(np.abs(got - want))
        print("chain %d: state draw max abs error %.3e (max |state| %.3e)" % (c, err, np.abs(want).max()))
        assert err < 1e-8 * np.abs(want).max(), c
        lw, sw = eng.ss_trend_get_weights(c)
        assert relerr(lw, o.w[0]) < RTOL and relerr(sw, o.w[1]) < RTOL, c
        assert lw[-1] == W[c, 0, -1] and sw[-1] == W[c, 1, -1]   # entry T - 1 is never redrawn
        suf = eng.ss_trend_get_weight_suf(c)
        assert suf[0] == T - 1 and suf[3] == T - 1
        assert relerr(suf, o.wsuf, 1e-3) < RTOL, c
        sm = eng.ss_get_state_model(c, 0)
        assert np.array_equal(sm["suf_n"], o.suf_n[0]) and relerr(sm["suf_ss"], o.suf_ss[0]) < RTOL, c


# ---- the regression-free loop ------------------------------------------------------------------------
def check_state_models(eng, o, ch, tag):
    for j in range(len(o.blocks)):
        sm = eng.ss_get_state_model(ch, j)
        nv = len(sm["variances"])
        assert relerr(sm["variances"], o.var[j]) < RTOL, tag + (j,)
        assert np.array_equal(sm["suf_n"], o.suf_n[j][:nv]), tag + (j,)
        assert relerr(sm["suf_ss"], o.suf_ss[j][:nv]) < RTOL, tag + (j,)
        if j == o.qt:
            assert relerr(sm["nu"], o.nu) < RTOL, tag
    lw, sw = eng.ss_trend_get_weights(ch)
    assert relerr(lw, o.w[0]) < RTOL and relerr(sw, o.w[1]) < RTOL, tag
    assert relerr(eng.ss_trend_get_weight_suf(ch), o.wsuf, 1e-3) < RTOL, tag
    st = eng.ss_get_state_draw(ch)
    assert np.max(np.abs(st - o.state)) < 1e-8 * np.abs(o.state).max(), tag


@gpu
@pytest.mark.parametrize("k", range(len(stc.LOOP_CASES)))
def test_parameter_and_state_loop_matches_restatement(oracle, k):
    c = stc.loop_case(k)
    eng = engine(c["chains"], c["seed"], c["y"], c["X"], c["obs"], c["blocks"], c["gam"][0])
    for ch in range(c["chains"]):
        eng.set_state(c["gam"][ch], c["beta"][ch], c["sigsq"], chain=ch)
    ora = {ch: stc.loop_oracle(oracle, c, ch) for ch in c["check"]}
    smax = c["blocks"][0]["sigma_upper_limit"]
    for r in range(c["rounds"]):
        eng.ss_trend_draw_parameters()
        for ch, (o, ystar) in ora.items():
            o.draw_parameters()
            sm = eng.ss_get_state_model(ch, o.qt)
            assert relerr(sm["variances"], o.var[o.qt]) < RTOL and relerr(sm["nu"], o.nu) < RTOL, (k, ch, r)
            assert np.all(sm["variances"] <= smax ** 2)
        eng.ss_impute_state()
        for ch, (o, ystar) in ora.items():
            o.impute_state(ystar, c["sigsq"])
            check_state_models(eng, o, ch, (k, ch, r))
    for ch, (o, _) in ora.items():
        assert o.margin > 1e-9


# ---- whole rounds --------------------------------------------------------------------------------------
@gpu
def test_whole_rounds_match_restatement(oracle):
    T, p, chains, seed, rounds, sig0 = 40, 5, 4, 311, 12, 0.7
    X, y, _, _ = general_data(T, p, 2, [(4, 1)], seed=35)
    rs = np.random.Generator(np.random.PCG64(36))
    y = y + np.cumsum(np.where(rs.uniform(size=T) < 0.1, 4.0 * rs.standard_normal(T), 0.0))
    obs = np.ones(T, np.uint8)
    obs[[7, 22]] = 0
    blocks = stc.student_trend_spec(y, [ST, ("seasonal", 4, 1)], initial_nu=(8.0, 12.0))
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    b0 = np.zeros(p)
    check = [0, chains - 1]

    def fresh():
        e = engine(chains, seed, y, X, obs, blocks, g0)
        e.ss_set_tuning(kernel=1)   # (the default choice: a Student trend never takes the shape-specialised kernel)
        e.set_state(g0, b0, sig0)
        return e

    eng = fresh()
    ora = {ch: sto.StudentTrendOracle(oracle, T, obs, blocks, seed, ch) for ch in check}
    for o in ora.values():
        o.impute_state(y - X @ b0, sig0)   # the first call's impute_state, with the parameters as they stand
    ob = obs.astype(bool)
    for r in range(rounds):
        eng.ss_sweep(1)
        gam, beta, sig = eng.get_states()
        for ch, o in ora.items():
            # the state-model half, given the device's regression draw of this round
            o.draw_state_models()
            o.impute_state(y - X @ (beta[ch] * gam[ch]), sig[ch])
            check_state_models(eng, o, ch, (ch, r))
            # the regression's statistics of the device's own state draw
            e = np.where(ob, y - eng.ss_get_state_draw(ch) @ o.S.Z, 0.0)
            suf = eng.ss_get_chain_suf(ch)
            assert relerr(suf["xty"], X.T @ e, 1e-6) < RTOL and relerr(suf["yty"], e @ e) < RTOL, (ch, r)
            assert suf["n"] == ob.sum()
    for o in ora.values():
        assert o.margin > 1e-9
    eng2 = fresh()
    eng2.ss_sweep(rounds)
    for u, v in zip(eng.get_states(), eng2.get_states()):
        assert np.array_equal(u, v)
    for ch in range(chains):
        assert np.array_equal(eng.ss_get_state_draw(ch), eng2.ss_get_state_draw(ch))
        for a, b in zip(eng.ss_trend_get_weights(ch), eng2.ss_trend_get_weights(ch)):
            assert np.array_equal(a, b)
        u, v = eng.ss_get_state_model(ch, 0), eng2.ss_get_state_model(ch, 0)
        assert all(np.array_equal(u[key], v[key]) for key in u)


# ---- distribution --------------------------------------------------------------------------------------
@gpu
def test_state_draws_have_the_dense_posterior_moments():
    T, chains, sigsq = 12, 4096, 0.6
    rs = np.random.Generator(np.random.PCG64(5))
    y = np.cumsum(rs.standard_normal(T)) + 3.0
    blocks = stc.student_trend_spec(y, [ST])
    blocks[0]["initial_sigma"] = np.array([0.55, 0.22])
    obs = np.ones(T, np.uint8)
    obs[7] = 0
    W = np.exp(rs.uniform(np.log(1e-2), np.log(1e2), (2, T)))   # four decades
    X = np.ones((T, 1))
    g0 = np.zeros(1, np.uint8)
    eng = engine(chains, 20263, y, X, obs, blocks, g0)
    eng.set_state(g0, np.zeros(1), sigsq)
    eng.ss_trend_set_weights(W[0], W[1])
    eng.ss_impute_state()
    draws = np.stack([eng.ss_get_state_draw(c).reshape(-1) for c in range(chains)])
    S = sto.TrendStructure(blocks, T)
    S.w = W
    mean, cov = sso.dense_posterior(S, [blocks[0]["initial_sigma"] ** 2], y, obs.astype(bool), np.full(T, sigsq))
    d = len(mean)
    bound = sso.bonferroni_bound(d + d * (d + 1) // 2)   # (level 1e-3, fixed with the seed before any run)
    zm, zc = sso.moment_z(draws, mean, cov)
    print("largest |z|: mean %.3f covariance %.3f, bound %.3f" % (np.abs(zm).max(), np.abs(zc).max(), bound))
    assert np.abs(zm).max() < bound
    assert np.abs(zc).max() < bound


# ---- interface -------------------------------------------------------------------------------------------
@gpu
def test_refusals_and_their_texts():
    import boom_amd
    T, p = 30, 3
    X, y, _, _ = general_data(T, p, 1, [], seed=2)
    blocks = stc.student_trend_spec(y, [ST, ("seasonal", 4, 1)])
    g0 = np.zeros(p, np.uint8)
    # a second Student trend
    eng = boom_amd.Engine(2, seed=1)
    eng.ss_set_data(y, X, None)
    refused(lambda: eng.ss_set_state_models(stc.student_trend_spec(y, [ST, ST])),
            "at most one Student local linear trend per list of state models")
    # initial nu: not positive, outside the uniform prior's support
    for nu0 in [(0.0, 5.0), (5.0, -1.0), (0.5, 5.0), (5.0, 600.0), (np.nan, 5.0)]:
        refused(lambda: eng.ss_set_state_models(stc.student_trend_spec(y, [ST], initial_nu=nu0)),
                "the initial nu must be positive and have positive prior density")
    # the trend's entry points on a list without one
    from cases import general_spec
    eng.ss_set_state_models(general_spec(y, [("trend",)]))
    refused(lambda: eng.ss_trend_draw_parameters(), "the list of state models holds no Student local linear trend")
    refused(lambda: eng.ss_trend_get_weights(0), "the list of state models holds no Student local linear trend")
    eng = engine(2, 1, y, X, None, blocks, g0)
    # weights
    for bad in (0.0, -1.0, np.nan, np.inf):
        w = np.ones(T)
        w[4] = bad
        refused(lambda: eng.ss_trend_set_weights(w, np.ones(T)), "Weights must be finite and positive.")
        refused(lambda: eng.ss_trend_set_weights(np.ones(T), w), "Weights must be finite and positive.")
    eng.ss_sweep(2)
    lw, sw = eng.ss_trend_get_weights(1)
    assert np.all(lw[:-1] != 1.0) and lw[-1] == 1.0 and sw[-1] == 1.0
    sm = eng.ss_get_state_model(0, 0)
    assert sm["suf_n"][0] == T - 1 and np.all(sm["nu"] >= 1.0) and np.all(sm["nu"] <= 500.0)
    # forecasts and the look-ahead
    refused(lambda: eng.ss_forecast(np.zeros((2, p))), "forecasts with a Student local linear trend are not implemented")
    refused(lambda: eng.ss_set_lookahead(4), "the look-ahead does not carry a Student local linear trend's weights")
    eng.ss_set_lookahead(1)
    eng.ss_draw_next()
    # the other observation families
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.5)
    text = "the Student local linear trend is built for the Gaussian observation model only"
    e2 = boom_amd.Engine(2, seed=1)
    e2.ss_student_set_data(y, X, None)
    refused(lambda: e2.ss_set_state_models(blocks), text)
    # ... and the list first, the family's data after it
    e3 = boom_amd.Engine(2, seed=1)
    e3.ss_set_data(y, X, None)
    e3.ss_set_state_models(blocks)
    e3.ss_student_set_data(y, X, None)
    e3.sss_set_slab(mu, prec, scales_with_sigsq=True)
    e3.set_spike(pi)
    e3.set_sigma_prior(1.0, 1.0)
    e3.set_state(g0)
    refused(lambda: e3.ss_student_sweep(1), text)


@gpu
def test_pybind_classes_agree_with_the_c_abi():
    """boom.StudentLocalLinearTrendStateModel in a StateSpaceRegressionModel (the façade of
    include/boom_amd.hpp behind it): three rounds == the engine through the C-ABI on the same seed, bit
    for bit"""
    import boom_amd._boom as boom
    T, p, chains, seed = 40, 4, 3, 23
    X, y, _, obs = general_data(T, p, 2, [(4, 1)], seed=6, missing_frac=0.05)
    nu_priors = ((0, 1.0, 500.0), (1, 2.0, 0.1))
    blocks = stc.student_trend_spec(y, [ST, ("seasonal", 4, 1)], nu_priors, (6.0, 20.0))
    prior, _, sig_up = bsts_priors(X, y, 2)
    model = boom.StateSpaceRegressionModel(y, X, [bool(o) for o in obs], chains=chains, seed=seed)
    b = blocks[0]
    trend = boom.StudentLocalLinearTrendStateModel(float(b["initial_sigma"][0]), 6.0, float(b["initial_sigma"][1]), 20.0)
    for i in range(2):
        trend.set_prior(i, b["df"][i], b["sigma_guess"][i], b["sigma_upper_limit"][i])
        trend.set_nu_prior(i, *nu_priors[i])
    trend.set_initial_state_mean(b["a0"])
    trend.set_initial_state_variance(b["P0"])
    b = blocks[1]
    seas = boom.SeasonalStateModel(4)
    seas.set_sigsq(b["initial_sigma"][0] ** 2)
    seas.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    seas.set_initial_state_mean(b["a0"])
    seas.set_initial_state_variance(b["P0"][0])
    model.add_state(trend)
    model.add_state(seas)
    sampler = boom.StateSpacePosteriorSampler(model, boom.MvnGivenScalarSigma(prior["b"], prior["ominv"]),
                                              boom.ChisqModel(prior["df"], prior["sigma_guess"]),
                                              boom.VariableSelectionPrior(prior["pi"]), sig_up)
    model.set_method(sampler)
    assert model.state_dimension == 5
    import boom_amd
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_set_data(y, X, obs)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"], sigma_upper_limit=sig_up)
    eng.ss_set_state_models(blocks)
    eng.set_state(np.zeros(p, np.uint8))
    for _ in range(3):
        model.sample_posterior()
        eng.ss_sweep(1)
    for u, v in zip(model.chain_states(), eng.get_states()):
        assert np.array_equal(u, v)
    for c in range(chains):
        sm = eng.ss_get_state_model(c, 0)
        assert np.array_equal(model.student_trend_nu(c), sm["nu"])
        assert np.array_equal(model.state_variances(c)[:2], sm["variances"])
        assert np.array_equal(model.student_trend_weights(c), np.stack(eng.ss_trend_get_weights(c)))
        assert np.array_equal(model.state(c), eng.ss_get_state_draw(c).T)
