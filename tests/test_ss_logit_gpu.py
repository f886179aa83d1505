"""bsts family = "logit" on the device (ba_ss_logit_*): StateSpaceLogitModel with
StateSpaceLogitPosteriorSampler -- the general structural kernel on every chain's own latent
series v_t with the per-step observation variance H_t = 1 / q_t, the binomial auxiliary-mixture
imputation at eta_t = Z_t'alpha_t + x_t'beta over the observed steps, the round's order.

  identity      the state draw on latent data set the same in every chain against the Gaussian
                engine's on y = v, bit for bit
  fresh engine  a new model is v = 0, q = 4 / n_t: with n_t = 2 the first impute_state is the
                Gaussian engine's at sigma^2 = 1/2, bit for bit
  filter edges  one impute_state against the restatement (tests/ss_logit_oracle.py): values and
                precisions of every chain's own, precisions over six decades, missing steps with
                H = pi^2 / 3
  whole rounds  against the restatement on the same substreams: inclusion indicators bit-exact;
                beta, v, q, the state models' variances and statistics within 1e-8 relative, the
                state within 1e-8 of its largest magnitude (the bars of tests/test_ss_poisson_gpu.py)
  distribution  4096 chains' state draws against the dense Gaussian posterior
  interface     refusals and their texts, recorded draws, ba_get_state, the pybind classes
  recovery      the summaries find the two predictors the success probability depends on
"""
import numpy as np
import pytest

import ss_logit_oracle as slo
import ss_poisson_oracle as spo
from cases import bsts_priors, general_data, general_spec
from test_ss_student_gpu import chain_parameters, gaussian_engine, refused, relerr, state_stream

gpu = pytest.mark.gpu
RTOL = 1e-8


def slab_of(p, expected=2.5):
    return np.zeros(p), np.eye(p), np.full(p, min(0.9, expected / p))


def binomial_series(T, p, seed, max_trials=1, coef=(0.8, -0.6), seasons=0, with_path=False, fixed_trials=0):
    """successes from a known logit path (a random walk, X beta, a seasonal pattern) at 1 ..
    max_trials trials per step (fixed_trials: that many at every step); returns X, successes,
    trials and the empirical logit log((y + 1/2) / (n - y + 1/2)), which sizes the state priors
    (with_path: the state's part of the logit too)"""
    rs = np.random.Generator(np.random.PCG64(seed))
    X = rs.standard_normal((T, p))
    beta = np.zeros(p)
    beta[:len(coef)] = coef
    path = -0.3 + np.cumsum(0.05 * rs.standard_normal(T))
    if seasons:
        pattern = 0.4 * rs.standard_normal(seasons)
        path = path + (pattern - pattern.mean())[np.arange(T) % seasons]
    trials = (np.full(T, fixed_trials) if fixed_trials else rs.integers(1, max_trials + 1, T)).astype(float)
    successes = rs.binomial(trials.astype(int), 1 / (1 + np.exp(-(path + X @ beta)))).astype(float)
    series = np.log((successes + 0.5) / (trials - successes + 0.5))
    if with_path:
        return X, successes, trials, series, path
    return X, successes, trials, series


def spec(series, desc, upper=np.inf):
    blocks = general_spec(series, desc)
    for b in blocks:
        b["sigma_upper_limit"] = np.full(len(b["sigma_upper_limit"]), float(upper))
    return blocks


def logit_engine(chains, seed, successes, trials, X, obs, blocks, g0, pi=None, max_flips=-1, clt=5):
    import boom_amd
    p = X.shape[1]
    mu, prec, pi0 = slab_of(p)
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_logit_set_data(successes, trials, X, obs, clt_threshold=clt)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=False, max_flips=max_flips)
    eng.set_spike(pi0 if pi is None else pi)
    eng.ss_set_state_models(blocks)
    eng.set_state(g0)
    return eng


def same_state_and_statistics(a, b, chains, blocks, tag):
    for c in range(chains):
        assert np.array_equal(a.ss_get_state_draw(c), b.ss_get_state_draw(c)), tag + (c,)
        for k in range(len(blocks)):
            u, w = a.ss_get_state_model(c, k), b.ss_get_state_model(c, k)
            assert np.array_equal(u["suf_ss"], w["suf_ss"]) and np.array_equal(u["suf_n"], w["suf_n"]), tag + (c, k)


# ---- 1. identity ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("desc,T,missing", [
    ([("trend",), ("seasonal", 4, 1)], 70, 0.05),     # a 64-step block boundary, a partial last block
    ([("trend",), ("seasonal", 4, 1)], 70, 0.0),
    ([("level",), ("seasonal", 20, 1)], 70, 0.05),    # m = 20 > 16: blocks of 32 steps
    ([("level",), ("seasonal", 20, 1)], 70, 0.0),
])
def test_shared_latent_data_equal_the_scalar_kernel(desc, T, missing):
    """q = 1: the Gaussian engine's impute_state on y = v at sigma^2 = 1, bit for bit; then q = 4:
    at sigma^2 = 1/4 (exact in binary)"""
    p, chains, seed = 3, 4, 77
    seas = [(b[1], b[2]) for b in desc if b[0] == "seasonal"]
    X, v, _, obs = general_data(T, p, 2, seas, seed=T, missing_frac=missing)
    blocks = general_spec(v, desc)
    gam, beta = chain_parameters(p, chains, 3)
    successes, trials = np.zeros(T), np.ones(T)
    for q in (1.0, 4.0):
        a = logit_engine(chains, seed, successes, trials, X, obs, blocks, gam[0])
        b = gaussian_engine(chains, seed, v, X, obs, blocks, gam[0])
        for c in range(chains):
            a.set_state(gam[c], beta[c], 1.0, chain=c)
            b.set_state(gam[c], beta[c], 1.0 / q, chain=c)
        a.ss_logit_set_latent(v, np.full(T, q))
        a.ss_logit_impute_state()
        b.ss_impute_state()
        same_state_and_statistics(a, b, chains, blocks, (q,))


@gpu
def test_a_fresh_engine_starts_from_four_over_the_trials():
    """a new model: v = 0 and q = 4 / n_t, here 2 at every observed step (exact in binary) and 0
    at the missing ones; the first impute_state is the Gaussian engine's on y = 0 at sigma^2 = 1/2"""
    import boom_amd
    desc, T, p, chains, seed = [("trend",), ("seasonal", 4, 1)], 70, 3, 4, 78
    X, y, _, obs = general_data(T, p, 2, [(4, 1)], seed=5, missing_frac=0.05)
    assert 0 < (obs == 0).sum() < T
    blocks = general_spec(y, desc)
    gam, beta = chain_parameters(p, chains, 4)
    a = logit_engine(chains, seed, np.ones(T), np.full(T, 2.0), X, obs, blocks, gam[0])
    ob = obs.astype(bool)
    for c in range(chains):
        v, q = a.ss_logit_get_latent(c)
        assert np.all(v == 0.0) and np.array_equal(q, np.where(ob, 2.0, 0.0))
    # (the Gaussian engine's priors are sized on y; its series is the new model's v = 0)
    prior, _, sig_up = bsts_priors(X, y, 2)
    b = boom_amd.Engine(chains, seed=seed)
    b.ss_set_data(np.zeros(T), X, obs)
    b.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"], sigma_upper_limit=sig_up)
    b.ss_set_state_models(blocks)
    b.ss_set_tuning(kernel=0)
    b.set_state(gam[0])
    for c in range(chains):
        a.set_state(gam[c], beta[c], 1.0, chain=c)
        b.set_state(gam[c], beta[c], 0.5, chain=c)
    a.ss_logit_impute_state()
    b.ss_impute_state()
    same_state_and_statistics(a, b, chains, blocks, ())


# ---- 2. filter edges -----------------------------------------------------------------------------
@gpu
def test_impute_state_matches_restatement_on_every_chains_own_series(oracle):
    """values and precisions that differ from chain to chain, precisions from 1e-3 to 1e3, the
    first step and a step of the second block of 64 missing (H = pi^2 / 3 there)"""
    desc, T, p, chains, seed = [("trend",), ("seasonal", 4, 1)], 70, 3, 4, 41
    X, y, _, _ = general_data(T, p, 2, [(4, 1)], seed=12)
    obs = np.ones(T, np.uint8)
    obs[[0, 66]] = 0
    blocks = general_spec(y, desc)
    gam, beta = chain_parameters(p, chains, 8)
    eng = logit_engine(chains, seed, np.zeros(T), np.ones(T), X, obs, blocks, gam[0])
    rs = np.random.Generator(np.random.PCG64(2))
    V = y[None, :] + rs.standard_normal((chains, T))
    Q = np.exp(rs.uniform(np.log(1e-3), np.log(1e3), (chains, T)))
    Q[:, [1, 65]] = [1e-3, 1e3]
    for c in range(chains):
        eng.set_state(gam[c], beta[c], 1.0, chain=c)
        eng.ss_logit_set_latent(V[c], Q[c], chain=c)
    eng.ss_logit_impute_state()
    S = slo.Structure(blocks)
    var = [np.asarray(b["initial_sigma"], float) ** 2 for b in blocks]
    ob = obs.astype(bool)
    for c in range(chains):
        H = slo.observation_variances(Q[c], ob)
        assert H[0] == slo.MISSING_VARIANCE and H[66] == H[0] and abs(H[0] - np.pi ** 2 / 3) < 1e-15
        inc = np.flatnonzero(gam[c])
        want = slo.impute_state(S, var, V[c] - X[:, inc] @ beta[c][inc], ob, H, state_stream(oracle, seed, c))
        got = eng.ss_get_state_draw(c)
        assert np.max(np.abs(got - want)) < 1e-8 * np.abs(want).max(), c
        n, ss = slo.state_model_suf(S, want)
        for k in range(len(blocks)):
            sm = eng.ss_get_state_model(c, k)
            nv = len(sm["variances"])
            assert np.array_equal(sm["suf_n"], n[k][:nv]), (c, k)
            assert relerr(sm["suf_ss"], ss[k][:nv], 1e-300) < RTOL, (c, k)
        v, q = eng.ss_logit_get_latent(c)
        assert np.array_equal(v, np.where(ob, V[c], 0.0)) and np.array_equal(q, np.where(ob, Q[c], 0.0)), c


# ---- 3. whole rounds -----------------------------------------------------------------------------
ROUND_CASES = [
    # blocks, T, rounds, largest number of trials, missing steps, slot limit, seed
    ([("level",)], 40, 12, 1, [], 0, 57),                               # Bernoulli
    ([("trend",), ("seasonal", 4, 1)], 40, 12, 4, [5, 23], 0, 58),
    ([("level",)], 40, 12, 40, [], 0, 59),     # both branches in one series (clt_threshold 5); n min(p, q) <= 20: no BTPE
    ([("level",)], 300, 3, 4, [], 0, 60),      # two workgroups of the imputation, five blocks of 64 steps
    ([("level",)], 40, 12, 4, [7], 2, 61),     # a slot serves 2 uniforms: the imputation reads its spill streams
]
CLT = 5


def round_case(k):
    desc, T, rounds, max_trials, miss, slots, seed = ROUND_CASES[k]
    p, chains = 5, 4
    seasons = max([b[1] for b in desc if b[0] == "seasonal"], default=0)
    X, successes, trials, series = binomial_series(T, p, 31 + k, max_trials=max_trials, seasons=seasons)
    obs = np.ones(T, np.uint8)
    obs[miss] = 0
    blocks = spec(series, desc)
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    mu, prec, pi = slab_of(p)

    def make_oracle(o, chain):
        return slo.SsLogitOracle(o, successes, trials, X, obs, blocks, mu, prec, pi, seed, chain, g0, clt_threshold=CLT)
    return dict(T=T, p=p, chains=chains, seed=seed, rounds=rounds, X=X, successes=successes, trials=trials, obs=obs,
                blocks=blocks, g0=g0, slots=slots, check=[0, chains - 1], oracle=make_oracle)


@gpu
@pytest.mark.parametrize("k", range(len(ROUND_CASES)))
def test_rounds_match_restatement(oracle, k):
    c = round_case(k)

    def engine():
        e = logit_engine(c["chains"], c["seed"], c["successes"], c["trials"], c["X"], c["obs"], c["blocks"], c["g0"],
                         clt=CLT)
        e.set_slot_limit(c["slots"])
        return e
    eng = engine()
    oracle.set_slot_limit(c["slots"])
    try:
        ora = {ch: c["oracle"](oracle, ch) for ch in c["check"]}
        for r in range(c["rounds"]):
            eng.ss_logit_sweep(1)   # (round 0: the start from v = 0, q = 4 / n; it imputes with s = 1)
            gam, beta, sig = eng.get_states()
            for ch, o in ora.items():
                g, b = o.draw()
                tag = (k, ch, r)
                assert o.last_s == r + 1
                assert np.array_equal(gam[ch], g), tag
                assert relerr(beta[ch], b) < RTOL, tag
                assert sig[ch] == 1.0
                v, q = eng.ss_logit_get_latent(ch)
                assert relerr(q, o.q, 1e-300) < RTOL and relerr(v, o.v) < RTOL, tag
                st = eng.ss_get_state_draw(ch)
                assert np.max(np.abs(st - o.state)) < 1e-8 * np.abs(o.state).max(), tag
                for j, blk in enumerate(c["blocks"]):
                    sm = eng.ss_get_state_model(ch, j)
                    nv = len(sm["variances"])
                    assert relerr(sm["variances"], o.var[j], 1e-300) < RTOL, tag + (j,)
                    assert np.array_equal(sm["suf_n"], o.suf_n[j][:nv]), tag + (j,)
                    assert relerr(sm["suf_ss"], o.suf_ss[j][:nv], 1e-300) < RTOL, tag + (j,)
    finally:
        oracle.set_slot_limit(0)
    for ch, o in ora.items():
        print("case %d chain %d: smallest branch margin of the imputer %.3e, BTPE draws %d" % (k, ch, o.margin, o.btpe))
        assert o.margin > 1e-9 and o.btpe == 0, (ch, o.margin, o.btpe)
    # several rounds in one call: the same draws
    eng2 = engine()
    eng2.ss_logit_sweep(c["rounds"])
    for u, w in zip(eng.get_states(), eng2.get_states()):
        assert np.array_equal(u, w)
    for u, w in zip(eng.ss_logit_get_latent(1), eng2.ss_logit_get_latent(1)):
        assert np.array_equal(u, w)
    assert np.array_equal(eng.ss_get_state_draw(1), eng2.ss_get_state_draw(1))


# ---- 4. distribution -----------------------------------------------------------------------------
@gpu
def test_state_draws_have_the_dense_posterior_moments():
    blocks, S, var, v, obs, q, _ = spo.fixed_case()
    H = slo.observation_variances(q, obs)   # (pi^2 / 3 at the missing step)
    T, chains = len(v), 4096
    X = np.ones((T, 1))
    g0 = np.zeros(1, np.uint8)
    eng = logit_engine(chains, 20264, np.zeros(T), np.ones(T), X, obs.astype(np.uint8), blocks, g0)
    eng.ss_logit_set_latent(v, q)
    eng.ss_logit_impute_state()
    draws = np.stack([eng.ss_get_state_draw(c).reshape(-1) for c in range(chains)])
    mean, cov = slo.dense_posterior(S, var, v, obs, H)
    d = len(mean)
    bound = slo.bonferroni_bound(d + d * (d + 1) // 2)   # (fixed with the seed before any run)
    zm, zc = slo.moment_z(draws, mean, cov)
    print("largest |z|: mean %.3f covariance %.3f, bound %.3f" % (np.abs(zm).max(), np.abs(zc).max(), bound))
    assert np.abs(zm).max() < bound
    assert np.abs(zc).max() < bound


# ---- 5. interface --------------------------------------------------------------------------------
def small_problem():
    T, p = 30, 3
    X, successes, trials, series = binomial_series(T, p, 2, max_trials=3)
    return T, p, X, successes, trials, spec(series, [("level",)])


@gpu
def test_refusals_and_their_texts():
    import boom_amd
    T, p, X, successes, trials, blocks = small_problem()
    mu, prec, pi = slab_of(p)
    g0 = np.zeros(p, np.uint8)
    eng = boom_amd.Engine(2, seed=1)
    first = "call ba_ss_logit_set_data first"
    # the family's calls on an engine without its data
    refused(lambda: eng.ss_logit_sweep(1), first)
    refused(lambda: eng.ss_logit_get_latent(0), first)
    eng.ss_set_data(np.zeros(T), X, None)
    refused(lambda: eng.ss_logit_sweep(1), first)
    refused(lambda: eng.ss_logit_impute_state(), first)
    refused(lambda: eng.ss_logit_set_latent(np.zeros(T), np.ones(T)), first)
    # the data: successes and trials are checked at the observed steps only
    obs = np.ones(T, np.uint8)
    obs[3] = 0
    for bad in (0.0, 1.5, -1.0, np.nan):
        n = trials.copy()
        n[4] = bad
        refused(lambda: eng.ss_logit_set_data(np.zeros(T), n, X, obs), "trials must be integers of at least 1")
    for bad in (-1.0, 0.5, np.nan):
        y = successes.copy()
        y[4] = bad
        refused(lambda: eng.ss_logit_set_data(y, trials, X, obs), "successes must be non-negative integers")
    y = successes.copy()
    y[4] = trials[4] + 1
    refused(lambda: eng.ss_logit_set_data(y, trials, X, obs), "must not exceed the number of trials")
    for bad in (0, 65):
        refused(lambda: eng.ss_logit_set_data(successes, trials, X, obs, clt_threshold=bad),
                "clt_threshold must be between 1 and 64")
    y, n = successes.copy(), trials.copy()
    y[3], n[3] = np.nan, np.nan
    eng.ss_logit_set_data(y, n, X, obs)                    # (a missing step's are never read)
    # no state list
    eng.sss_set_slab(mu, prec, scales_with_sigsq=False)
    eng.set_spike(pi)
    refused(lambda: eng.ss_logit_sweep(1), "call ba_ss_add_state_model first")
    eng.ss_set_local_level(0.01, 0.1, 1.0, 0.0, 1.0, 1.0)
    refused(lambda: eng.ss_logit_sweep(1), "the logit state-space family takes a list of state models")
    refused(lambda: eng.ss_logit_sweep(1), "not ba_ss_set_local_level")
    eng.ss_set_state_models(blocks)
    eng.set_state(g0)
    # sweeps of other kinds
    use = "logit state-space data are set: use ba_ss_logit_sweep"
    for call in (lambda: eng.ss_sweep(1), lambda: eng.ss_impute_state(), lambda: eng.ss_draw_next(),
                 lambda: eng.logit_sweep(1), lambda: eng.poisson_sweep(1), lambda: eng.ss_student_sweep(1),
                 lambda: eng.ss_student_impute_state(), lambda: eng.ss_poisson_sweep(1),
                 lambda: eng.ss_poisson_impute_state(), lambda: eng.student_sweep(1), lambda: eng.sweep(1),
                 lambda: eng.sss_sweep(1), lambda: eng.quantile_sweep(1)):
        refused(call, use)
    refused(lambda: eng.ss_student_get_weights(0), "call ba_ss_student_set_data first")
    refused(lambda: eng.ss_poisson_get_latent(0), "call ba_ss_poisson_set_data first")
    refused(lambda: eng.ss_poisson_set_latent(np.zeros(T), np.ones(T)), "call ba_ss_poisson_set_data first")
    refused(lambda: eng.logit_set_imputer(1), "logit state-space data are set: the imputer is the auxiliary mixture's")
    refused(lambda: eng.ss_forecast(np.zeros((2, p))), "forecasts with binomial observation noise are not implemented")
    # latent data
    for bad, text in ((-1.0, "precision must be non-negative."), (0.0, "must be positive and finite"),
                      (np.inf, "must be positive and finite"), (np.nan, "must be positive and finite")):
        q = np.ones(T)
        q[4] = bad
        refused(lambda: eng.ss_logit_set_latent(np.zeros(T), q), text)
    v = np.zeros(T)
    v[4] = np.nan
    refused(lambda: eng.ss_logit_set_latent(v, np.ones(T)), "the latent value of an observed step must be finite")
    refused(lambda: eng.ss_logit_set_latent(np.zeros(T), np.ones(T), chain=2), "chain index out of range")
    q = np.ones(T)
    q[3] = -1.0                                            # (a missing step's entries are not read)
    eng.ss_logit_set_latent(np.zeros(T), q)
    # a slab that scales with sigma^2
    eng.sss_set_slab(mu, prec, scales_with_sigsq=True)
    refused(lambda: eng.ss_logit_sweep(1), "the logit state-space sampler takes a fixed-precision slab (scales_with_sigsq = 0)")
    eng.sss_set_slab(mu, prec, scales_with_sigsq=False)
    eng.ss_logit_sweep(2)
    assert eng.ss_get_state_draw(0).shape == (T, 1)
    v, q = eng.ss_logit_get_latent(0)
    assert v[3] == 0.0 and q[3] == 0.0 and np.all(q[obs.astype(bool)] > 0)


@gpu
def test_recorded_draws_and_get_state():
    T, p, X, successes, trials, blocks = small_problem()
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    chains, seed, n = 3, 19, 6
    a = logit_engine(chains, seed, successes, trials, X, None, blocks, g0)
    a.enable_draws(n)
    a.ss_logit_sweep(n)
    g, b, s = a.get_draws(0, n)
    b1 = logit_engine(chains, seed, successes, trials, X, None, blocks, g0)
    for r in range(n):
        b1.ss_logit_sweep(1)
        gg, bb, ss = b1.get_state(0)
        assert np.array_equal(g[r], gg) and np.array_equal(b[r], bb) and s[r] == ss == 1.0, r
    gg, bb, ss = a.get_state(0)
    assert np.array_equal(g[-1], gg) and np.array_equal(b[-1], bb) and s[-1] == ss


@gpu
def test_pybind_classes_agree_with_the_c_abi():
    """boom.StateSpaceLogitModel + StateSpaceLogitPosteriorSampler (the facade of
    include/boom_amd.hpp behind them): three rounds == the engine through the C-ABI on the same
    seed, bit for bit"""
    import boom_amd._boom as boom
    T, p, chains, seed = 40, 4, 3, 23
    X, successes, trials, series = binomial_series(T, p, 6, max_trials=8, seasons=4)   # (both branches)
    obs = np.ones(T, np.uint8)
    obs[[9, 30]] = 0
    desc = [("level",), ("seasonal", 4, 1)]
    blocks = general_spec(series, desc)
    mu, prec, pi = slab_of(p)
    model = boom.StateSpaceLogitModel(successes, trials, X, [bool(o) for o in obs], chains=chains, seed=seed)
    b = blocks[0]
    level = boom.LocalLevelStateModel(float(b["initial_sigma"][0]))
    level.set_initial_state_mean(float(b["a0"][0]))
    level.set_initial_state_variance(float(b["P0"][0]))
    level.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    b = blocks[1]
    seas = boom.SeasonalStateModel(4)
    seas.set_sigsq(b["initial_sigma"][0] ** 2)
    seas.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    seas.set_initial_state_mean(b["a0"])
    seas.set_initial_state_variance(b["P0"][0])
    model.add_state(level)
    model.add_state(seas)
    with pytest.raises(Exception, match="Slab does not match model dimension."):
        boom.StateSpaceLogitPosteriorSampler(model, boom.MvnModel(np.zeros(p + 1), np.eye(p + 1), True),
                                             boom.VariableSelectionPrior(pi))
    with pytest.raises(Exception, match="Spike does not match model dimension."):
        boom.StateSpaceLogitPosteriorSampler(model, boom.MvnModel(mu, prec, True),
                                             boom.VariableSelectionPrior(np.full(p + 1, 0.5)))
    sampler = boom.StateSpaceLogitPosteriorSampler(model, boom.MvnModel(mu, prec, True), boom.VariableSelectionPrior(pi))
    model.set_method(sampler)
    assert model.state_dimension == 4
    eng = logit_engine(chains, seed, successes, trials, X, obs, blocks, np.zeros(p, np.uint8))
    for _ in range(3):
        model.sample_posterior()
        eng.ss_logit_sweep(1)
    for u, w in zip(model.chain_states(), eng.get_states()):
        assert np.array_equal(u, w)
    for c in range(chains):
        v, q = eng.ss_logit_get_latent(c)
        assert np.array_equal(model.latent_values(c), v) and np.array_equal(model.latent_precisions(c), q)
        assert np.array_equal(model.state(c), eng.ss_get_state_draw(c).T)
    # set_latent_data and impute_state through the classes
    model.set_latent_data(series, np.full(T, 2.0))
    model.impute_state()
    eng.ss_logit_set_latent(series, np.full(T, 2.0))
    eng.ss_logit_impute_state()
    assert np.array_equal(model.state(1), eng.ss_get_state_draw(1).T)


# ---- 6. signal recovery --------------------------------------------------------------------------
RECOVERY_SHAPE, RECOVERY_TRIALS, RECOVERY_SEED, RECOVERY_COEF = (200, 6), 20, 11, (0.5, -0.5)


def recovery_data(with_path=False):
    T, p = RECOVERY_SHAPE
    return binomial_series(T, p, RECOVERY_SEED, coef=RECOVERY_COEF, fixed_trials=RECOVERY_TRIALS, with_path=with_path)


@gpu
def test_ss_logit_recovers_the_signals():
    """a series whose success probability depends on 2 of 6 predictors, 20 trials a step (Bernoulli
    data at T = 200 carry too little information for the z-scores below): after 150 + 100 rounds of
    64 chains the summaries include those two and not the rest.

    What the summaries should show is a property of the data drawn, not only of the sampler (the
    docstring of test_ss_poisson_recovers_the_signals has the argument): with prior odds 1/5, a slab
    of unit variance and a coefficient standard error below 0.05, a predictor whose z-score is z has
    posterior inclusion odds of about 0.2 * 0.05 * exp(z^2 / 2) when the state is known -- under
    0.02 at |z| = 1, and beyond 1e19 at |z| = 10.  The data seed is one whose four null predictors
    all have |z| < 1 in a plain binomial logistic regression with the generating state as offset,
    and whose two signals sit at |z| > 10, which tests/test_ss_logit_cpu.py checks without this
    sampler.  The thresholds are those of the Poisson family's test on data of the same kind."""
    T, p = RECOVERY_SHAPE
    X, successes, trials, series = recovery_data()
    blocks = spec(series, [("level",)])
    eng = logit_engine(64, 5, successes, trials, X, None, blocks, np.zeros(p, np.uint8), pi=np.full(p, 1.0 / p))
    eng.ss_logit_sweep(150)
    eng.reset_summaries()
    eng.ss_logit_sweep(100)
    sm = eng.get_summaries()
    inc = sm["inclusion_count"] / sm["sweeps"]
    print("inclusion frequencies", inc)
    assert inc[:2].min() > 0.95 and inc[2:].max() < 0.3
