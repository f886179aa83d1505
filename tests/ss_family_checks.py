"""The bodies of the tests that the Student-t, Poisson and logit state space families have in common, written
once over a description of the family (Family).  tests/test_ss_{student,poisson,logit}_{gpu,cpu}.py call them
under their own test names; what a family asserts on its own stays there.  (Not a test module.)"""
import numpy as np
import pytest

import ss_family_oracle as sfo
import ss_poisson_oracle as spo
import ss_logit_oracle as slo
import ss_student_oracle as sso
from cases import general_data, general_spec
from ss_family_cases import (binomial_series, chain_parameters, count_series, gaussian_engine, golden_mix,
                             logit_engine, poisson_engine, relerr, round_case, slab_of, spec, state_stream,
                             student_engine, student_slab_of)
from ss_gpu_helpers import refused

RTOL = 1e-8


class Family:
    """name: the family's word in the entry points (ba_ss_<name>_*); engine(chains, seed, *data, X, obs, blocks,
    g0, ...): its engine; latent: the word of its latent data's setter and getter; slab_of(p): its slab and spike;
    fixed_sigsq: sigma^2 stays 1 (the slab must then not scale with it); neutral(T): data that make its imputer
    irrelevant; missing_variance: H_t of a missing step; small(): the data of the interface tests -- (T, p, X,
    data, the series that sizes the priors, blocks)"""

    def __init__(self, name, engine, latent, slab_of, fixed_sigsq, neutral=None, missing_variance=None, small=None,
                 oracle=None):
        self.name, self.engine, self.latent, self.slab_of, self.fixed_sigsq = name, engine, latent, slab_of, fixed_sigsq
        self.neutral, self.missing_variance, self.small, self.oracle = neutral, missing_variance, small, oracle
        self.first = "call ba_ss_%s_set_data first" % name

    def call(self, eng, what, *args, **kw):
        return getattr(eng, "ss_%s_%s" % (self.name, what))(*args, **kw)

    def sweep(self, eng, n):
        return self.call(eng, "sweep", n)

    def impute_state(self, eng):
        return self.call(eng, "impute_state")

    def set_latent(self, eng, *latent, **kw):
        return self.call(eng, "set_" + self.latent, *latent, **kw)

    def get_latent(self, eng, chain):
        return self.call(eng, "get_" + self.latent, chain)

    def unit_latent(self, T):
        """latent data of the simplest kind: weights 1; values 0 and precisions 1"""
        return (np.zeros(T), np.ones(T)) if self.fixed_sigsq else (np.ones(T),)


def _student_small():
    T, p = 30, 3
    X, y, _, _ = general_data(T, p, 1, [], seed=2)
    return T, p, X, (y,), y, general_spec(y, [("level",)])


def _poisson_small():
    T, p = 30, 3
    X, counts, exposure, series = count_series(T, p, 2)
    return T, p, X, (counts, exposure), series, spec(series, [("level",)])


def _logit_small():
    T, p = 30, 3
    X, successes, trials, series = binomial_series(T, p, 2, max_trials=3)
    return T, p, X, (successes, trials), series, spec(series, [("level",)])


def _poisson_oracle(o, data, X, obs, blocks, slab, seed, chain, g0):
    return spo.SsPoissonOracle(o, *data, X, obs, blocks, golden_mix(), *slab, seed, chain, g0)


def _logit_oracle(o, data, X, obs, blocks, slab, seed, chain, g0):
    return slo.SsLogitOracle(o, *data, X, obs, blocks, *slab, seed, chain, g0)


STUDENT = Family("student", student_engine, "weights", student_slab_of, False, small=_student_small)
POISSON = Family("poisson", poisson_engine, "latent", slab_of, True, neutral=lambda T: (np.ones(T), np.ones(T)),
                 missing_variance=spo.MISSING_VARIANCE, small=_poisson_small, oracle=_poisson_oracle)
LOGIT = Family("logit", logit_engine, "latent", slab_of, True, neutral=lambda T: (np.zeros(T), np.ones(T)),
               missing_variance=slo.MISSING_VARIANCE, small=_logit_small, oracle=_logit_oracle)


# ---- pieces --------------------------------------------------------------------------------------
def same_state_and_statistics(a, b, chains, blocks, tag=()):
    """two engines' state draws and state-model statistics, bit for bit"""
    for c in range(chains):
        assert np.array_equal(a.ss_get_state_draw(c), b.ss_get_state_draw(c)), tag + (c,)
        for k in range(len(blocks)):
            u, w = a.ss_get_state_model(c, k), b.ss_get_state_model(c, k)
            assert np.array_equal(u["suf_ss"], w["suf_ss"]) and np.array_equal(u["suf_n"], w["suf_n"]), tag + (c, k)


def state_and_models_match(eng, o, blocks, ch, tag):
    """chain ch's state draw within 1e-8 of the restatement's largest magnitude; the state models' variances and
    statistics within RTOL, the counts equal"""
    st = eng.ss_get_state_draw(ch)
    assert np.max(np.abs(st - o.state)) < 1e-8 * np.abs(o.state).max(), tag
    for j in range(len(blocks)):
        sm = eng.ss_get_state_model(ch, j)
        nv = len(sm["variances"])
        assert relerr(sm["variances"], o.var[j], 1e-300) < RTOL, tag + (j,)
        assert np.array_equal(sm["suf_n"], o.suf_n[j][:nv]), tag + (j,)
        assert relerr(sm["suf_ss"], o.suf_ss[j][:nv], 1e-300) < RTOL, tag + (j,)


def draws_have_the_moments(eng, chains, S, var, series, obs, H):
    """the chains' state draws against the dense Gaussian posterior: every z-statistic of the mean and the
    covariance under the Bonferroni bound at level 1e-3"""
    draws = np.stack([eng.ss_get_state_draw(c).reshape(-1) for c in range(chains)])
    mean, cov = sso.dense_posterior(S, var, series, obs, H)
    d = len(mean)
    bound = sso.bonferroni_bound(d + d * (d + 1) // 2)   # (fixed with the seed before any run)
    zm, zc = sso.moment_z(draws, mean, cov)
    print("largest |z|: mean %.3f covariance %.3f, bound %.3f" % (np.abs(zm).max(), np.abs(zc).max(), bound))
    assert np.abs(zm).max() < bound
    assert np.abs(zc).max() < bound


def level_and_seasonal(boom, blocks):
    """the façade's state models of a [level, seasonal of 4] list"""
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
    return level, seas


def three_rounds_agree(fam, model, eng):
    """three rounds through the classes == the engine through the C-ABI on the same seed, bit for bit"""
    assert model.state_dimension == 4
    for _ in range(3):
        model.sample_posterior()
        fam.sweep(eng, 1)
    for u, w in zip(model.chain_states(), eng.get_states()):
        assert np.array_equal(u, w)
    for c in range(eng.chains):
        assert np.array_equal(model.state(c), eng.ss_get_state_draw(c).T)


# ---- the GPU tests -------------------------------------------------------------------------------
def shared_latent_data_equal_the_scalar_kernel(fam, desc, T, missing):
    """q = 1: the Gaussian engine's impute_state on y = v at sigma^2 = 1, bit for bit; then q = 4:
    at sigma^2 = 1/4 (exact in binary) -- the per-chain series read through y_stride is the shared
    one, and the scalar and Student paths are what they were"""
    p, chains, seed = 3, 4, 77
    seas = [(b[1], b[2]) for b in desc if b[0] == "seasonal"]
    X, v, _, obs = general_data(T, p, 2, seas, seed=T, missing_frac=missing)
    blocks = general_spec(v, desc)
    gam, beta = chain_parameters(p, chains, 3)
    for q in (1.0, 4.0):
        a = fam.engine(chains, seed, *fam.neutral(T), X, obs, blocks, gam[0])
        b = gaussian_engine(chains, seed, v, X, obs, blocks, gam[0])
        for c in range(chains):
            a.set_state(gam[c], beta[c], 1.0, chain=c)
            b.set_state(gam[c], beta[c], 1.0 / q, chain=c)
        fam.set_latent(a, v, np.full(T, q))
        fam.impute_state(a)
        b.ss_impute_state()
        same_state_and_statistics(a, b, chains, blocks, (q,))


def impute_state_matches_restatement_on_every_chains_own_series(fam, oracle):
    """values and precisions that differ from chain to chain (the test that fails if the kernel
    reads chain 0's series for every chain), precisions from 1e-3 to 1e3, the first step and a
    step of the second block of 64 missing.  Returns every chain's observation variances."""
    desc, T, p, chains, seed = [("trend",), ("seasonal", 4, 1)], 70, 3, 4, 41
    X, y, _, _ = general_data(T, p, 2, [(4, 1)], seed=12)
    obs = np.ones(T, np.uint8)
    obs[[0, 66]] = 0
    blocks = general_spec(y, desc)
    gam, beta = chain_parameters(p, chains, 8)
    eng = fam.engine(chains, seed, *fam.neutral(T), X, obs, blocks, gam[0])
    rs = np.random.Generator(np.random.PCG64(2))
    V = y[None, :] + rs.standard_normal((chains, T))
    Q = np.exp(rs.uniform(np.log(1e-3), np.log(1e3), (chains, T)))
    Q[:, [1, 65]] = [1e-3, 1e3]
    for c in range(chains):
        eng.set_state(gam[c], beta[c], 1.0, chain=c)
        fam.set_latent(eng, V[c], Q[c], chain=c)
    fam.impute_state(eng)
    S = sso.Structure(blocks)
    var = [np.asarray(b["initial_sigma"], float) ** 2 for b in blocks]
    ob = obs.astype(bool)
    Hs = []
    for c in range(chains):
        H = sfo.observation_variances(Q[c], ob, fam.missing_variance)
        assert H[0] == fam.missing_variance and H[66] == H[0]
        inc = np.flatnonzero(gam[c])
        want = sso.impute_state(S, var, V[c] - X[:, inc] @ beta[c][inc], ob, H, state_stream(oracle, seed, c))
        got = eng.ss_get_state_draw(c)
        assert np.max(np.abs(got - want)) < 1e-8 * np.abs(want).max(), c
        n, ss = sso.state_model_suf(S, want)
        for k in range(len(blocks)):
            sm = eng.ss_get_state_model(c, k)
            nv = len(sm["variances"])
            assert np.array_equal(sm["suf_n"], n[k][:nv]), (c, k)
            assert relerr(sm["suf_ss"], ss[k][:nv], 1e-300) < RTOL, (c, k)
        v, q = fam.get_latent(eng, c)
        assert np.array_equal(v, np.where(ob, V[c], 0.0)) and np.array_equal(q, np.where(ob, Q[c], 0.0)), c
        Hs.append(H)
    return Hs


def rounds_match_restatement(fam, oracle, k, end):
    """whole rounds of case k against the restatement on the same substreams; end(k, ch, o): what the family
    asserts of a checked chain's restatement once the rounds are over (its margins)"""
    c = round_case(fam.name, k)

    def engine():
        e = c["engine"]()
        e.set_slot_limit(c["slots"])
        return e
    eng = engine()
    oracle.set_slot_limit(c["slots"])
    try:
        ora = {ch: c["oracle"](oracle, ch) for ch in c["check"]}
        for r in range(c["rounds"]):
            fam.sweep(eng, 1)   # (round 0: the start from a new model's latent data; it imputes with s = 1)
            gam, beta, sig = eng.get_states()
            for ch, o in ora.items():
                g, b = o.draw()
                tag = (k, ch, r)
                assert o.last_s == r + 1
                assert np.array_equal(gam[ch], g), tag
                assert relerr(beta[ch], b) < RTOL, tag
                assert sig[ch] == 1.0
                v, q = fam.get_latent(eng, ch)
                assert relerr(q, o.q, 1e-300) < RTOL and relerr(v, o.v) < RTOL, tag
                state_and_models_match(eng, o, c["blocks"], ch, tag)
    finally:
        oracle.set_slot_limit(0)
    for ch, o in ora.items():
        end(k, ch, o)
    # several rounds in one call: the same draws
    eng2 = engine()
    fam.sweep(eng2, c["rounds"])
    for u, w in zip(eng.get_states(), eng2.get_states()):
        assert np.array_equal(u, w)
    for u, w in zip(fam.get_latent(eng, 1), fam.get_latent(eng2, 1)):
        assert np.array_equal(u, w)
    assert np.array_equal(eng.ss_get_state_draw(1), eng2.ss_get_state_draw(1))


def state_draws_have_the_dense_posterior_moments(fam, seed):
    blocks, S, var, v, obs, q = sfo.fixed_case()
    H = sfo.observation_variances(q, obs, fam.missing_variance)
    T, chains = len(v), 4096
    X = np.ones((T, 1))
    g0 = np.zeros(1, np.uint8)
    eng = fam.engine(chains, seed, *fam.neutral(T), X, obs.astype(np.uint8), blocks, g0)
    fam.set_latent(eng, v, q)
    fam.impute_state(eng)
    draws_have_the_moments(eng, chains, S, var, v, obs, H)


def recorded_draws_and_get_state(fam, recorded=None):
    """recorded: (the recorded draws of chain 0 of a family's own parameter, its value in chain 0 now)"""
    T, p, X, data, _, blocks = fam.small()
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    chains, seed, n = 3, 19, 6
    a = fam.engine(chains, seed, *data, X, None, blocks, g0)
    a.enable_draws(n)
    fam.sweep(a, n)
    g, b, s = a.get_draws(0, n)
    own = recorded[0](a, n) if recorded else None
    b1 = fam.engine(chains, seed, *data, X, None, blocks, g0)
    for r in range(n):
        fam.sweep(b1, 1)
        gg, bb, ss = b1.get_state(0)
        assert np.array_equal(g[r], gg) and np.array_equal(b[r], bb) and s[r] == ss, r
        if fam.fixed_sigsq:
            assert ss == 1.0, r
        if recorded:
            assert own[r] == recorded[1](b1), r
    gg, bb, ss = a.get_state(0)
    assert np.array_equal(g[-1], gg) and np.array_equal(b[-1], bb) and s[-1] == ss


# ... the refusals, in the order of a model's life; the family's own stand between these in its file
def refusals_before_the_data(fam, eng, T, X, series):
    """the family's calls on an engine without its data"""
    refused(lambda: fam.sweep(eng, 1), fam.first)
    refused(lambda: fam.get_latent(eng, 0), fam.first)
    eng.ss_set_data(series, X, None)
    refused(lambda: fam.sweep(eng, 1), fam.first)
    refused(lambda: fam.impute_state(eng), fam.first)
    refused(lambda: fam.set_latent(eng, *fam.unit_latent(T)), fam.first)


def refusals_without_a_state_list(fam, eng, level_mean=0.0):
    refused(lambda: fam.sweep(eng, 1), "call ba_ss_add_state_model first")
    eng.ss_set_local_level(0.01, 0.1, 1.0, level_mean, 1.0, 1.0)
    refused(lambda: fam.sweep(eng, 1), "not ba_ss_set_local_level")


def refusals_of_latent_data(fam, eng, T):
    for bad, text in ((-1.0, "precision must be non-negative."), (0.0, "must be positive and finite"),
                      (np.inf, "must be positive and finite"), (np.nan, "must be positive and finite")):
        q = np.ones(T)
        q[4] = bad
        refused(lambda: fam.set_latent(eng, np.zeros(T), q), text)


def refusal_of_the_other_slab(fam, eng, T, mu, prec, text):
    """a slab that scales with sigma^2 where the family's must not (or the reverse); then two sweeps"""
    eng.sss_set_slab(mu, prec, scales_with_sigsq=fam.fixed_sigsq)
    refused(lambda: fam.sweep(eng, 1), text)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=not fam.fixed_sigsq)
    fam.sweep(eng, 2)
    assert eng.ss_get_state_draw(0).shape == (T, 1)


def latent_pybind_classes_agree_with_the_c_abi(fam, X, data, series, model_of):
    """boom.StateSpace<Family>Model + StateSpace<Family>PosteriorSampler (the façade of include/boom_amd.hpp
    behind them): three rounds == the engine through the C-ABI on the same seed, bit for bit.
    model_of(boom, is_observed, chains, seed): the family's model on the data"""
    import boom_amd._boom as boom
    T, p = X.shape
    chains, seed = 3, 23
    obs = np.ones(T, np.uint8)
    obs[[9, 30]] = 0
    blocks = general_spec(series, [("level",), ("seasonal", 4, 1)])
    mu, prec, pi = fam.slab_of(p)
    model = model_of(boom, [bool(o) for o in obs], chains, seed)
    for sm in level_and_seasonal(boom, blocks):
        model.add_state(sm)
    Sampler = getattr(boom, "StateSpace%sPosteriorSampler" % fam.name.capitalize())
    with pytest.raises(Exception, match="Slab does not match model dimension."):
        Sampler(model, boom.MvnModel(np.zeros(p + 1), np.eye(p + 1), True), boom.VariableSelectionPrior(pi))
    with pytest.raises(Exception, match="Spike does not match model dimension."):
        Sampler(model, boom.MvnModel(mu, prec, True), boom.VariableSelectionPrior(np.full(p + 1, 0.5)))
    model.set_method(Sampler(model, boom.MvnModel(mu, prec, True), boom.VariableSelectionPrior(pi)))
    eng = fam.engine(chains, seed, *data, X, obs, blocks, np.zeros(p, np.uint8))
    three_rounds_agree(fam, model, eng)
    for c in range(chains):
        v, q = fam.get_latent(eng, c)
        assert np.array_equal(model.latent_values(c), v) and np.array_equal(model.latent_precisions(c), q)
    # set_latent_data and impute_state through the classes
    model.set_latent_data(series, np.full(T, 2.0))
    model.impute_state()
    fam.set_latent(eng, series, np.full(T, 2.0))
    fam.impute_state(eng)
    assert np.array_equal(model.state(1), eng.ss_get_state_draw(1).T)


# ---- the CPU tests of the two latent-data families' restatements ---------------------------------
def small_case(series, nan_at_missing=False):
    """series: count_series or binomial_series at T = 30, p = 3.  Trend + seasonal, two missing steps (NaN
    data there on request): (X, data, obs, blocks, slab, g0)"""
    X, a, b, series = series
    T, p = X.shape
    obs = np.ones(T, np.uint8)
    obs[[4, 17]] = 0
    blocks = spec(series, [("trend",), ("seasonal", 4, 1)])
    if nan_at_missing:
        a, b = a.copy(), b.copy()
        a[[4, 17]] = np.nan
        b[[4, 17]] = np.nan
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    return X, (a, b), obs, blocks, slab_of(p), g0


def first_draw(fam, oracle, case, q0):
    """case: the family's small_case(); q0(data): the precisions of a new model at every step"""
    X, data, obs, blocks, slab, g0 = case
    make = lambda: fam.oracle(oracle, data, X, obs, blocks, slab, 7, 1, g0)   # noqa: E731
    o = make()
    o.impute_state()
    ob = obs.astype(bool)
    Xo, q = X[ob], q0(data)[ob]
    xqx = Xo.T @ (Xo * q[:, None])
    assert np.allclose(o.xtx, xqx, rtol=1e-14, atol=0)
    assert np.allclose(o.xty, -(Xo.T @ (o.offset()[ob] * q)), rtol=1e-12, atol=1e-13)
    # ... and draw() from the start: the first imputation uses up s = 0 and stores nothing
    o = make()
    seen = []
    keep = o.draw_observation_model

    def spy():
        seen.append((o.imputations, o.xtx.copy(), o.v.copy(), o.q.copy()))
        keep()
    o.draw_observation_model = spy
    for r in range(3):
        o.draw()
        assert o.last_s == r + 1 and o.imputations == r + 2
    imputations, xtx, v, q = seen[0]
    assert imputations == 1 and np.all(v == 0) and np.array_equal(q, np.where(ob, q0(data), 0.0))
    assert np.allclose(xtx, xqx, rtol=1e-14, atol=0)
    assert np.all(o.q[ob] > 0) and np.all(o.q[~ob] == 0) and np.all(np.isfinite(o.state))


def missing_steps_read_no_data(fam, oracle, small_case):
    runs = []
    for nan in (False, True):
        X, data, obs, blocks, slab, g0 = small_case(nan)
        o = fam.oracle(oracle, data, X, obs, blocks, slab, 7, 0, g0)
        for _ in range(3):
            o.draw()
        runs.append((o.gamma.copy(), o.beta.copy(), o.v.copy(), o.q.copy(), o.state.copy()))
    for a, b in zip(*runs):
        assert np.all(np.isfinite(b)) and np.array_equal(a, b)


def parity_seeds_keep_their_margins(fam, oracle, end, before=lambda c: None):
    """the whole-round cases of the device test through the restatement alone; end(k, chain, o): the family's
    assertions on a checked chain after the rounds compared; before(c): on the case"""
    from ss_family_cases import ROUND_CASES
    for k in range(len(ROUND_CASES[fam.name])):
        c = round_case(fam.name, k)
        before(c)
        oracle.set_slot_limit(c["slots"])
        try:
            for chain in c["check"]:
                o = c["oracle"](oracle, chain)
                for _ in range(c["rounds"]):
                    o.draw()
                end(k, chain, o)
        finally:
            oracle.set_slot_limit(0)
