"""bsts family = "logit" on the device (ba_ss_logit_*): StateSpaceLogitModel with
StateSpaceLogitPosteriorSampler -- the general structural kernel on every chain's own latent
series v_t with the per-step observation variance H_t = 1 / q_t, the binomial auxiliary-mixture
imputation at eta_t = Z_t'alpha_t + x_t'beta over the observed steps, the round's order.  The bodies
the family shares with the Poisson one are tests/ss_family_checks.py's.

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

import ss_family_checks as checks
from cases import bsts_priors, general_data, general_spec
from ss_family_cases import ROUND_CASES, binomial_series, chain_parameters, logit_engine, recovery_data, slab_of, spec
from ss_family_checks import LOGIT
from ss_gpu_helpers import refused

gpu = pytest.mark.gpu


# ---- 1. identity ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("desc,T,missing", [
    ([("trend",), ("seasonal", 4, 1)], 70, 0.05),     # a 64-step block boundary, a partial last block
    ([("trend",), ("seasonal", 4, 1)], 70, 0.0),
    ([("level",), ("seasonal", 20, 1)], 70, 0.05),    # m = 20 > 16: blocks of 32 steps
    ([("level",), ("seasonal", 20, 1)], 70, 0.0),
])
def test_shared_latent_data_equal_the_scalar_kernel(desc, T, missing):
    checks.shared_latent_data_equal_the_scalar_kernel(LOGIT, desc, T, missing)


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
    checks.same_state_and_statistics(a, b, chains, blocks)


# ---- 2. filter edges -----------------------------------------------------------------------------
@gpu
def test_impute_state_matches_restatement_on_every_chains_own_series(oracle):
    for H in checks.impute_state_matches_restatement_on_every_chains_own_series(LOGIT, oracle):
        assert abs(H[0] - np.pi ** 2 / 3) < 1e-15   # (H = pi^2 / 3 at the missing steps)


# ---- 3. whole rounds -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", range(len(ROUND_CASES["logit"])))
def test_rounds_match_restatement(oracle, k):
    def end(k, ch, o):
        print("case %d chain %d: smallest branch margin of the imputer %.3e, BTPE draws %d" % (k, ch, o.margin, o.btpe))
        assert o.margin > 1e-9 and o.btpe == 0, (ch, o.margin, o.btpe)
    checks.rounds_match_restatement(LOGIT, oracle, k, end)


# ---- 4. distribution -----------------------------------------------------------------------------
@gpu
def test_state_draws_have_the_dense_posterior_moments():
    checks.state_draws_have_the_dense_posterior_moments(LOGIT, 20264)   # (pi^2 / 3 at the missing step)


# ---- 5. interface --------------------------------------------------------------------------------
@gpu
def test_refusals_and_their_texts():
    import boom_amd
    T, p, X, (successes, trials), _, blocks = LOGIT.small()
    mu, prec, pi = slab_of(p)
    g0 = np.zeros(p, np.uint8)
    eng = boom_amd.Engine(2, seed=1)
    checks.refusals_before_the_data(LOGIT, eng, T, X, np.zeros(T))
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
    checks.refusals_without_a_state_list(LOGIT, eng)
    refused(lambda: eng.ss_logit_sweep(1), "the logit state-space family takes a list of state models")
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
    checks.refusals_of_latent_data(LOGIT, eng, T)
    v = np.zeros(T)
    v[4] = np.nan
    refused(lambda: eng.ss_logit_set_latent(v, np.ones(T)), "the latent value of an observed step must be finite")
    refused(lambda: eng.ss_logit_set_latent(np.zeros(T), np.ones(T), chain=2), "chain index out of range")
    q = np.ones(T)
    q[3] = -1.0                                            # (a missing step's entries are not read)
    eng.ss_logit_set_latent(np.zeros(T), q)
    # a slab that scales with sigma^2
    checks.refusal_of_the_other_slab(LOGIT, eng, T, mu, prec,
                                     "the logit state-space sampler takes a fixed-precision slab (scales_with_sigsq = 0)")
    v, q = eng.ss_logit_get_latent(0)
    assert v[3] == 0.0 and q[3] == 0.0 and np.all(q[obs.astype(bool)] > 0)


@gpu
def test_recorded_draws_and_get_state():
    checks.recorded_draws_and_get_state(LOGIT)


@gpu
def test_pybind_classes_agree_with_the_c_abi():
    X, successes, trials, series = binomial_series(40, 4, 6, max_trials=8, seasons=4)   # (both branches)

    def model_of(boom, is_observed, chains, seed):
        return boom.StateSpaceLogitModel(successes, trials, X, is_observed, chains=chains, seed=seed)
    checks.latent_pybind_classes_agree_with_the_c_abi(LOGIT, X, (successes, trials), series, model_of)


# ---- 6. signal recovery --------------------------------------------------------------------------
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
    X, successes, trials, series = recovery_data("logit")
    p = X.shape[1]
    blocks = spec(series, [("level",)])
    eng = logit_engine(64, 5, successes, trials, X, None, blocks, np.zeros(p, np.uint8), pi=np.full(p, 1.0 / p))
    eng.ss_logit_sweep(150)
    eng.reset_summaries()
    eng.ss_logit_sweep(100)
    sm = eng.get_summaries()
    inc = sm["inclusion_count"] / sm["sweeps"]
    print("inclusion frequencies", inc)
    assert inc[:2].min() > 0.95 and inc[2:].max() < 0.3
