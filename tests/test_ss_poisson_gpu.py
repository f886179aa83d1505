"""bsts family = "poisson" on the device (ba_ss_poisson_*): StateSpacePoissonModel with
StateSpacePoissonPosteriorSampler -- the general structural kernel on every chain's own latent
series v_t with the per-step observation variance H_t = 1 / q_t, the Poisson imputation at
eta_t = Z_t'alpha_t + x_t'beta over the observed steps, the round's order.  The bodies the family
shares with the logit one are tests/ss_family_checks.py's.

  identity      the state draw on latent data set the same in every chain against the Gaussian
                engine's on y = v, bit for bit
  filter edges  one impute_state against the restatement (tests/ss_poisson_oracle.py): values and
                precisions of every chain's own, precisions over six decades, missing steps
  whole rounds  against the restatement on the same substreams: inclusion indicators bit-exact;
                beta, v, q, the state models' variances and statistics within 1e-8 relative, the
                state within 1e-8 of its largest magnitude (the bars of tests/test_poisson_gpu.py
                and tests/test_ss_student_gpu.py)
  distribution  4096 chains' state draws against the dense Gaussian posterior
  interface     refusals and their texts, recorded draws, ba_get_state, the pybind classes
  recovery      the summaries find the two predictors the rate depends on
"""
import numpy as np
import pytest

import ss_family_checks as checks
from ss_family_cases import ROUND_CASES, count_series, golden_mix, poisson_engine, recovery_data, slab_of, spec
from ss_family_checks import POISSON
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
    checks.shared_latent_data_equal_the_scalar_kernel(POISSON, desc, T, missing)


# ---- 2. filter edges -----------------------------------------------------------------------------
@gpu
def test_impute_state_matches_restatement_on_every_chains_own_series(oracle):
    checks.impute_state_matches_restatement_on_every_chains_own_series(POISSON, oracle)


# ---- 3. whole rounds -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", range(len(ROUND_CASES["poisson"])))
def test_rounds_match_restatement(oracle, k):
    def end(k, ch, o):
        print("case %d chain %d: smallest branch margin of the imputer %.3e" % (k, ch, o.margin))
        assert o.margin > 1e-9, (ch, o.margin)
    checks.rounds_match_restatement(POISSON, oracle, k, end)


# ---- 4. distribution -----------------------------------------------------------------------------
@gpu
def test_state_draws_have_the_dense_posterior_moments():
    checks.state_draws_have_the_dense_posterior_moments(POISSON, 20263)


# ---- 5. interface --------------------------------------------------------------------------------
@gpu
def test_refusals_and_their_texts():
    import boom_amd
    T, p, X, (counts, exposure), series, blocks = POISSON.small()
    mu, prec, pi = slab_of(p)
    mix = golden_mix()
    g0 = np.zeros(p, np.uint8)
    eng = boom_amd.Engine(2, seed=1)
    checks.refusals_before_the_data(POISSON, eng, T, X, np.log(counts + 0.5))
    # the data: counts and exposures are checked at the observed steps only
    obs = np.ones(T, np.uint8)
    obs[3] = 0
    for bad, text in ((-1.0, "counts must be non-negative integers"), (1.5, "counts must be non-negative integers")):
        y = counts.copy()
        y[4] = bad
        refused(lambda: eng.ss_poisson_set_data(y, exposure, X, mix, obs), text)
    ex = exposure.copy()
    ex[4] = 0.0
    refused(lambda: eng.ss_poisson_set_data(counts, ex, X, mix, obs), "exposures must be positive")
    y, ex = counts.copy(), exposure.copy()
    y[3], ex[3] = np.nan, np.nan
    eng.ss_poisson_set_data(y, ex, X, mix, obs)            # (a missing step's are never read)
    # no state list
    eng.sss_set_slab(mu, prec, scales_with_sigsq=False)
    eng.set_spike(pi)
    checks.refusals_without_a_state_list(POISSON, eng)
    eng.ss_set_state_models(blocks)
    eng.set_state(g0)
    # sweeps of other kinds
    use = "Poisson state-space data are set: use ba_ss_poisson_sweep"
    for call in (lambda: eng.ss_sweep(1), lambda: eng.ss_impute_state(), lambda: eng.ss_draw_next(),
                 lambda: eng.poisson_sweep(1), lambda: eng.ss_student_sweep(1), lambda: eng.ss_student_impute_state(),
                 lambda: eng.student_sweep(1), lambda: eng.sweep(1), lambda: eng.sss_sweep(1),
                 lambda: eng.quantile_sweep(1)):
        refused(call, use)
    refused(lambda: eng.ss_forecast(np.zeros((2, p))), "forecasts with Poisson observation noise are not implemented")
    # latent data
    checks.refusals_of_latent_data(POISSON, eng, T)
    q = np.ones(T)
    q[3] = -1.0                                            # (a missing step's entries are not read)
    eng.ss_poisson_set_latent(np.zeros(T), q)
    # a slab that scales with sigma^2
    checks.refusal_of_the_other_slab(POISSON, eng, T, mu, prec, "fixed-precision slab (scales_with_sigsq = 0)")
    v, q = eng.ss_poisson_get_latent(0)
    assert v[3] == 0.0 and q[3] == 0.0 and np.all(q[obs.astype(bool)] > 0)


@gpu
def test_a_sweep_without_mixtures_is_refused():
    import boom_amd
    from boom_amd.capi import _fcol, _f64, _p
    T, p, X, (counts, exposure), _, blocks = POISSON.small()
    eng = boom_amd.Engine(2, seed=1)
    eng._check(eng.lib.ba_ss_poisson_set_data(eng._h, T, p, _p(_f64(counts)), _p(_f64(exposure)), _p(_fcol(X)), None))
    eng.p, eng.T = p, T
    mu, prec, pi = slab_of(p)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=False)
    eng.set_spike(pi)
    eng.ss_set_state_models(blocks)
    refused(lambda: eng.ss_poisson_sweep(1), "call ba_poisson_set_mixtures first")
    bad = dict(golden_mix())
    keep = bad["counts"] != int(counts[counts > 0][0])
    off = np.concatenate([[0], np.cumsum(bad["ncomp"])])
    sel = np.concatenate([np.arange(off[i], off[i + 1]) for i in range(len(keep)) if keep[i]])
    bad.update(counts=bad["counts"][keep], ncomp=bad["ncomp"][keep], mu=bad["mu"][sel], sigma=bad["sigma"][sel],
               weight=bad["weight"][sel])
    refused(lambda: eng._poisson_set_mixtures(bad), "no mixture")


@gpu
def test_recorded_draws_and_get_state():
    checks.recorded_draws_and_get_state(POISSON)


@gpu
def test_pybind_classes_agree_with_the_c_abi():
    X, counts, exposure, series = count_series(40, 4, 6, seasons=4)
    mix = golden_mix()

    def model_of(boom, is_observed, chains, seed):
        model = boom.StateSpacePoissonModel(counts, exposure, X, is_observed, chains=chains, seed=seed)
        model.set_mixture_table([int(c) for c in mix["counts"]], [int(c) for c in mix["ncomp"]], mix["mu"], mix["sigma"],
                                mix["weight"], mix["largest_index"])
        return model
    checks.latent_pybind_classes_agree_with_the_c_abi(POISSON, X, (counts, exposure), series, model_of)


# ---- 6. signal recovery --------------------------------------------------------------------------
@gpu
def test_ss_poisson_recovers_the_signals():
    """a series whose rate depends on 2 of 6 predictors: after 150 + 100 rounds of 64 chains the
    summaries include those two and not the rest (the thresholds of
    test_poisson_recovers_the_signals_and_rejects_bad_arguments).

    What the summaries should show is a property of the data drawn, not only of the sampler: with
    prior odds 1/5, a slab of unit variance and a coefficient standard error near 0.035, a
    predictor whose z-score is z has posterior inclusion odds of about 0.2 * 0.035 * exp(z^2 / 2)
    when the state is known -- 0.01 at |z| = 1, 0.1 at |z| = 2.3 -- and more than that, slowly
    mixing from chain to chain, once the level has to be learned too (a data set with a null
    predictor at z = 2.3 has it in 30 % of the draws, in the restatement as on the device).  The
    data seed is therefore one whose four null predictors all have |z| < 1 in a plain Poisson
    regression with the generating state as offset, which tests/test_ss_poisson_cpu.py checks
    without this sampler; the two signals sit at |z| > 10."""
    X, counts, exposure, series = recovery_data("poisson")
    p = X.shape[1]
    blocks = spec(series, [("level",)])
    eng = poisson_engine(64, 5, counts, exposure, X, None, blocks, np.zeros(p, np.uint8), pi=np.full(p, 1.0 / p))
    eng.ss_poisson_sweep(150)
    eng.reset_summaries()
    eng.ss_poisson_sweep(100)
    sm = eng.get_summaries()
    inc = sm["inclusion_count"] / sm["sweeps"]
    print("inclusion frequencies", inc)
    assert inc[:2].min() > 0.95 and inc[2:].max() < 0.3
