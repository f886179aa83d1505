"""bsts family = "student" on the device (ba_ss_student_*): StateSpaceStudentRegressionModel with
StateSpaceStudentPosteriorSampler -- the general structural kernel with the per-step observation
variance H_t = sigma^2 / w_t, the Student kernels on the response y - Z alpha over the observed
steps, the round's order.

  identities    the H_t instances of the kernel against the scalar ones, bit for bit
  filter edges  one impute_state against the restatement (tests/ss_student_oracle.py): weights
                over six decades, missing steps, a weight of exactly 0, nu <= 2
  whole rounds  against the restatement on the same substreams: inclusion indicators bit-exact;
                beta, sigma^2, nu, the weights, the state, the state models' variances and
                sufficient statistics within 1e-8 relative (the bars of tests/test_student_gpu.py
                and tests/test_structural_general_gpu.py)
  distribution  4096 chains' state draws against the dense Gaussian posterior
  interface     refusals and their texts, recorded draws, ba_get_state
"""
import numpy as np
import pytest

import ss_family_checks as checks
import ss_student_oracle as sso
from cases import general_data, general_spec, kernel_instance
from ss_family_cases import (ROUND_CASES, chain_parameters, gaussian_engine, relerr, round_case, state_stream,
                             student_engine, student_slab_of as slab_of)
from ss_family_checks import RTOL, STUDENT
from ss_gpu_helpers import refused

gpu = pytest.mark.gpu


# ---- 3. identities ---------------------------------------------------------------------------
TRIG = ("trig", 12.0, [1.0])


@gpu
@pytest.mark.parametrize("desc,T,missing", [
    ([("trend",), ("seasonal", 4, 1)], 70, 0.05),     # a 64-step block boundary, a partial last block
    ([("level",), ("seasonal", 20, 1)], 40, 0.0),     # m = 20 > 16: blocks of 32 steps
    # the H_t instances no list above reaches (T = None: two time blocks and three steps, 2 chains, p = 2):
    # a seasonal that pads the state to the leading dimension, a one-frequency trig block for GLOB
    ([("level",), ("seasonal", 4, 1), TRIG], None, 0.0),     # LDC 17, GLOB
    ([("level",), ("seasonal", 18, 1), TRIG], None, 0.0),    # LDC 33, GLOB
    ([("level",), ("seasonal", 34, 1)], None, 0.0),          # LDC 61
    ([("level",), ("seasonal", 34, 1), TRIG], None, 0.0),    # LDC 61, GLOB
    ([("level",), ("seasonal", 61, 1)], None, 0.0),          # LDC 65
    ([("level",), ("seasonal", 61, 1), TRIG], None, 0.0),    # LDC 65, GLOB
])
@pytest.mark.parametrize("weight", [1.0, 4.0])
def test_constant_weights_equal_the_scalar_kernel(desc, T, missing, weight):
    """w = 1: the Gaussian engine's impute_state at the same sigma^2, bit for bit; w = 4: at
    sigma^2 / 4 (exact in binary)"""
    p, chains, seed, sigsq = 3, 4, 77, 0.5
    if T is None:
        p, chains = 2, 2
        T = 2 * kernel_instance(general_spec(np.arange(8.0), desc))[2] + 3
    seas = [(b[1], b[2]) for b in desc if b[0] == "seasonal"]
    X, y, _, obs = general_data(T, p, 2, seas, seed=T, missing_frac=missing)
    blocks = general_spec(y, desc)
    gam, beta = chain_parameters(p, chains, 3)
    a = student_engine(chains, seed, y, X, obs, blocks, gam[0])
    b = gaussian_engine(chains, seed, y, X, obs, blocks, gam[0])
    for c in range(chains):
        a.set_state(gam[c], beta[c], sigsq, chain=c)
        b.set_state(gam[c], beta[c], sigsq / weight, chain=c)
    a.ss_student_set_weights(np.full(T, weight))
    a.ss_student_impute_state()
    b.ss_impute_state()
    checks.same_state_and_statistics(a, b, chains, blocks)


# ---- 4. filter edges ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nu", [5.0, 2.0, 1.5])
def test_impute_state_matches_restatement_at_the_edges(oracle, nu):
    """weights from 1e-3 to 1e3, the first step missing, a missing step in the second block of
    64, a weight of exactly 0 on an observed step (H_t = the marginal variance), nu <= 2 (the
    1e8 sigma^2 arm)"""
    desc, T, p, chains, seed, sigsq = [("trend",), ("seasonal", 4, 1)], 70, 3, 4, 41, 0.8
    X, y, _, _ = general_data(T, p, 2, [(4, 1)], seed=12)
    obs = np.ones(T, np.uint8)
    obs[[0, 66]] = 0
    blocks = general_spec(y, desc)
    gam, beta = chain_parameters(p, chains, 8)
    eng = student_engine(chains, seed, y, X, obs, blocks, gam[0])
    eng.student_set_nu(nu)
    rs = np.random.Generator(np.random.PCG64(2))
    W = np.exp(rs.uniform(np.log(1e-3), np.log(1e3), (chains, T)))
    W[:, 10] = 0.0
    W[:, [1, 65]] = [1e-3, 1e3]
    for c in range(chains):
        eng.set_state(gam[c], beta[c], sigsq, chain=c)
        eng.ss_student_set_weights(W[c], chain=c)
    eng.ss_student_impute_state()
    S = sso.Structure(blocks)
    var = [np.asarray(b["initial_sigma"], float) ** 2 for b in blocks]
    ob = obs.astype(bool)
    for c in range(chains):
        H = sso.observation_variances(W[c], ob, sigsq, nu)
        assert H[10] == sso.marginal_variance(sigsq, nu) and H[0] == H[10]
        inc = np.flatnonzero(gam[c])
        want = sso.impute_state(S, var, y - X[:, inc] @ beta[c][inc], ob, H, state_stream(oracle, seed, c))
        got = eng.ss_get_state_draw(c)
        assert np.max(np.abs(got - want)) < 1e-8 * np.abs(want).max(), c
        w = eng.ss_student_get_weights(c)
        assert np.array_equal(w, np.where(ob, W[c], 0.0)), c


# ---- 5. whole rounds ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", range(len(ROUND_CASES["student"])))
def test_rounds_match_restatement(oracle, k):
    """(the family's own loop: sigma^2 and nu are drawn, the weights stand where the others have value and
    precision, and the device reports margins of its own)"""
    c = round_case("student", k)
    eng = c["engine"]()
    ora = {ch: c["oracle"](oracle, ch) for ch in c["check"]}
    for r in range(c["rounds"]):
        eng.ss_student_sweep(1)   # (round 0: the start from all weights 1, two weight imputations)
        gam, beta, sig = eng.get_states()
        nu = eng.student_get_nu()
        for ch, o in ora.items():
            g, b, s2, v = o.draw()
            tag = (k, ch, r)
            assert np.array_equal(gam[ch], g), tag
            assert relerr(beta[ch], b) < RTOL, tag
            assert relerr(sig[ch], s2, 1e-300) < RTOL and relerr(nu[ch], v, 1e-300) < RTOL, tag
            assert sig[ch] <= c["smax"] ** 2
            assert relerr(eng.ss_student_get_weights(ch), o.w, 1e-300) < RTOL, tag
            checks.state_and_models_match(eng, o, c["blocks"], ch, tag)
    margin = eng.student_get_margin()
    for ch, o in ora.items():
        assert o.margin > 1e-9 and margin[ch] > 1e-9, (ch, o.margin, margin[ch])
    # several rounds in one call: the same draws
    eng2 = c["engine"]()
    eng2.ss_student_sweep(c["rounds"])
    for u, v in zip(eng.get_states(), eng2.get_states()):
        assert np.array_equal(u, v)
    assert np.array_equal(eng.student_get_nu(), eng2.student_get_nu())
    assert np.array_equal(eng.ss_get_state_draw(1), eng2.ss_get_state_draw(1))


# ---- 6. distribution ----------------------------------------------------------------------------
@gpu
def test_state_draws_have_the_dense_posterior_moments():
    blocks, S, var, y, obs, w, sigsq, nu, H = sso.fixed_case()
    T, chains = len(y), 4096
    X = np.ones((T, 1))
    g0 = np.zeros(1, np.uint8)
    eng = student_engine(chains, 20262, y, X, obs.astype(np.uint8), blocks, g0)
    eng.set_state(g0, np.zeros(1), sigsq)
    eng.student_set_nu(nu)
    eng.ss_student_set_weights(w)
    eng.ss_student_impute_state()
    checks.draws_have_the_moments(eng, chains, S, var, y, obs, H)


# ---- 7. interface -------------------------------------------------------------------------------
@gpu
def test_refusals_and_their_texts():
    import boom_amd
    T, p, X, (y,), _, blocks = STUDENT.small()
    mu, prec, pi = slab_of(p)
    g0 = np.zeros(p, np.uint8)
    eng = boom_amd.Engine(2, seed=1)
    checks.refusals_before_the_data(STUDENT, eng, T, X, y)
    # no state list
    eng.ss_student_set_data(y, X, None)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=True)
    eng.set_spike(pi)
    eng.set_sigma_prior(1.0, 1.0)
    checks.refusals_without_a_state_list(STUDENT, eng, level_mean=float(y[0]))
    eng.ss_set_state_models(blocks)
    eng.set_state(g0)
    # sweeps of other kinds
    for call in (lambda: eng.ss_sweep(1), lambda: eng.ss_impute_state(), lambda: eng.student_sweep(1),
                 lambda: eng.sweep(1), lambda: eng.sss_sweep(1), lambda: eng.quantile_sweep(1)):
        refused(call, "Student-t state-space data are set: use ba_ss_student_sweep")
    refused(lambda: eng.ss_forecast(np.zeros((2, p))), "forecasts with Student-t observation noise are not implemented")
    # weights
    for bad in (-1.0, np.nan, np.inf):
        w = np.ones(T)
        w[4] = bad
        refused(lambda: eng.ss_student_set_weights(w), "Weights must be finite and non-negative.")
    # a slab that does not scale with sigma^2
    checks.refusal_of_the_other_slab(STUDENT, eng, T, mu, prec, "scales with sigma^2 (scales_with_sigsq = 1)")


@gpu
def test_recorded_draws_and_get_state():
    checks.recorded_draws_and_get_state(STUDENT, recorded=(lambda a, n: a.student_get_nu_draws(0, n),
                                                           lambda b1: b1.student_get_nu(0)))


@gpu
def test_pybind_classes_agree_with_the_c_abi():
    """boom.StateSpaceStudentRegressionModel + StateSpaceStudentPosteriorSampler (the façade of
    include/boom_amd.hpp behind them): three rounds == the engine through the C-ABI on the same
    seed, bit for bit"""
    import boom_amd._boom as boom
    T, p, chains, seed = 40, 4, 3, 23
    X, y, _, obs = general_data(T, p, 2, [(4, 1)], seed=6, missing_frac=0.05)
    desc = [("level",), ("seasonal", 4, 1)]
    blocks = general_spec(y, desc)
    mu, prec, pi = slab_of(p)
    model = boom.StateSpaceStudentRegressionModel(y, X, [bool(o) for o in obs], chains=chains, seed=seed)
    for sm in checks.level_and_seasonal(boom, blocks):
        model.add_state(sm)
    sampler = boom.StateSpaceStudentPosteriorSampler(model, boom.MvnGivenScalarSigma(mu, prec),
                                                     boom.VariableSelectionPrior(pi), boom.ChisqModel(1.0, 1.0),
                                                     boom.UniformModel(0.1, 100.0))
    model.set_method(sampler)
    eng = student_engine(chains, seed, y, X, obs, blocks, np.zeros(p, np.uint8))
    checks.three_rounds_agree(STUDENT, model, eng)
    for c in range(chains):
        assert model.nu(c) == eng.student_get_nu(c) and model.sigsq(c) == eng.get_state(c)[2]
        assert np.array_equal(model.weights(c), eng.ss_student_get_weights(c))
