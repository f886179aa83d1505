"""Models of more than 64 variables: the HBM-resident sweep kernel
(boom_amd/csrc/ssvs_big_kernel.hip) behind the same C-ABI entry points.

The reference factors whatever k x k system the current model asks for
(BregVsSampler.cpp:395-426); the engine's LDS kernel stops at 64 variables, parks
the chain at a sweep boundary, and the large-model kernel picks it up -- the
draws must still be the oracle's, sweep for sweep (gamma bit-exact, beta /
sigma^2 within 1e-8).  VERDICT r1 item 2.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from cases import bsts_priors, regression_data, spike_slab_prior, state_space_data, suf_from_xy
from oracle_lib import ssvs_options
from test_ssvs_gpu import make_engine, relerr

pytestmark = pytest.mark.gpu
RTOL = 1e-8


def _oracle_runs(oracle, suf, prior, opts, seed, g0, nsw, chains):
    def run(c):
        return oracle.ssvs_run(suf, prior, opts, ("philox", seed, c), g0, nsw,
                               want_margin=True)
    with ThreadPoolExecutor(len(chains)) as ex:
        return dict(zip(chains, ex.map(run, chains)))


def test_hundred_signals_p256_sweep_for_sweep(oracle):
    """100 true signals at p = 256 from a cold start: every chain crosses 64
    variables inside its first sweeps (LDS capacities 32 -> 48 -> 64, then the
    HBM-resident kernel at 128)."""
    X, y, _ = regression_data(3000, 256, 100, seed=41)
    suf = oracle.neregsuf(X, y)
    prior = spike_slab_prior(suf, 100)
    g0 = np.zeros(256, np.uint8)
    g0[0] = 1
    chains, seed, nsw, step = 8, 19, 24, 6
    eng = make_engine(chains, seed, suf=suf, prior=prior, g0=g0)
    check = [0, 3, 7]
    ora = _oracle_runs(oracle, suf, prior, ssvs_options(), seed, g0, nsw, check)
    done = 0
    while done < nsw:
        eng.sweep(step)
        done += step
        gam, beta, sig = eng.get_states()
        for c in check:
            o = ora[c]
            assert o["status"] == 0
            assert np.array_equal(gam[c], o["gamma"][done - 1]), (c, done)
            assert relerr(beta[c], o["beta"][done - 1]) < RTOL, (c, done)
            assert abs(sig[c] - o["sigsq"][done - 1]) < RTOL * sig[c], (c, done)
    assert max(o["gamma"].sum(axis=1).max() for o in ora.values()) > 90
    sm = eng.get_summaries()
    assert sm["sweeps"] == chains * nsw
    assert sm["min_margin"] > 1e-9 and min(o["min_margin"] for o in ora.values()) > 1e-9
    inc = np.zeros(256)
    for c in check:
        inc += ora[c]["gamma"].sum(axis=0)
    assert np.all(sm["inclusion_count"] >= inc)
    # asynchronous launches queued behind chains that parked: nothing is lost
    eng2 = make_engine(chains, seed, suf=suf, prior=prior, g0=g0)
    for _ in range(nsw // step):
        eng2.sweep(step, sync=False)
    eng2.sync()
    a, b = eng.get_states(), eng2.get_states()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # a pinned capacity still turns this into the reported error
    import boom_amd
    eng3 = make_engine(chains, seed, suf=suf, prior=prior, g0=g0, max_model_size_hint=64)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng3.sweep(nsw)
    assert "working capacity" in str(ei.value)


def test_capacity_grows_past_128(oracle):
    """150 signals: the large-model kernel itself is outgrown (128 -> 256), the
    per-lane solves run over three panels"""
    X, y, _ = regression_data(4000, 320, 150, seed=59)
    suf = oracle.neregsuf(X, y)
    prior = spike_slab_prior(suf, 150)
    g0 = np.zeros(320, np.uint8)
    g0[0] = 1
    chains, seed, nsw = 3, 31, 8
    eng = make_engine(chains, seed, suf=suf, prior=prior, g0=g0)
    ora = _oracle_runs(oracle, suf, prior, ssvs_options(), seed, g0, nsw, [0, 2])
    for s in range(0, nsw, 2):
        eng.sweep(2)
        gam, beta, sig = eng.get_states()
        for c in (0, 2):
            o = ora[c]
            assert o["status"] == 0
            assert np.array_equal(gam[c], o["gamma"][s + 1]), (c, s)
            assert relerr(beta[c], o["beta"][s + 1]) < RTOL, (c, s)
            assert abs(sig[c] - o["sigsq"][s + 1]) < RTOL * sig[c], (c, s)
    assert max(o["gamma"].sum(axis=1).max() for o in ora.values()) > 140


def test_recorded_draws_and_lookahead_with_large_models(oracle):
    """every draw of one launch recorded (the record widens beyond 64 variables
    per draw), and ba_draw_next serving the same draws"""
    X, y, _ = regression_data(1500, 150, 75, seed=43)
    suf = oracle.neregsuf(X, y)
    prior = spike_slab_prior(suf, 75)
    g0 = np.zeros(150, np.uint8)
    g0[0] = 1
    chains, seed, nsw = 4, 23, 16
    eng = make_engine(chains, seed, suf=suf, prior=prior, g0=g0)
    eng.enable_draws(nsw)
    eng.sweep(nsw)
    ora = _oracle_runs(oracle, suf, prior, ssvs_options(), seed, g0, nsw, [0, 3])
    for c in (0, 3):
        gam, beta, sig = eng.get_draws(c, nsw)
        o = ora[c]
        assert o["gamma"].sum(axis=1).max() > 64
        for s in range(nsw):
            assert np.array_equal(gam[s], o["gamma"][s]), (c, s)
            assert relerr(beta[s], o["beta"][s]) < RTOL, (c, s)
            assert abs(sig[s] - o["sigsq"][s]) < RTOL * sig[s], (c, s)
    b = make_engine(chains, seed, suf=suf, prior=prior, g0=g0)
    b.set_lookahead(5)
    for s in range(nsw):
        b.draw_next()
        gam, beta, sig = b.get_states()
        for c in (0, 3):
            assert np.array_equal(gam[c], ora[c]["gamma"][s]), (c, s)
            assert relerr(beta[c], ora[c]["beta"][s]) < RTOL, (c, s)


def test_large_models_general_priors_and_swaps(oracle):
    """non-zero prior means (exact-path proposals), the correlation swap move
    with real candidates and a model-size cap above 64, all in the large-model
    kernel"""
    X, y, _ = regression_data(1200, 120, 70, seed=47, collinear=[1, 80, 90, 100])
    suf = oracle.neregsuf(X, y)
    pm = np.zeros(120)
    pm[[0, 5, 33, 77, 110]] = [0.5, -0.2, 0.1, 0.3, -0.4]
    prior = spike_slab_prior(suf, 70, prior_mean=pm)
    opts = ssvs_options(max_model_size=78, swap_threshold=0.5)
    g0 = np.zeros(120, np.uint8)
    g0[0] = 1
    chains, seed, nsw = 5, 29, 20
    eng = make_engine(chains, seed, suf=suf, prior=prior, opts=opts, g0=g0)
    ora = _oracle_runs(oracle, suf, prior, opts, seed, g0, nsw, [0, 4])
    for s in range(0, nsw, 5):
        eng.sweep(5)
        gam, beta, sig = eng.get_states()
        for c in (0, 4):
            o = ora[c]
            assert o["status"] == 0
            assert np.array_equal(gam[c], o["gamma"][s + 4]), (c, s)
            assert relerr(beta[c], o["beta"][s + 4]) < RTOL, (c, s)
            assert abs(sig[c] - o["sigsq"][s + 4]) < RTOL * sig[c], (c, s)
    assert gam.sum(axis=1).max() <= 78
    assert max(o["gamma"].sum(axis=1).max() for o in ora.values()) > 64


def test_dense_posterior_variant_p512(oracle):
    """SURVEY 8d's dense-posterior variant of config 2 (64 true signals, p=512):
    chains hover around the LDS kernel's limit, some on either side."""
    n, p, nsig, chains, seed = 10000, 512, 64, 256, 5
    X, y, _ = regression_data(n, p, nsig, seed=8675309)
    suf = suf_from_xy(X, y)
    prior = spike_slab_prior(suf, nsig)
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    eng = make_engine(chains, seed, suf=suf, prior=prior, g0=g0)
    nsw = 30
    eng.sweep(nsw)
    ora = _oracle_runs(oracle, suf, prior, ssvs_options(), seed, g0, nsw, [0, 255])
    gam, beta, sig = eng.get_states()
    for c in (0, 255):
        o = ora[c]
        assert np.array_equal(gam[c], o["gamma"][-1]), c
        assert relerr(beta[c], o["beta"][-1]) < RTOL, c
        assert abs(sig[c] - o["sigsq"][-1]) < RTOL * sig[c], c
    k = gam.sum(axis=1)
    assert k.min() >= 64 and k.max() > 64 and gam[:, :nsig].all()


def test_state_space_with_a_large_regression_model(oracle):
    """bsts path with more than 64 included regressors: (SSVS, Kalman) pairs keep
    alternating while chains live in the large-model kernel"""
    T, p, nsig = 600, 90, 72
    X, y, _, obs = state_space_data(T, p, nsig, seed=51)
    prior, ss, sig_up = bsts_priors(X, y, nsig)
    opts = ssvs_options(sigma_upper_limit=sig_up)
    g0 = np.zeros(p, np.uint8)
    import boom_amd
    eng = boom_amd.Engine(4, seed=13)
    eng.ss_set_data(y, X, obs)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"],
                   prior["sigma_guess"], sigma_upper_limit=sig_up)
    eng.ss_set_local_level(ss["level_df"], ss["level_sigma_guess"],
                           ss["level_sigma_upper_limit"], ss["initial_state_mean"],
                           ss["initial_state_variance"], ss["initial_level_sigma"])
    eng.set_state(g0)
    nsw = 11
    ora = {c: oracle.ss_run(y, X, obs, prior, opts, ss, ("philox", 13, c), g0, nsw)
           for c in (0, 3)}
    for s in range(nsw):
        eng.ss_sweep(1)
        gam, beta, sig = eng.get_states()
        for c in (0, 3):
            o = ora[c]
            assert o["status"] == 0
            assert np.array_equal(gam[c], o["gamma"][s]), (c, s)
            assert relerr(beta[c], o["beta"][s]) < RTOL, (c, s)
            st = eng.ss_get_state(c)
            assert np.max(np.abs(st["state"] - o["state"][s])) < 1e-8 * np.abs(o["state"][s]).max()
    assert max(o["gamma"].sum(axis=1).max() for o in ora.values()) > 64


def test_model_hovering_across_128_variables(oracle):
    """110 signals and a prior that lets about twenty of the 90 noise variables in: the model size
    settles around 128, the edge where the large-model kernel's proposals change from the matrix
    cores (k <= 128) to the per-lane panel solves and where two panels become three.  Every checked
    chain crosses it in both directions within the 12 sweeps -- asserted on the oracle's own trace
    before anything is compared."""
    from test_partial_rebuild_gpu import _crosses
    X, y, _ = regression_data(600, 200, 110, seed=61)
    suf = oracle.neregsuf(X, y)
    prior = spike_slab_prior(suf, 156, kappa=2.0)
    g0 = np.zeros(200, np.uint8)
    g0[0] = 1
    chains, seed, nsw, check = 3, 37, 12, [0, 1, 2]
    ora = _oracle_runs(oracle, suf, prior, ssvs_options(), seed, g0, nsw, check)
    for c in check:
        assert ora[c]["status"] == 0
        ksize = ora[c]["gamma"].sum(axis=1).astype(np.int64)[None, :]
        assert _crosses(ksize, 128), (c, ksize)
        assert ora[c]["min_margin"] > 1e-9
    eng = make_engine(chains, seed, suf=suf, prior=prior, g0=g0)
    for s in range(nsw):
        eng.sweep(1)
        gam, beta, sig = eng.get_states()
        for c in check:
            o = ora[c]
            assert np.array_equal(gam[c], o["gamma"][s]), (c, s)
            assert relerr(beta[c], o["beta"][s]) < RTOL, (c, s)
            assert abs(sig[c] - o["sigsq"][s]) < RTOL * sig[c], (c, s)
    assert eng.get_summaries()["min_margin"] > 1e-9


@pytest.mark.parametrize("p", [80, 150])
def test_rank_deficient_large_model_is_the_reference_error(oracle, p):
    """the same two failures as test_ssvs_gpu's rank-deficient case, on a model of more than 64
    variables: both of a build's factorisations fail (V_g has a zero column, the prior
    precision A_g is zero), each on its own wavefront of the large-model kernel since round 6 --
    the waves have to keep meeting at the build's barriers after either verdict.  p = 80: one
    panel and the matrix-core fills' inverses (k <= 128); p = 150: three panels, no inverses."""
    import boom_amd
    X, y, _ = regression_data(400, p, 3, seed=10)
    X[:, 70] = 0.0
    suf = oracle.neregsuf(X, y)
    prior = spike_slab_prior(suf, 3)
    prior["ominv"] = np.zeros((p, p))
    g0 = np.ones(p, np.uint8)
    for max_flips, want, msg in ((0, 1, "not positive definite"),
                                 (-1, 3, "did not start with a legal configuration")):
        opts = ssvs_options(max_flips=max_flips)
        o = oracle.ssvs_run(suf, prior, opts, ("philox", 3, 0), g0, 2)
        assert o["status"] == want
        eng = make_engine(3, 3, suf=suf, prior=prior, opts=opts, g0=g0)
        with pytest.raises(boom_amd.BoomAmdError) as ei:
            eng.sweep(2)
        assert msg in str(ei.value)
    # ... and a healthy model of the same size next: the engine's large-model state is intact
    X2, y2, _ = regression_data(400, p, 3, seed=11)
    suf2 = oracle.neregsuf(X2, y2)
    prior2 = spike_slab_prior(suf2, 3)
    g1 = np.ones(p, np.uint8)
    eng = make_engine(2, 5, suf=suf2, prior=prior2, g0=g1)
    ora = _oracle_runs(oracle, suf2, prior2, ssvs_options(), 5, g1, 2, [0, 1])
    eng.sweep(2)
    gam, beta, sig = eng.get_states()
    for c in (0, 1):
        assert ora[c]["status"] == 0
        assert np.array_equal(gam[c], ora[c]["gamma"][-1]), c
        assert relerr(beta[c], ora[c]["beta"][-1]) < RTOL, c
