"""The readers of the device's draw record through the C-ABI: ba_get_coefficient_traces (which
feeds the benchmark's ESS/s figure) against ba_get_draws bit for bit, and ba_predict against the
recorded draws in numpy.longdouble -- on a record of the 64-variable kernel and on one widened
by the large-model kernel, with 257 new rows (one past the predict kernel's 256-thread block).

Bound of a prediction: a sum of k products, k the draw's model size, so
|got - ref| <= gamma_k sum_j |beta_j x_ij| with gamma_k = k u / (1 - k u), u = 2^-53 (widened
by 2^-10 for the reference's own rounding at u = 2^-64)."""
import numpy as np
import pytest

from cases import regression_data, spike_slab_prior, suf_from_xy
from test_ssvs_gpu import make_engine

pytestmark = pytest.mark.gpu
LD = np.longdouble
U53 = 2.0 ** -53


def _small_engine(oracle):
    """the engine of test_predict_from_the_record (test_walk_modes_gpu.py): 40 variables"""
    import boom_amd
    X, y, _ = regression_data(500, 40, 5, seed=2)
    suf = suf_from_xy(X, y)
    prior = spike_slab_prior(suf, 5)
    eng = boom_amd.Engine(6, seed=9)
    eng.build_suf_from_xy(X, y)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"])
    g0 = np.zeros(40, np.uint8)
    g0[0] = 1
    eng.set_state(g0)
    return eng, 50, 12


def _wide_engine(oracle):
    """the engine of test_recorded_draws_and_lookahead_with_large_models (test_large_models_gpu.py):
    p = 150, 75 signals, the record widened beyond 64 variables per draw"""
    X, y, _ = regression_data(1500, 150, 75, seed=43)
    suf = oracle.neregsuf(X, y)
    prior = spike_slab_prior(suf, 75)
    g0 = np.zeros(150, np.uint8)
    g0[0] = 1
    return make_engine(4, 23, suf=suf, prior=prior, g0=g0), 16, 5


@pytest.fixture(scope="module", params=["p40", "p150_widened"])
def recorded(request, oracle):
    """the engine after enable_draws(nsw); sweep(nsw), and every chain's draws as ba_get_draws
    gives them (read once, shared by the tests below)"""
    eng, nsw, burn = (_small_engine if request.param == "p40" else _wide_engine)(oracle)
    eng.enable_draws(nsw)
    eng.sweep(nsw)
    draws = [eng.get_draws(c, nsw) for c in range(eng.chains)]
    gam = np.stack([d[0] for d in draws])
    beta = np.stack([d[1] for d in draws])
    if request.param == "p150_widened":
        assert gam.sum(axis=2).max() > 64       # (the record is the widened one)
    else:
        assert gam.sum(axis=2).max() <= 64
    return eng, nsw, burn, gam, beta


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_coefficient_traces_equal_the_draws(recorded):
    eng, nsw, _, gam, beta = recorded
    p = eng.p
    counts = gam.sum(axis=(0, 1)).astype(np.int64)
    never, often = np.flatnonzero(counts == 0), np.argsort(-counts)
    assert never.size > 0 and counts[often[3]] > 0
    # a never-included variable, the last variable, ones that come and go; then another list; a
    # list that names a variable twice (every place of it gets the path; before this test the
    # earlier places stayed zero); every variable
    lists = [[int(often[0]), int(never[0]), p - 1, int(often[3]), 0],
             [p - 1, int(often[1]), int(never[-1])],
             [int(often[0]), int(often[1]), int(often[0]), int(never[0]), int(often[0])],
             list(range(p))]
    for variables in lists:
        for n in (nsw, nsw - 3, 1):     # (fewer sweeps than the enabled length too)
            tr = eng.get_coefficient_traces(n, variables)
            assert tr.shape == (eng.chains, len(variables), n)
            for v, j in enumerate(variables):
                # [c, v, s] == draws of chain c [s, j], every chain, bit for bit
                assert np.array_equal(_bits(tr[:, v, :]), _bits(beta[:, :n, j])), (variables, n, j)
    tr = eng.get_coefficient_traces(nsw, [int(never[0])])
    assert np.all(_bits(tr) == 0)
    # reading changes nothing
    again = [eng.get_draws(c, nsw)[1] for c in range(eng.chains)]
    assert np.array_equal(_bits(np.stack(again)), _bits(beta))


def test_predict_matches_the_draws_in_longdouble(recorded):
    eng, nsw, burn, gam, beta = recorded
    p, nnew = eng.p, 257
    newX = np.random.Generator(np.random.PCG64(3)).standard_normal((nnew, p))
    got = eng.predict(newX, burn, nsw - burn)
    assert got.shape == (eng.chains, nsw - burn, nnew)
    Xl = newX.astype(LD)
    worst = 0.0
    for c in range(eng.chains):
        b = beta[c, burn:].astype(LD)
        ref, mag = b @ Xl.T, np.abs(b) @ np.abs(Xl).T
        k = gam[c, burn:].sum(axis=1).astype(float)
        bound = (LD(1.0 + 2.0 ** -10) * (k * U53 / (1.0 - k * U53)).astype(LD))[:, None] * mag
        err = np.abs(got[c].astype(LD) - ref)
        worst = max(worst, float(np.max(err / np.maximum(bound, LD(1e-300)))))
        assert np.all(err <= bound), (c, worst)
    print("predict, p = %d: largest share of the bound %.3g" % (p, worst))


def test_reader_refusals(recorded):
    import boom_amd
    eng, nsw, _, _, _ = recorded
    p = eng.p
    for variables, text in (([], "bad argument"), ([0, p], "variable index out of range"),
                            ([-1], "variable index out of range")):
        with pytest.raises(boom_amd.BoomAmdError) as ei:
            eng.get_coefficient_traces(nsw, variables)
        assert ei.value.code == -1 and str(ei.value) == text      # BA_E_INVALID
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.get_coefficient_traces(nsw + 1, [0])
    assert ei.value.code == -1 and str(ei.value) == "nsweeps out of range"


def test_readers_refuse_before_enable_draws():
    import boom_amd
    X, y, _ = regression_data(200, 8, 2, seed=4)
    suf = suf_from_xy(X, y)
    prior = spike_slab_prior(suf, 2)
    eng = boom_amd.Engine(2, seed=1)
    eng.build_suf_from_xy(X, y)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"])
    eng.set_state(np.ones(8, np.uint8))
    eng.sweep(3)
    for call in (lambda: eng.get_coefficient_traces(3, [0]), lambda: eng.predict(np.ones((2, 8)), 0, 3),
                 lambda: eng.get_draws(0, 3)):
        with pytest.raises(boom_amd.BoomAmdError) as ei:
            call()
        assert ei.value.code == -9 and str(ei.value) == "draw recording is not enabled"    # BA_E_STATE
