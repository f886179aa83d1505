"""The yardstick of the state space Poisson family (tests/ss_poisson_oracle.py) checked on the
CPU before the device is compared with it:
  1. its imputer, with offset 0 and every step observed, followed by the oracle's SpikeSlabSampler
     on X'QX and X'Qv, reproduces Oracle.poisson_run (the C restatement pinned on the compiled
     reference by tests/golden/poisson_*.npz): indicators equal, beta within 1e-10 relative -- the
     two differ in the order of sums over n = 300 terms, about 7e-14; another branch taken would
     show as order 1;
  2. the first draw(): the statistics after the first impute_state are those of v = 0, q = 1, the
     first imputation leaves them alone, and round r imputes with s = r + 1;
  3. a missing step's count and exposure are never read (NaN there changes nothing);
  4. the seeds of the device's whole-round cases (tests/test_ss_poisson_gpu.py) keep the imputer's
     branch margins above 1e-9 on the checked chains;
  5. the data of the device's signal-recovery test are data on which the thresholds it asserts
     are what a correct sampler gives: by a plain Poisson regression with the generating state as
     offset, the two signals have |z| > 10 and every null predictor |z| < 1.
"""
import numpy as np
import pytest

import ss_poisson_oracle as spo
from test_oracle_golden import _golden_mix, load


def relerr(a, b, floor=1e-3):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


@pytest.mark.parametrize("name", ["poisson_exposure", "poisson_small_counts"])
def test_imputer_reproduces_the_pinned_regression_sampler(oracle, name):
    g = load(name)
    X, y, ex, mix = g["X"], g["y"], g["exposure"], _golden_mix(g)
    p = X.shape[1]
    seed, chain, nsw = 19, 2, 25
    ref = oracle.poisson_run(X, y, ex, dict(mu=g["mu"], prec=g["prec"]), g["pi"], mix, ("philox", seed, chain),
                             g["init_gamma"], np.zeros(p), nsw, max_flips=int(g["max_flips"]))
    assert ref["status"] == 0
    G, B, margin = spo.poisson_regression_rounds(oracle, X, y, ex, mix, g["mu"], g["prec"], g["pi"], seed, chain,
                                                 g["init_gamma"], nsw, max_flips=int(g["max_flips"]))
    print("largest relative difference of beta %.3e, smallest branch margin %.3e" % (relerr(B, ref["beta"]), margin))
    assert np.array_equal(G, ref["gamma"])
    assert relerr(B, ref["beta"]) < 1e-10


def small_case(nan_at_missing=False):
    from test_ss_poisson_gpu import count_series, golden_mix, slab_of, spec
    T, p = 30, 3
    X, counts, exposure, series = count_series(T, p, 3, seasons=4)
    obs = np.ones(T, np.uint8)
    obs[[4, 17]] = 0
    blocks = spec(series, [("trend",), ("seasonal", 4, 1)])
    if nan_at_missing:
        counts, exposure = counts.copy(), exposure.copy()
        counts[[4, 17]] = np.nan
        exposure[[4, 17]] = np.nan
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    return X, counts, exposure, obs, blocks, golden_mix(), slab_of(p), g0


def test_first_draw(oracle):
    X, counts, exposure, obs, blocks, mix, (mu, prec, pi), g0 = small_case()
    o = spo.SsPoissonOracle(oracle, counts, exposure, X, obs, blocks, mix, mu, prec, pi, 7, 1, g0)
    o.impute_state()
    ob = obs.astype(bool)
    Xo = X[ob]
    assert np.allclose(o.xtx, Xo.T @ Xo, rtol=1e-14, atol=0)
    assert np.allclose(o.xty, -(Xo.T @ o.offset()[ob]), rtol=1e-12, atol=1e-13)
    # ... and draw() from the start: the first imputation uses up s = 0 and stores nothing
    o = spo.SsPoissonOracle(oracle, counts, exposure, X, obs, blocks, mix, mu, prec, pi, 7, 1, g0)
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
    assert imputations == 1 and np.all(v == 0) and np.array_equal(q, ob.astype(float))
    assert np.allclose(xtx, Xo.T @ Xo, rtol=1e-14, atol=0)
    assert np.all(o.q[ob] > 0) and np.all(o.q[~ob] == 0) and np.all(np.isfinite(o.state))


def test_missing_steps_read_neither_count_nor_exposure(oracle):
    runs = []
    for nan in (False, True):
        X, counts, exposure, obs, blocks, mix, (mu, prec, pi), g0 = small_case(nan)
        o = spo.SsPoissonOracle(oracle, counts, exposure, X, obs, blocks, mix, mu, prec, pi, 7, 0, g0)
        for _ in range(3):
            o.draw()
        runs.append((o.gamma.copy(), o.beta.copy(), o.v.copy(), o.q.copy(), o.state.copy()))
    for a, b in zip(*runs):
        assert np.all(np.isfinite(b)) and np.array_equal(a, b)


def test_parity_seeds_keep_their_margins(oracle):
    """the whole-round cases of the device test: every checked chain's smallest branch margin
    stays above 1e-9 over the rounds compared (a seed that does not is changed, not the bar)"""
    from test_ss_poisson_gpu import ROUND_CASES, round_case
    for k in range(len(ROUND_CASES)):
        c = round_case(k)
        oracle.set_slot_limit(c["slots"])
        try:
            for chain in c["check"]:
                o = c["oracle"](oracle, chain)
                for _ in range(c["rounds"]):
                    o.draw()
                print("case %d chain %d: margin %.3e" % (k, chain, o.margin))
                assert o.margin > 1e-9, (k, chain, o.margin)
        finally:
            oracle.set_slot_limit(0)


def test_recovery_data_have_clear_signals_and_quiet_nulls():
    """a Poisson regression by Newton's method with offset log(exposure) + the generating state:
    the coefficients' z-scores (see the docstring of test_ss_poisson_recovers_the_signals)"""
    from test_ss_poisson_gpu import RECOVERY_COEF, RECOVERY_SEED, RECOVERY_SHAPE, count_series
    T, p = RECOVERY_SHAPE
    X, counts, exposure, _, path = count_series(T, p, RECOVERY_SEED, coef=RECOVERY_COEF, with_path=True)
    assert counts.max() < 26   # (the clip did not bind)
    off = np.log(exposure) + path
    b = np.zeros(p)
    for _ in range(50):
        mu = np.exp(off + X @ b)
        H = X.T @ (X * mu[:, None])
        b = b + np.linalg.solve(H, X.T @ (counts - mu))
    se = np.sqrt(np.diag(np.linalg.inv(H)))
    z = b / se
    print("z-scores", np.round(z, 2), "standard errors", np.round(se, 3))
    k = len(RECOVERY_COEF)
    assert np.abs(z[:k]).min() > 10 and np.abs(z[k:]).max() < 1 and se.max() < 0.05
