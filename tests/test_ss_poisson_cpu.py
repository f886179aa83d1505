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

import ss_family_checks as checks
import ss_poisson_oracle as spo
from golden_lib import _golden_mix, load
from ss_family_cases import RECOVERY_COEF, count_series, recovery_data, relerr
from ss_family_checks import POISSON


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
    return checks.small_case(count_series(30, 3, 3, seasons=4), nan_at_missing)


def test_first_draw(oracle):
    checks.first_draw(POISSON, oracle, small_case(), lambda data: np.ones(len(data[0])))   # (a new model: q = 1)


def test_missing_steps_read_neither_count_nor_exposure(oracle):
    checks.missing_steps_read_no_data(POISSON, oracle, small_case)


def test_parity_seeds_keep_their_margins(oracle):
    """the whole-round cases of the device test: every checked chain's smallest branch margin
    stays above 1e-9 over the rounds compared (a seed that does not is changed, not the bar)"""
    def end(k, chain, o):
        print("case %d chain %d: margin %.3e" % (k, chain, o.margin))
        assert o.margin > 1e-9, (k, chain, o.margin)
    checks.parity_seeds_keep_their_margins(POISSON, oracle, end)


def test_recovery_data_have_clear_signals_and_quiet_nulls():
    """a Poisson regression by Newton's method with offset log(exposure) + the generating state:
    the coefficients' z-scores (see the docstring of test_ss_poisson_recovers_the_signals)"""
    X, counts, exposure, _, path = recovery_data("poisson", with_path=True)
    p = X.shape[1]
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
