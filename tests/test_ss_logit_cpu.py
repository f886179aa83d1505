"""The yardstick of the state space logit family (tests/ss_logit_oracle.py) checked on the CPU
before the device is compared with it:
  1. its imputer, with offset 0 and every step observed, followed by the oracle's SpikeSlabSampler
     (BinomialLogitSpikeSlabSampler's shuffle) on X'QX and X'(sum), reproduces Oracle.logit_run
     (the C restatement pinned on the compiled reference by tests/golden/logit_*.npz): indicators
     equal, beta within 1e-10 relative -- the two differ in the order of sums over n <= 300 terms;
     another branch taken, a wrong trun_norm_moments or a wrong rmultinom would show as order 1;
  2. the first draw(): the statistics after the first impute_state are those of v = 0,
     q = 4 / n_t, the first imputation leaves them alone, and round r imputes with s = r + 1;
  3. a missing step's successes and trials are never read (NaN there changes nothing);
  4. the seeds of the device's whole-round cases (tests/test_ss_logit_gpu.py) keep the imputer's
     branch margins above 1e-9 on the checked chains, and none of their binomial draws reaches
     BTPE (n min(p, 1 - p) < 30 everywhere), so every branch comparison is under the record;
  5. the data of the device's signal-recovery test are data on which the thresholds it asserts
     are what a correct sampler gives: by a plain binomial logistic regression with the generating
     state as offset, the two signals have |z| > 10 and every null predictor |z| < 1.
"""
import numpy as np
import pytest

import ss_family_checks as checks
import ss_logit_oracle as slo
from golden_lib import load
from ss_family_cases import RECOVERY_COEF, binomial_series, recovery_data, relerr
from ss_family_checks import LOGIT


@pytest.mark.parametrize("name", ["logit_bernoulli", "logit_binomial4", "logit_binomial60_large_sample",
                                  "logit_binomial200_large_sample"])
def test_imputer_reproduces_the_pinned_regression_sampler(oracle, name):
    g = load(name)
    X, y, nt = g["X"], g["y"], g["ntrials"]
    p = X.shape[1]
    seed, chain, nsw, clt = 19, 2, 6, int(g["clt_threshold"])
    ref = oracle.logit_run(X, y, nt, dict(mu=g["mu"], prec=g["prec"]), g["pi"], ("philox", seed, chain),
                           g["init_gamma"], np.zeros(p), nsw, clt_threshold=clt, max_flips=int(g["max_flips"]))
    assert ref["status"] == 0
    G, B, rec = slo.logit_regression_rounds(oracle, X, y, nt, g["mu"], g["prec"], g["pi"], seed, chain,
                                            g["init_gamma"], nsw, clt_threshold=clt, max_flips=int(g["max_flips"]))
    print("largest relative difference of beta %.3e, smallest branch margin %.3e, BTPE draws %d"
          % (relerr(B, ref["beta"]), rec.margin, rec.btpe))
    assert np.array_equal(G, ref["gamma"])
    assert relerr(B, ref["beta"]) < 1e-10


def small_case(nan_at_missing=False):
    return checks.small_case(binomial_series(30, 3, 3, max_trials=8, seasons=4), nan_at_missing)   # (both branches at threshold 5)


def test_first_draw(oracle):
    case = small_case()
    trials = case[1][1]
    assert trials.min() < trials.max()
    checks.first_draw(LOGIT, oracle, case, lambda data: 4.0 / data[1])   # (a new model: q = 4 / n_t)


def test_missing_steps_read_neither_successes_nor_trials(oracle):
    checks.missing_steps_read_no_data(LOGIT, oracle, small_case)


def test_parity_seeds_keep_their_margins(oracle):
    """the whole-round cases of the device test: every checked chain's smallest branch margin
    stays above 1e-9 over the rounds compared (a seed that does not is changed, not the bar), and
    no binomial draw takes BTPE, whose comparisons the record does not hold"""
    def before(c):
        # n min(p, 1 - p) <= n / 2 < 30 whatever the linear predictor
        assert c["trials"].max() / 2 < 30

    def end(k, chain, o):
        print("case %d chain %d: margin %.3e, BTPE draws %d" % (k, chain, o.margin, o.btpe))
        assert o.margin > 1e-9, (k, chain, o.margin)
        assert o.btpe == 0, (k, chain, o.btpe)
    checks.parity_seeds_keep_their_margins(LOGIT, oracle, end, before)


def test_recovery_data_have_clear_signals_and_quiet_nulls():
    """a binomial logistic regression by Newton's method with the generating state as offset: the
    coefficients' z-scores (see the docstring of test_ss_logit_recovers_the_signals)"""
    X, successes, trials, _, path = recovery_data("logit", with_path=True)
    p = X.shape[1]
    b = np.zeros(p)
    for _ in range(50):
        pr = 1 / (1 + np.exp(-(path + X @ b)))
        H = X.T @ (X * (trials * pr * (1 - pr))[:, None])
        b = b + np.linalg.solve(H, X.T @ (successes - trials * pr))
    se = np.sqrt(np.diag(np.linalg.inv(H)))
    z = b / se
    print("z-scores", np.round(z, 2), "standard errors", np.round(se, 3))
    k = len(RECOVERY_COEF)
    assert np.abs(z[:k]).min() > 10 and np.abs(z[k:]).max() < 1 and se.max() < 0.05
