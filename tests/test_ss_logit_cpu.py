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

import ss_logit_oracle as slo
from test_oracle_golden import load


def relerr(a, b, floor=1e-3):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


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
    from test_ss_logit_gpu import binomial_series, slab_of, spec
    T, p = 30, 3
    X, successes, trials, series = binomial_series(T, p, 3, max_trials=8, seasons=4)   # (both branches at threshold 5)
    obs = np.ones(T, np.uint8)
    obs[[4, 17]] = 0
    blocks = spec(series, [("trend",), ("seasonal", 4, 1)])
    if nan_at_missing:
        successes, trials = successes.copy(), trials.copy()
        successes[[4, 17]] = np.nan
        trials[[4, 17]] = np.nan
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    return X, successes, trials, obs, blocks, slab_of(p), g0


def test_first_draw(oracle):
    X, successes, trials, obs, blocks, (mu, prec, pi), g0 = small_case()
    assert trials.min() < trials.max()
    o = slo.SsLogitOracle(oracle, successes, trials, X, obs, blocks, mu, prec, pi, 7, 1, g0)
    o.impute_state()
    ob = obs.astype(bool)
    Xo, q0 = X[ob], 4.0 / trials[ob]
    xqx = Xo.T @ (Xo * q0[:, None])
    assert np.allclose(o.xtx, xqx, rtol=1e-14, atol=0)
    assert np.allclose(o.xty, -(Xo.T @ (o.offset()[ob] * q0)), rtol=1e-12, atol=1e-13)
    # ... and draw() from the start: the first imputation uses up s = 0 and stores nothing
    o = slo.SsLogitOracle(oracle, successes, trials, X, obs, blocks, mu, prec, pi, 7, 1, g0)
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
    assert imputations == 1 and np.all(v == 0) and np.array_equal(q, np.where(ob, 4.0 / trials, 0.0))
    assert np.allclose(xtx, xqx, rtol=1e-14, atol=0)
    assert np.all(o.q[ob] > 0) and np.all(o.q[~ob] == 0) and np.all(np.isfinite(o.state))


def test_missing_steps_read_neither_successes_nor_trials(oracle):
    runs = []
    for nan in (False, True):
        X, successes, trials, obs, blocks, (mu, prec, pi), g0 = small_case(nan)
        o = slo.SsLogitOracle(oracle, successes, trials, X, obs, blocks, mu, prec, pi, 7, 0, g0)
        for _ in range(3):
            o.draw()
        runs.append((o.gamma.copy(), o.beta.copy(), o.v.copy(), o.q.copy(), o.state.copy()))
    for a, b in zip(*runs):
        assert np.all(np.isfinite(b)) and np.array_equal(a, b)


def test_parity_seeds_keep_their_margins(oracle):
    """the whole-round cases of the device test: every checked chain's smallest branch margin
    stays above 1e-9 over the rounds compared (a seed that does not is changed, not the bar), and
    no binomial draw takes BTPE, whose comparisons the record does not hold"""
    from test_ss_logit_gpu import ROUND_CASES, round_case
    for k in range(len(ROUND_CASES)):
        c = round_case(k)
        # n min(p, 1 - p) <= n / 2 < 30 whatever the linear predictor
        assert c["trials"].max() / 2 < 30
        oracle.set_slot_limit(c["slots"])
        try:
            for chain in c["check"]:
                o = c["oracle"](oracle, chain)
                for _ in range(c["rounds"]):
                    o.draw()
                print("case %d chain %d: margin %.3e, BTPE draws %d" % (k, chain, o.margin, o.btpe))
                assert o.margin > 1e-9, (k, chain, o.margin)
                assert o.btpe == 0, (k, chain, o.btpe)
        finally:
            oracle.set_slot_limit(0)


def test_recovery_data_have_clear_signals_and_quiet_nulls():
    """a binomial logistic regression by Newton's method with the generating state as offset: the
    coefficients' z-scores (see the docstring of test_ss_logit_recovers_the_signals)"""
    from test_ss_logit_gpu import RECOVERY_COEF, recovery_data
    X, successes, trials, _, path = recovery_data(with_path=True)
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
