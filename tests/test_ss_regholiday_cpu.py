"""The restatement of RegressionHolidayStateModel (tests/ss_regholiday_oracle.py, the yardstick of
tests/test_ss_regholiday_gpu.py) pinned on what does not depend on it: a dense solve, the model built the
long way as a state component, and counts written out by hand.  No GPU."""
import numpy as np
import pytest

import ss_holiday_oracle as sho
import ss_regholiday_cases as src
import ss_regholiday_oracle as sro


@pytest.mark.parametrize("T", [70, 130])
def test_counts(T):
    """observed active steps per coefficient: a missing active day is not counted, a coefficient that is never
    active and one that is active on missing days only have count 0"""
    _, _, obs = src.data(T)
    models = src.models(T)
    got = sro.counts(models, obs, T)
    want = src.expected_counts(T)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert want[0][5] == 0 and want[1][2] == 0
    assert obs[12] == 0 and obs[62] == 0 and models[1]["calendar"][12] == 2 and models[0]["calendar"][62] == 0
    # two models on the same day, windows over t = 0, both time-block edges and T - 1
    c0, c1 = src.calendars(T)
    assert c0[63] >= 0 and c1[63] >= 0 and c0[64] >= 0 and c1[64] >= 0
    assert c0[0] >= 0 and c0[T - 1] >= 0 and (T < 129 or (c0[127] >= 0 and c0[128] >= 0))


@pytest.mark.parametrize("T", [70, 130])
def test_zero_normals_give_the_dummy_regression_posterior_mean(T):
    """with rnorm(mean, sd) = mean the coefficient draw is the conjugate posterior mean of the regression of
    y - x'beta - (everything else's contribution) on the model's dummies, by a dense solve, within 1e-12"""
    X, y, obs = src.data(T)
    models = src.models(T)
    rs = np.random.Generator(np.random.PCG64(T))
    beta = rs.standard_normal(src.P)
    zalpha = rs.standard_normal(T)   # (any state contribution of the other models)
    sigsq = 0.6
    coefs = [m["coefficients"] for m in models]
    totals = sro.observe(models, coefs, y, X @ beta, zalpha, obs)
    drawn = sro.draw(models, totals, sro.counts(models, obs, T), sigsq, lambda mean, sd: mean)
    for k, m in enumerate(models):
        # the response model k sees: the series less the regression, the state and the OTHER model's effect
        other = np.zeros(T)
        for t in range(T):
            es = sro.effects(models, coefs, t)
            other[t] = sum(e for j, e in enumerate(es) if j != k and e is not None)
        want = sro.dummies_posterior_mean(m, y - X @ beta - zalpha - other, obs, T, sigsq)
        assert np.max(np.abs(drawn[k] - want)) <= 1e-12 * max(1.0, np.abs(want).max()), (k, drawn[k] - want)


def test_count_zero_gives_the_priors_draw():
    T = 70
    _, _, obs = src.data(T)
    models = src.models(T)
    cnts = sro.counts(models, obs, T)
    totals = [np.zeros(6), np.zeros(4)]
    seen = []
    drawn = sro.draw(models, totals, cnts, 0.5, lambda mean, sd: seen.append((mean, sd)) or mean + sd * 0.25)
    for (k, j) in ((0, 5), (1, 2)):
        mu, tau = models[k]["prior"]
        mean, sd = sro.posterior(0.0, 0.0, 0.5, mu, tau)
        assert abs(mean - mu) <= 1e-15 * abs(mu) and abs(sd - tau) <= 1e-15 * tau
        assert abs(drawn[k][j] - (mu + 0.25 * tau)) <= 1e-15 * (abs(mu) + tau)
    assert len(seen) == 10   # (model, coefficient) order, one draw each


@pytest.mark.parametrize("T", [70, 130])
def test_impute_state_with_the_model_is_impute_state_on_the_offset_series(oracle, T):
    """the list with every model as a constant state component observed through Z_t = its coefficient (a0 = 1,
    P0 = 0, no error: it reads no normal) against the list without them on y - effect: the same state draw
    within 1e-12 of max |state|, and the constant stays 1"""
    import ctypes as C
    X, y, obs = src.data(T)
    base = src.list_small(y)
    models = src.models(T)
    coefs = [m["coefficients"] for m in models]
    rs = np.random.Generator(np.random.PCG64(T + 1))
    beta = rs.standard_normal(src.P)
    sigsq = 0.7
    ystar = y - X @ beta
    var = [np.array(b["initial_sigma"], dtype=float) ** 2 for b in base]
    H = np.full(T, sigsq)
    oracle.lib.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    oracle.lib.bo_rnorm.restype = C.c_double

    def stream():
        rng = oracle.rng_philox(5, 0, 2, 0)
        return rng, (lambda mu, sd: oracle.lib.bo_rnorm(C.byref(rng), float(mu), float(sd)))

    r1, n1 = stream()
    plain = sho.impute_state(sho.Structure(base), var, sro.offset_series(ystar, models, coefs), obs.astype(bool), H, n1)
    r2, n2 = stream()
    aug = sho.impute_state(sro.AugmentedStructure(base, models, coefs), var + [np.zeros(1)] * len(models), ystar,
                           obs.astype(bool), H, n2)
    assert r1.pos == r2.pos
    m = plain.shape[1]
    assert np.all(aug[:, m:] == 1.0)
    assert np.max(np.abs(aug[:, :m] - plain)) <= 1e-12 * np.abs(plain).max()


def test_forecast_offset_adds_the_effects_in_model_order():
    T = 70
    models = src.models(T)
    coefs = [m["coefficients"] for m in models]
    out = sro.forecast_offset(np.zeros(src.HORIZON), models, coefs, T)
    want = np.zeros(src.HORIZON)
    want[1] = coefs[1][3]
    want[3], want[4] = coefs[0][3], coefs[0][4]
    assert np.array_equal(out, want)
