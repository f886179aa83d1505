"""QuantileRegressionSpikeSlabSampler on the device (ba_quantile_*): the inverse-Gaussian
weight imputation and the sweep at sigma^2 = 1 on the weighted suf -- against the Python
restatement of draw() on the same substreams (tests/quantile_oracle.py), against quadrature,
against a separately written Gibbs sampler, and on its behaviour.

Bars (those of tests/test_student_gpu.py): inclusion indicators bit-exact, beta within 1e-8
relative.  Every parity case asserts that the restatement's smallest non-zero residual stayed
above 1e-7: the weight's mean is 1 / |r|, so below that a rounding of the residual is no
longer small against the beta bar.
"""
import numpy as np
import pytest

from quantile_oracle import QuantileOracle

pytestmark = pytest.mark.gpu
RTOL = 1e-8
MIN_R = 1e-7
USE_Q = "quantile regression data are set: use ba_quantile_sweep"
Q_FIRST = "call ba_quantile_set_data first"


def relerr(a, b, floor=1e-3):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def make_data(n, p, nsig, seed, scale=0.5):
    """an intercept and standard normal predictors, nsig signals, Laplace errors (the check
    loss's own error law at q = 0.5)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    X[:, 0] = 1.0
    beta = np.zeros(p)
    beta[:nsig] = rng.choice([-2.0, -1.0, 1.0, 1.5], nsig)
    y = X @ beta + scale * rng.laplace(size=n)
    return X, y, beta


def make_engine(chains, seed, X, y, q, mu, prec, pi, g0, max_flips=-1, beta0=None, **kw):
    import boom_amd
    eng = boom_amd.Engine(chains, seed=seed, **kw)
    eng.quantile_set_data(X, y, q)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=False, max_flips=max_flips)
    eng.set_spike(pi)
    eng.set_state(g0, beta0)
    return eng


def check_parity(eng, ora, nsweeps, each=None):
    """nsweeps single sweeps of the engine against the restatements ora (local chain ->
    QuantileOracle) at the file's bars; each(s, gamma, beta) sees the engine's state after
    sweep s"""
    for s in range(nsweeps):
        eng.quantile_sweep(1)
        gam, beta, sig = eng.get_states()
        assert np.all(sig == 1.0)
        if each is not None:
            each(s, gam, beta)
        for c, o in ora.items():
            g, b = o.draw()
            assert np.array_equal(gam[c], g), (c, s)
            assert relerr(beta[c], b) < RTOL, (c, s)
    for c, o in ora.items():
        assert min(o.min_abs_r) > MIN_R, (c, min(o.min_abs_r))


CASES = [
    # n, p, signals, q, max_flips, slab mean
    (300, 10, 3, 0.5, -1, 0.0),
    (800, 24, 5, 0.9, 6, 0.0),
    (500, 70, 8, 0.1, 12, 0.0),
    (600, 16, 4, 0.25, -1, 0.3),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_quantile_sweeps_match_restatement(oracle, case):
    n, p, nsig, q, mf, mu0 = CASES[case]
    X, y, _ = make_data(n, p, nsig, 200 + case)
    mu, prec = np.full(p, mu0), 0.1 * np.eye(p)
    pi = np.full(p, min(0.9, 5.0 / p))
    g0 = np.zeros(p, np.uint8)
    g0[:2] = 1
    chains, seed, nsw = 6, 71 + case, 25
    eng = make_engine(chains, seed, X, y, q, mu, prec, pi, g0, max_flips=mf)
    ora = {c: QuantileOracle(oracle, X, y, q, mu, prec, pi, seed, c, g0, max_flips=mf) for c in (0, chains - 1)}
    check_parity(eng, ora, nsw)
    # several sweeps in one call: the same draws
    eng2 = make_engine(chains, seed, X, y, q, mu, prec, pi, g0, max_flips=mf)
    eng2.quantile_sweep(nsw)
    a, b = eng.get_states(), eng2.get_states()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("q", [0.05, 0.5, 0.95])
def test_quantile_weights_match_the_imputation(oracle, q):
    """The weights alone, after one sweep from a set state.  The two sides' residuals differ by
    the order of a sum of k + 1 terms (and the device's fused multiply-adds), i.e. by at most
    (k + 1) 2^-52 s_i with s_i = |y_i| + sum_j |x_ij beta_j|; mu = 1 / r takes that relative
    error s_i / |r_i| times over, both roots have a log-derivative in mu between 0 and 2, and
    the root's own few roundings are the 1e-12: |dw| / w <= 1e-12 + 4 (k + 4) 2^-52 s_i / |r_i|.
    Then the sweep's beta, which reads X'Wz and so the shift 1 - 2 q of z."""
    n, p = 700, 12
    X, y, _ = make_data(n, p, 3, 3)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.3)
    g0 = np.zeros(p, np.uint8)
    g0[:3] = 1
    k = 3
    beta0 = np.linspace(0.5, 1.5, p)
    chains, seed = 3, 77
    eng = make_engine(chains, seed, X, y, q, mu, prec, pi, g0, beta0=beta0)
    eng.quantile_sweep(1)
    gam, beta, _ = eng.get_states()
    s_i = np.abs(y) + np.abs(X[:, :k] * beta0[:k]).sum(axis=1)
    for c in range(chains):
        o = QuantileOracle(oracle, X, y, q, mu, prec, pi, seed, c, g0, beta0=beta0)
        g, b = o.draw()
        w_dev, w_ora, r = eng.quantile_get_weights(c), o.weights, o.residuals
        assert np.all(r > MIN_R) and np.all(w_ora > 0)
        bound = 1e-12 + 4 * (k + 4) * 2.0 ** -52 * s_i / r
        excess = np.abs(w_dev - w_ora) / w_ora / bound
        print("q %.2f chain %d: largest |dw| / w %.3g, largest share of the bound %.3g"
              % (q, c, float(np.max(np.abs(w_dev - w_ora) / w_ora)), float(excess.max())))
        assert np.all(excess <= 1.0), (c, float(excess.max()))
        assert np.array_equal(gam[c], g), c
        assert relerr(beta[c], b) < RTOL, c


@pytest.mark.parametrize("n", [37, 256, 257])
def test_quantile_small_n_and_block_edges(oracle, n):
    """n below one impute block, exactly one block, and one past it"""
    p = 6
    X, y, _ = make_data(n, p, 2, 400 + n)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.5)
    g0 = np.zeros(p, np.uint8)
    g0[:2] = 1
    chains, seed = 6, 60 + n
    eng = make_engine(chains, seed, X, y, 0.3, mu, prec, pi, g0)
    ora = {c: QuantileOracle(oracle, X, y, 0.3, mu, prec, pi, seed, c, g0) for c in (0, chains - 1)}
    check_parity(eng, ora, 15)


def test_quantile_empty_starting_model(oracle):
    """k = 0: eta is 0 for every observation of the first sweep"""
    n, p = 300, 8
    X, y, _ = make_data(n, p, 3, 17)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.4)
    g0 = np.zeros(p, np.uint8)
    chains, seed = 4, 23
    eng = make_engine(chains, seed, X, y, 0.6, mu, prec, pi, g0)
    ora = {c: QuantileOracle(oracle, X, y, 0.6, mu, prec, pi, seed, c, g0) for c in (0, chains - 1)}
    check_parity(eng, ora, 12)


def test_quantile_more_than_256_variables(oracle):
    """p = 260: the included-variable compaction runs in two chunks of 256, with included
    variables on both sides of 256"""
    n, p = 400, 260
    rng = np.random.default_rng(260)
    X = rng.standard_normal((n, p))
    X[:, 0] = 1.0
    sig_idx = [0, 255, 256, 259]
    truth = np.zeros(p)
    truth[sig_idx] = [1.0, 1.5, -1.0, 2.0]
    y = X @ truth + 0.5 * rng.laplace(size=n)
    mu, prec = np.zeros(p), 0.1 * np.eye(p)
    pi = np.full(p, 0.01)
    pi[sig_idx] = 0.9
    g0 = np.zeros(p, np.uint8)
    g0[sig_idx] = 1
    chains, seed = 2, 52
    eng = make_engine(chains, seed, X, y, 0.4, mu, prec, pi, g0)
    ora = {c: QuantileOracle(oracle, X, y, 0.4, mu, prec, pi, seed, c, g0) for c in range(chains)}

    def straddles(s, gam, beta):
        for c in range(chains):
            inc = np.flatnonzero(gam[c])
            assert inc.min() < 256 and inc.max() >= 256, (c, s)
    check_parity(eng, ora, 5, straddles)


def test_quantile_large_model_escalates(oracle):
    """a model of more than 64 variables: the chains move to the large-model kernel"""
    n, p = 600, 72
    X, y, _ = make_data(n, p, 70, 7)
    mu, prec = np.zeros(p), 0.1 * np.eye(p)
    pi = np.full(p, 0.97)
    g0 = np.ones(p, np.uint8)
    chains, seed = 4, 5
    eng = make_engine(chains, seed, X, y, 0.5, mu, prec, pi, g0)
    ora = {c: QuantileOracle(oracle, X, y, 0.5, mu, prec, pi, seed, c, g0) for c in (0, chains - 1)}

    def large(s, gam, beta):
        for c in ora:
            assert gam[c].sum() > 64, (c, s)
    check_parity(eng, ora, 8, large)
    for o in ora.values():
        assert o.gamma.sum() > 64


def test_quantile_many_chains(oracle):
    """1024 chains, draw for draw at the first, a middle and the last (high blockIdx.y)"""
    n, p = 64, 6
    X, y, _ = make_data(n, p, 2, 1024)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.5)
    g0 = np.zeros(p, np.uint8)
    g0[:2] = 1
    chains, seed = 1024, 88
    eng = make_engine(chains, seed, X, y, 0.7, mu, prec, pi, g0)
    ora = {c: QuantileOracle(oracle, X, y, 0.7, mu, prec, pi, seed, c, g0) for c in (0, 511, 1023)}
    check_parity(eng, ora, 10)


def test_quantile_more_chains_than_the_request_batch(oracle):
    """33 000 chains: more than the 32 768 requests of one column launch, so the planes workspace
    is sized by its other user, the rows products of every chain at once (planes_sizing.h; sized
    by the batch alone it was 232 chains short here).  The first chain, the first one past the
    batch and the last against the restatement at the file's bars; chains 0 and 1023 bit for bit
    those of a 1024-chain engine on the same data and seed."""
    n, p = 64, 4
    X, y, _ = make_data(n, p, 2, 33000)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.5)
    g0 = np.zeros(p, np.uint8)
    g0[:2] = 1
    chains, seed, nsw = 33000, 93, 3
    eng = make_engine(chains, seed, X, y, 0.4, mu, prec, pi, g0)
    ora = {c: QuantileOracle(oracle, X, y, 0.4, mu, prec, pi, seed, c, g0) for c in (0, 32768, chains - 1)}
    check_parity(eng, ora, nsw)
    small = make_engine(1024, seed, X, y, 0.4, mu, prec, pi, g0)
    small.quantile_sweep(nsw)
    a, b = eng.get_states(), small.get_states()
    for c in (0, 1023):
        assert np.array_equal(a[0][c], b[0][c]) and np.array_equal(a[1][c].view(np.uint64), b[1][c].view(np.uint64)), c


def test_quantile_chain_offset(oracle):
    """an engine whose chains are 5 and 6 of a larger run reads those chains' substreams"""
    n, p = 200, 6
    X, y, _ = make_data(n, p, 2, 31)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.5)
    g0 = np.zeros(p, np.uint8)
    g0[:2] = 1
    seed = 14
    eng = make_engine(2, seed, X, y, 0.5, mu, prec, pi, g0, chain_offset=5)
    ora = {c: QuantileOracle(oracle, X, y, 0.5, mu, prec, pi, seed, 5 + c, g0) for c in (0, 1)}
    check_parity(eng, ora, 8)
    # ... which are not those of chains 0 and 1
    plain = make_engine(2, seed, X, y, 0.5, mu, prec, pi, g0)
    plain.quantile_sweep(8)
    assert not np.array_equal(plain.get_states()[1], eng.get_states()[1])


def test_quantile_forced_spill(oracle):
    """a slot that serves two numbers: the normal takes both (or more), the uniform -- and the
    rest of a slow normal -- come from the slot's spill stream, on both sides"""
    n, p = 300, 8
    X, y, _ = make_data(n, p, 3, 44)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.4)
    g0 = np.zeros(p, np.uint8)
    g0[:2] = 1
    chains, seed = 4, 9
    eng = make_engine(chains, seed, X, y, 0.5, mu, prec, pi, g0)
    eng.set_slot_limit(2)
    ref = make_engine(chains, seed, X, y, 0.5, mu, prec, pi, g0)
    ora = {c: QuantileOracle(oracle, X, y, 0.5, mu, prec, pi, seed, c, g0) for c in (0, chains - 1)}
    oracle.set_slot_limit(2)
    try:
        check_parity(eng, ora, 5)
    finally:
        oracle.set_slot_limit(0)
    ref.quantile_sweep(5)
    assert not np.array_equal(ref.get_states()[1], eng.get_states()[1])   # (the switch does something)


def test_quantile_zero_residuals(oracle):
    """exact zero residuals (empty model, y exactly 0): weight 0, nothing read, the observation
    out of that sweep's regression; the chains go on and their status stays OK"""
    n, p = 200, 5
    X, y, _ = make_data(n, p, 2, 91)
    zeros = [0, 63, 64, n - 1]
    y[zeros] = 0.0
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.4)
    g0 = np.zeros(p, np.uint8)
    chains, seed = 3, 37
    eng = make_engine(chains, seed, X, y, 0.35, mu, prec, pi, g0)
    ora = {c: QuantileOracle(oracle, X, y, 0.35, mu, prec, pi, seed, c, g0) for c in range(chains)}
    check_parity(eng, ora, 1)
    others = np.setdiff1d(np.arange(n), zeros)
    for c, o in ora.items():
        w = eng.quantile_get_weights(c)
        assert np.all(w[zeros] == 0.0) and np.all(o.weights[zeros] == 0.0)
        assert np.all(np.isfinite(w[others])) and np.all(w[others] > 0)
    check_parity(eng, ora, 9)
    eng.sync()   # (raises if a chain's status is not OK)


def _check_loss_sum(y, b, q):
    u = y[None, :] - b[:, None]
    return np.sum(u * (q - (u < 0)), axis=1)


def test_quantile_intercept_posterior_matches_quadrature():
    """p = 1, everything else integrated on a grid: the posterior of the intercept is
    proportional to exp(-2 sum_i rho_q(y_i - beta) - 0.005 beta^2).  1024 independent chains;
    the standard errors come from the spread of their means.  Bar fixed beforehand: 4 standard
    errors, for the mean and for the mass below the quadrature median."""
    n, q = 40, 0.25
    rng = np.random.default_rng(5)
    y = 1.0 + rng.standard_normal(n)
    X = np.ones((n, 1))
    grid = np.linspace(y.min() - 1.0, y.max() + 1.0, 20001)
    lp = -2.0 * _check_loss_sum(y, grid, q) - 0.005 * grid ** 2
    d = np.exp(lp - lp.max())
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (d[1:] + d[:-1]) * np.diff(grid))])
    gd = grid * d
    mean = float(np.sum(0.5 * (gd[1:] + gd[:-1]) * np.diff(grid))) / cdf[-1]
    cdf /= cdf[-1]
    median = float(np.interp(0.5, cdf, grid))
    chains, burn, keep = 1024, 100, 400
    eng = make_engine(chains, 21, X, y, q, np.zeros(1), 0.01 * np.eye(1), np.ones(1), np.ones(1, np.uint8))
    eng.quantile_sweep(burn)
    draws = np.zeros((keep, chains))
    for t in range(keep):
        eng.quantile_sweep(1)
        draws[t] = eng.get_states()[1][:, 0]
    cm = draws.mean(axis=0)
    se = cm.std(ddof=1) / np.sqrt(chains)
    below = (draws < median).mean(axis=0)
    se_b = below.std(ddof=1) / np.sqrt(chains)
    print("mean: device %.5f quadrature %.5f (se %.2g); mass below the median %.4f (se %.2g)"
          % (cm.mean(), mean, se, below.mean(), se_b))
    assert abs(cm.mean() - mean) < 4 * se, (cm.mean(), mean, se)
    assert abs(below.mean() - 0.5) < 4 * se_b, (below.mean(), se_b)


def _gibbs_numpy(X, y, q, prec_diag, pi, iters, seed):
    """a plain collapsed Gibbs sampler for the same posterior, own RNG: w | beta by
    Generator.wald, gamma_j | gamma_-j, w one at a time in a fresh random order (its own
    two-point draw from the marginal model probabilities, no enumeration), beta | gamma, w"""
    rng = np.random.default_rng(seed)
    n, p = X.shape
    shift = 1.0 - 2.0 * q
    lp1, lp0 = np.log(pi), np.log1p(-pi)
    gamma, beta = np.ones(p, bool), np.zeros(p)

    def logpost(g, A, b):
        idx = np.flatnonzero(g)
        lp = lp1[g].sum() + lp0[~g].sum()
        if idx.size == 0:
            return lp
        L = np.linalg.cholesky(A[np.ix_(idx, idx)] + np.diag(prec_diag[idx]))
        m = np.linalg.solve(L, b[idx])
        return lp + 0.5 * np.log(prec_diag[idx]).sum() - np.log(np.diag(L)).sum() + 0.5 * (m @ m)
    out = np.zeros((iters, 2 * p))
    for t in range(iters):
        r = np.abs(y - X @ beta)
        w = rng.wald(1.0 / r, 1.0)
        A = X.T @ (X * w[:, None])
        b = X.T @ (w * y - shift)
        cur = logpost(gamma, A, b)
        for j in rng.permutation(p):
            g2 = gamma.copy()
            g2[j] = not g2[j]
            new = logpost(g2, A, b)
            if np.log(rng.uniform()) < -np.logaddexp(0.0, cur - new):
                gamma, cur = g2, new
        idx = np.flatnonzero(gamma)
        beta = np.zeros(p)
        if idx.size:
            L = np.linalg.cholesky(A[np.ix_(idx, idx)] + np.diag(prec_diag[idx]))
            m = np.linalg.solve(L.T, np.linalg.solve(L, b[idx]))
            beta[idx] = m + np.linalg.solve(L.T, rng.standard_normal(idx.size))
        out[t, :p], out[t, p:] = gamma, beta
    return out


def test_quantile_posterior_matches_independent_gibbs():
    # the rule of test_student_posterior_matches_independent_gibbs, fixed before the first
    # run: |z| < 5 on every quantity (inclusion frequencies, then posterior means), the
    # device's standard error from its independent chains' means, the sampler's from batch
    # means.  A quantity both sides hold constant (an always-included signal) has no
    # standard error: there the two constants must be equal.
    n, p, q = 200, 6, 0.75
    X, y, _ = make_data(n, p, 2, 11)
    prec, pi = np.eye(p), np.full(p, 0.5)
    chains, burn, keep = 1024, 60, 140
    eng = make_engine(chains, 9, X, y, q, np.zeros(p), prec, pi, np.ones(p, np.uint8))
    eng.quantile_sweep(burn)
    draws = np.zeros((keep, chains, 2 * p))
    for t in range(keep):
        eng.quantile_sweep(1)
        g, b, _ = eng.get_states()
        draws[t, :, :p], draws[t, :, p:] = g, b
    cm = draws.mean(axis=0)
    dev_mean, dev_se = cm.mean(axis=0), cm.std(axis=0, ddof=1) / np.sqrt(chains)
    ref = _gibbs_numpy(X, y, q, np.diag(prec).copy(), pi, 8000, 2024)[1000:]
    nb = 50
    bm = ref[: len(ref) // nb * nb].reshape(nb, -1, 2 * p).mean(axis=1)
    ref_mean, ref_se = bm.mean(axis=0), bm.std(axis=0, ddof=1) / np.sqrt(nb)
    se = np.sqrt(dev_se ** 2 + ref_se ** 2)
    const = se == 0
    assert np.array_equal(dev_mean[const], ref_mean[const]), (dev_mean, ref_mean)
    z = (dev_mean[~const] - ref_mean[~const]) / se[~const]
    print("inclusion: device", np.round(dev_mean[:p], 4), "sampler", np.round(ref_mean[:p], 4), "\nz", np.round(z, 2))
    assert np.all(np.abs(z) < 5.0), (z, dev_mean, ref_mean)
    assert 0.01 < dev_mean[2:p].max() < 0.99      # (the case has inclusion draws that go both ways)


def test_quantile_fit_leaves_the_quantile_below():
    """q = 0.9: a fraction 0.9 of the responses lies below the fitted 0.9-quantile line x'beta-bar
    (within 3 binomial standard errors)"""
    n, p, q = 10000, 4, 0.9
    rng = np.random.default_rng(90)
    X = rng.standard_normal((n, p))
    X[:, 0] = 1.0
    y = X @ np.array([1.0, -1.0, 0.5, 0.0]) + rng.standard_normal(n)
    chains = 32
    eng = make_engine(chains, 6, X, y, q, np.zeros(p), 0.01 * np.eye(p), np.ones(p), np.ones(p, np.uint8))
    eng.quantile_sweep(60)
    eng.reset_summaries()
    eng.quantile_sweep(60)
    sm = eng.get_summaries()
    assert sm["sweeps"] == chains * 60
    bbar = sm["beta_sum"] / sm["sweeps"]
    frac = float(np.mean(y < X @ bbar))
    print("fraction below the fitted line: %.4f" % frac)
    assert abs(frac - q) < 3 * np.sqrt(q * (1 - q) / n), frac


def test_quantile_recorded_draws_equal_single_sweeps():
    n, p, q = 500, 16, 0.35
    X, y, _ = make_data(n, p, 4, 5)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.3)
    g0 = np.zeros(p, np.uint8)
    chains, seed, k = 8, 12, 9
    a = make_engine(chains, seed, X, y, q, mu, prec, pi, g0)
    a.enable_draws(k)
    a.quantile_sweep(k)
    b = make_engine(chains, seed, X, y, q, mu, prec, pi, g0)
    newX = np.random.default_rng(1).standard_normal((5, p))
    rows = []
    for s in range(k):
        b.quantile_sweep(1)
        rows.append(b.get_states())
    pred = a.predict(newX, 0, k)
    for c in (0, 3, chains - 1):
        g, bb, s2 = a.get_draws(c, k)
        for s in range(k):
            G, B, S = rows[s]
            assert np.array_equal(g[s], G[c]) and np.array_equal(bb[s], B[c])
            assert s2[s] == 1.0 and S[c] == 1.0
            assert np.allclose(pred[c, s], newX @ bb[s], rtol=1e-12, atol=1e-12)
    # the summaries count the sweeps since they were reset
    a.reset_summaries()
    a.quantile_sweep(k)
    sm = a.get_summaries()
    assert sm["sweeps"] == chains * k
    assert np.all(sm["inclusion_count"] <= chains * k)


def _install(eng, kind, X, y):
    n, p = X.shape
    binary = (y > 0).astype(float)
    if kind == "regression":
        eng.build_suf_from_xy(X, y)
    elif kind == "state_space":
        eng.ss_set_data(y[:50], X[:50])
    elif kind == "probit":
        eng.probit_set_data(X, binary, np.ones(n))
    elif kind == "logit":
        eng.logit_set_data(X, binary, np.ones(n))
    elif kind == "poisson":
        eng.poisson_set_data(X, np.ones(n), np.ones(n),
                             dict(counts=np.array([1]), ncomp=np.array([1]), mu=np.zeros(1),
                                  sigma=np.ones(1), weight=np.ones(1), largest_index=100))
    else:
        eng.student_set_data(X, y)


def test_quantile_refusals():
    import boom_amd
    n, p = 200, 5
    X, y, _ = make_data(n, p, 2, 1)
    mu, prec, pi = np.zeros(p), np.eye(p), np.full(p, 0.5)
    eng = boom_amd.Engine(4, seed=1)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.quantile_sweep(1)                                  # no data
    assert str(ei.value) == Q_FIRST
    for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
        with pytest.raises(boom_amd.BoomAmdError) as ei:
            eng.quantile_set_data(X, y, bad)
        assert "quantile" in str(ei.value)
    eng.quantile_set_data(X, y, 0.5)
    eng.set_spike(pi)
    # a slab whose precision scales with sigma^2 is not this sampler's
    eng.sss_set_slab(mu, prec, scales_with_sigsq=True)
    eng.set_state(np.zeros(p, np.uint8))
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.quantile_sweep(1)
    assert "fixed-precision slab" in str(ei.value)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=False)
    # sigma^2 is 1
    with pytest.raises(boom_amd.BoomAmdError):
        eng.set_state(np.zeros(p, np.uint8), sigsq=2.0)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.quantile_get_weights(0)                            # no imputation yet
    assert "ba_quantile_sweep" in str(ei.value)
    # every other sweep names this one
    for call in (eng.sweep, eng.sss_sweep, eng.adaptive_sweep, eng.probit_sweep, eng.logit_sweep,
                 eng.poisson_sweep, eng.student_sweep, eng.ss_sweep):
        with pytest.raises(boom_amd.BoomAmdError) as ei:
            call(1)
        assert str(ei.value) == USE_Q and ei.value.code == -9, call
    eng.quantile_sweep(2)
    assert np.all(np.isfinite(eng.quantile_get_weights(3)))
    # ... and this one asks for its data while the engine holds another kind
    for kind in ("regression", "probit", "logit", "poisson", "student", "state_space"):
        other = boom_amd.Engine(4, seed=1)
        _install(other, kind, X, y)
        with pytest.raises(boom_amd.BoomAmdError) as ei:
            other.quantile_sweep(1)
        assert str(ei.value) == Q_FIRST and ei.value.code == -9, kind
        with pytest.raises(boom_amd.BoomAmdError) as ei:
            other.quantile_get_weights(0)
        assert str(ei.value) == Q_FIRST, kind
        other.close()
    # new data of another kind on the same engine: its sweep runs again
    eng.student_set_data(X, y)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=True)
    eng.set_state(np.zeros(p, np.uint8))
    eng.student_sweep(1)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.quantile_sweep(1)
    assert str(ei.value) == Q_FIRST


def test_quantile_pybind_sampler_equals_the_engine():
    import boom_amd._boom as boom
    n, p, q = 400, 8, 0.3
    X, y, _ = make_data(n, p, 3, 8)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.4)
    chains, seed = 4, 41
    model = boom.QuantileRegressionModel(p, q, chains=chains, seed=seed)
    assert model.quantile == q and model.xdim == p
    model.set_data(X, y)
    sampler = boom.QuantileRegressionSpikeSlabSampler(model, boom.MvnModel(mu, prec, True),
                                                      boom.VariableSelectionPrior(pi))
    model.set_method(sampler)
    eng = make_engine(chains, seed, X, y, q, mu, prec, pi, np.ones(p, np.uint8))
    for _ in range(10):
        model.sample_posterior()
        eng.quantile_sweep(1)
        g, b, s = eng.get_state(0)
        assert np.array_equal(np.asarray(model.inc, dtype=np.uint8), g)
        assert np.array_equal(model.Beta, b)
    # limit_model_selection reaches the engine
    sampler.limit_model_selection(2)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=False, max_flips=2)
    for _ in range(5):
        sampler.draw()
        eng.quantile_sweep(1)
        g, b, s = eng.get_state(0)
        assert np.array_equal(np.asarray(model.inc, dtype=np.uint8), g) and np.array_equal(model.Beta, b)
    with pytest.raises(Exception):
        sampler.logpri()
