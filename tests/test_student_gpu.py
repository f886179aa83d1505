"""TRegressionSpikeSlabSampler on the device (ba_student_*): the weight imputation, the
sigma^2-conditional sweep on the weighted suf, sigma^2 and the slice-sampler draw of nu --
against the Python restatement of draw() on the same substreams (tests/student_oracle.py),
against a separately written Gibbs sampler, and on its behaviour.

Bars: inclusion indicators bit-exact, beta / sigma^2 / nu within 1e-8 relative, the slice
comparisons' recorded margin above 1e-9 (a rounding flip would show there first).
"""
import numpy as np
import pytest

from student_oracle import StudentOracle

pytestmark = pytest.mark.gpu
RTOL = 1e-8


def relerr(a, b, floor=1e-3):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def make_data(n, p, nsig, seed, df=3.0, outliers=0.0):
    from cases import student_data
    return student_data(n, p, nsig, seed, df=df, outliers=outliers)


def make_engine(chains, seed, X, y, mu, prec, pi, g0, nu_prior=(0, 0.1, 100.0), sigma_prior=(1.0, 1.0),
                sigma_max=np.inf, max_flips=-1):
    import boom_amd
    eng = boom_amd.Engine(chains, seed=seed)
    eng.student_set_data(X, y)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=True, max_flips=max_flips)
    eng.set_spike(pi)
    eng.set_sigma_prior(sigma_prior[0], sigma_prior[1], sigma_max)
    eng.student_set_nu_prior(*nu_prior)
    eng.set_state(g0)
    return eng


CASES = [
    # n, p, nsig, max_flips, sigma_max, nu_prior, slab mean
    (300, 10, 3, -1, np.inf, (0, 0.1, 100.0), 0.0),
    (800, 24, 5, 6, np.inf, (1, 2.0, 0.1), 0.0),
    (2000, 40, 6, -1, 1.2, (0, 0.1, 100.0), 0.0),
    (500, 70, 8, 12, np.inf, (1, 2.0, 0.1), 0.0),
    # a slab mean away from 0 (the Omega^{-1} mu / sigma^2 term) and a sigma upper limit far
    # below the posterior's scale (the truncated draw beyond the mode: adaptive rejection)
    (600, 16, 4, -1, 0.45, (0, 0.1, 100.0), 0.3),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_student_sweeps_match_restatement(oracle, case):
    n, p, nsig, mf, smax, nup, mu0 = CASES[case]
    X, y, _ = make_data(n, p, nsig, 100 + case)
    mu, prec = np.full(p, mu0), 0.1 * np.eye(p)
    pi = np.full(p, min(0.9, 5.0 / p))
    g0 = np.zeros(p, np.uint8)
    g0[:2] = 1
    chains, seed, nsw = 6, 31 + case, 25
    eng = make_engine(chains, seed, X, y, mu, prec, pi, g0, nu_prior=nup, sigma_max=smax, max_flips=mf)
    check = [0, chains - 1]
    ora = {c: StudentOracle(oracle, X, y, mu, prec, pi, seed, c, g0, nu_prior=nup, sigma_max=smax,
                            max_flips=mf) for c in check}
    for s in range(nsw):
        eng.student_sweep(1)
        gam, beta, sig = eng.get_states()
        nu = eng.student_get_nu()
        for c in check:
            g, b, s2, v = ora[c].draw()
            assert np.array_equal(gam[c], g), (c, s)
            assert relerr(beta[c], b) < RTOL, (c, s)
            assert relerr(sig[c], s2) < RTOL, (c, s)
            assert relerr(nu[c], v) < RTOL, (c, s)
            assert sig[c] <= smax ** 2
    margin = eng.student_get_margin()
    for c in check:
        assert margin[c] > 1e-9, (c, margin[c])
        assert abs(margin[c] - ora[c].margin) <= 1e-6 * max(ora[c].margin, 1e-12) + 1e-12
    # several sweeps in one call: the same draws
    eng2 = make_engine(chains, seed, X, y, mu, prec, pi, g0, nu_prior=nup, sigma_max=smax, max_flips=mf)
    eng2.student_sweep(nsw)
    a, b = eng.get_states(), eng2.get_states()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(eng.student_get_nu(), eng2.student_get_nu())


def test_student_without_model_selection_matches_restatement(oracle):
    """allow_model_selection(false): no inclusion draws (and no numbers read for them), the
    coefficients, sigma^2 and nu as before"""
    n, p = 500, 14
    X, y, _ = make_data(n, p, 4, 55)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.3)
    g0 = np.zeros(p, np.uint8)
    g0[[0, 2, 5]] = 1
    chains, seed = 4, 61
    eng = make_engine(chains, seed, X, y, mu, prec, pi, g0)
    eng.student_allow_model_selection(False)
    ora = {c: StudentOracle(oracle, X, y, mu, prec, pi, seed, c, g0, allow_selection=False)
           for c in (0, chains - 1)}
    for s in range(12):
        eng.student_sweep(1)
        gam, beta, sig = eng.get_states()
        nu = eng.student_get_nu()
        assert np.array_equal(gam, np.tile(g0, (chains, 1)))
        for c, o in ora.items():
            g, b, s2, v = o.draw()
            assert np.array_equal(gam[c], g)
            assert relerr(beta[c], b) < RTOL and relerr(sig[c], s2) < RTOL and relerr(nu[c], v) < RTOL, (c, s)
    eng.student_allow_model_selection(True)
    eng.student_sweep(20)
    assert not np.array_equal(eng.get_states()[0], np.tile(g0, (chains, 1)))


def test_student_large_model_escalates(oracle):
    """a model of more than 64 variables: the chains move to the large-model kernel"""
    n, p = 600, 72
    X, y, _ = make_data(n, p, 70, 7)
    mu, prec = np.zeros(p), 0.1 * np.eye(p)
    pi = np.full(p, 0.97)
    g0 = np.ones(p, np.uint8)
    chains, seed = 4, 5
    eng = make_engine(chains, seed, X, y, mu, prec, pi, g0)
    ora = {c: StudentOracle(oracle, X, y, mu, prec, pi, seed, c, g0) for c in (0, chains - 1)}
    for s in range(8):
        eng.student_sweep(1)
        gam, beta, sig = eng.get_states()
        nu = eng.student_get_nu()
        for c, o in ora.items():
            g, b, s2, v = o.draw()
            assert g.sum() > 64
            assert np.array_equal(gam[c], g), (c, s)
            assert relerr(beta[c], b) < RTOL and relerr(sig[c], s2) < RTOL and relerr(nu[c], v) < RTOL, (c, s)


@pytest.mark.parametrize("nu", [0.15, 0.6, 0.999, 1.0, 1.001, 4.5, 99.9])
def test_student_weights_match_the_imputation(oracle, nu):
    """the weights' shape (nu + 1) / 2 on both sides of 1: below it the gamma draw takes
    its GS branch (nu < 1), at 1 and above the normal-based one"""
    n, p = 700, 12
    X, y, _ = make_data(n, p, 3, 3)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.3)
    g0 = np.zeros(p, np.uint8)
    g0[:3] = 1
    beta0 = np.linspace(0.5, 1.5, p)
    chains, seed = 3, 77
    eng = make_engine(chains, seed, X, y, mu, prec, pi, g0)
    eng.set_state(g0, beta0, sigsq=1.7)
    eng.student_set_nu(nu)
    eng.student_sweep(1)
    for c in range(chains):
        o = StudentOracle(oracle, X, y, mu, prec, pi, seed, c, g0, beta0=beta0, sigsq0=1.7, nu0=nu)
        w = o.impute()
        assert relerr(eng.student_get_weights(c), w, floor=1e-300) < 1e-12


def check_parity(eng, ora, nsweeps, each=None):
    """nsweeps single sweeps of the engine against the restatements ora (chain -> StudentOracle)
    at the file's bars; each(s, gamma, beta, sigsq, nu) sees the engine's state after sweep s.
    Returns the checked chains' nu draws."""
    nus = {c: [] for c in ora}
    for s in range(nsweeps):
        eng.student_sweep(1)
        gam, beta, sig = eng.get_states()
        nu = eng.student_get_nu()
        if each is not None:
            each(s, gam, beta, sig, nu)
        for c, o in ora.items():
            g, b, s2, v = o.draw()
            assert np.array_equal(gam[c], g), (c, s)
            assert relerr(beta[c], b) < RTOL, (c, s)
            assert relerr(sig[c], s2) < RTOL, (c, s)
            assert relerr(nu[c], v) < RTOL, (c, s)
            nus[c].append(nu[c])
    margin = eng.student_get_margin()
    for c, o in ora.items():
        assert margin[c] > 1e-9, (c, margin[c])
        assert abs(margin[c] - o.margin) <= 1e-6 * max(o.margin, 1e-12) + 1e-12
    return nus


def test_student_more_than_256_variables(oracle):
    """p = 520: the included-variable compaction runs in three chunks of 256 (a ballot and a
    prefix sum carried by base), with included variables on both sides of 256 and 512"""
    n, p = 600, 520
    rng = np.random.default_rng(520)
    X = rng.standard_normal((n, p))
    X[:, 0] = 1.0
    sig_idx = [0, 3, 255, 256, 300, 511, 512, 519]
    beta = np.zeros(p)
    beta[sig_idx] = [1.0, -1.5, 1.5, -1.0, 2.0, -2.0, 1.0, 1.5]
    y = X @ beta + 0.8 * rng.standard_t(3.0, n)
    mu, prec = np.zeros(p), 0.1 * np.eye(p)
    pi = np.full(p, 0.01)
    pi[sig_idx] = 0.9
    g0 = np.zeros(p, np.uint8)
    g0[sig_idx] = 1
    chains, seed = 2, 52
    eng = make_engine(chains, seed, X, y, mu, prec, pi, g0)
    ora = {c: StudentOracle(oracle, X, y, mu, prec, pi, seed, c, g0) for c in range(chains)}

    def straddles(s, gam, beta, sig, nu):
        for c in range(chains):
            inc = np.flatnonzero(gam[c])
            assert inc.min() < 256 and np.any((inc >= 256) & (inc < 512)) and inc.max() >= 512, (c, s)
    check_parity(eng, ora, 5, straddles)


@pytest.mark.parametrize("n", [37, 256, 257])
def test_student_small_n_and_block_edges(oracle, n):
    """n below one impute block (idle lanes in every per-chain reduction), exactly one block,
    and one past it"""
    p = 6
    X, y, _ = make_data(n, p, 2, 400 + n)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.5)
    g0 = np.zeros(p, np.uint8)
    g0[:2] = 1
    chains, seed = 6, 60 + n
    eng = make_engine(chains, seed, X, y, mu, prec, pi, g0)
    ora = {c: StudentOracle(oracle, X, y, mu, prec, pi, seed, c, g0) for c in (0, chains - 1)}
    check_parity(eng, ora, 15)


# the prior-edge cases of tests/golden/make_golden_student.py, on the device's substreams:
# data (n, p, nsig, seed, error df), starting nu
PRIOR_EDGES = {
    "heavy_tails": ((300, 8, 3, 106, 0.7), 2.0),     # nu below 1
    "gaussian": ((400, 8, 3, 107, np.inf), 60.0),    # nu against Uniform(0.1, 100)'s bound
}


@pytest.mark.parametrize("name", sorted(PRIOR_EDGES))
def test_student_prior_edges(oracle, name):
    from cases import student_data
    (n, p, nsig, dseed, df), nu0 = PRIOR_EDGES[name]
    X, y, _ = student_data(n, p, nsig, dseed, df=df)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 5.0 / p)
    g0 = np.zeros(p, np.uint8)
    g0[:2] = 1
    chains, seed = 4, 41
    eng = make_engine(chains, seed, X, y, mu, prec, pi, g0)
    eng.student_set_nu(nu0)
    ora = {c: StudentOracle(oracle, X, y, mu, prec, pi, seed, c, g0, nu0=nu0) for c in (0, chains - 1)}
    nus = check_parity(eng, ora, 60)
    for c, v in nus.items():
        if name == "heavy_tails":
            assert min(v) < 1.0, (c, min(v))
        else:
            assert max(v) > 90.0, (c, max(v))


def test_student_many_chains(oracle):
    """1024 chains, draw for draw at the first, a middle and the last (high blockIdx.y in the
    impute grid, late workgroups of the sigma^2 / nu kernel)"""
    n, p = 300, 10
    X, y, _ = make_data(n, p, 3, 1024)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.5)
    g0 = np.zeros(p, np.uint8)
    g0[:2] = 1
    chains, seed = 1024, 88
    eng = make_engine(chains, seed, X, y, mu, prec, pi, g0)
    ora = {c: StudentOracle(oracle, X, y, mu, prec, pi, seed, c, g0) for c in (0, 511, 1023)}
    check_parity(eng, ora, 10)


def test_student_wsse_at_a_large_offset(oracle, capsys):
    """y = 1e4 + t_3 noise with an intercept: y'Wy is ~1e8 times the weighted sum of squared
    errors.  The device sums w_i r_i^2 directly; the reference's suf form
    beta'X'WX beta - 2 beta'X'Wy + y'Wy loses about log10(y'Wy / wsse) digits there.  Without a
    sigma limit sigma^2 is proportional to SS, so holding the device's sigma^2 to 1e-10 of the
    restatement's exactly summed form (wsse="exact") measures the sum alone."""
    from cases import student_data
    n, p = 400, 6
    X, y, _ = student_data(n, p, 3, 9, offset=1e4)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.5)
    mu[0], pi[0] = 1e4, 1.0
    g0 = np.zeros(p, np.uint8)
    g0[:2] = 1
    beta0 = np.zeros(p)
    beta0[0] = 1e4
    chains, seed, nsw, bar = 4, 43, 12, 1e-10
    eng = make_engine(chains, seed, X, y, mu, prec, pi, g0)
    eng.set_state(g0, beta0)
    ora = {c: StudentOracle(oracle, X, y, mu, prec, pi, seed, c, g0, beta0=beta0, wsse="exact")
           for c in (0, chains - 1)}
    eps = np.finfo(float).eps
    suf_err, dev_err = [], []
    for s in range(nsw):
        eng.student_sweep(1)
        gam, beta, sig = eng.get_states()
        nu = eng.student_get_nu()
        for c, o in ora.items():
            g, b, s2, v = o.draw()
            assert np.array_equal(gam[c], g), (c, s)
            assert relerr(beta[c], b) < RTOL and relerr(nu[c], v) < RTOL, (c, s)
            dev_err.append(abs(sig[c] - s2) / s2)
            assert dev_err[-1] <= bar, (c, s, dev_err[-1])
            ss = o.suf["wsse_exact"] + o.prior_ss
            # the case still discriminates: the suf form's expected error is 100 x the bar
            assert eps * o.suf["yty"] / ss >= 100 * bar, (c, s)
            suf_err.append(abs(o.suf["wsse_suf"] + o.prior_ss - ss) / ss)
    # ... and its measured error is too
    assert max(suf_err) >= 100 * bar, max(suf_err)
    with capsys.disabled():
        print("\nlarge offset: sigma^2 relative error, device %.2e (max); suf form %.2e max, %.2e median"
              % (max(dev_err), max(suf_err), float(np.median(suf_err))))


def _gibbs_numpy(X, y, prec, prior_df, guess, nu_prior, iters, seed):
    """a plain Gibbs sampler for the full Student-t regression (no selection), own RNG:
    w | . gamma, beta | . normal, sigma^2 | . inverse gamma, nu | . random-walk Metropolis on
    log nu (prior Uniform(a, b))"""
    from scipy.special import gammaln
    rng = np.random.default_rng(seed)
    n, p = X.shape
    beta, sigsq, nu = np.zeros(p), 1.0, 30.0
    a, b = nu_prior

    def lpost(v, u):
        if v < a or v > b:
            return -np.inf
        return n * (gammaln((v + 1) / 2) - gammaln(v / 2) - 0.5 * np.log(v * np.pi)) \
            - 0.5 * (v + 1) * np.sum(np.log1p(u / v)) + np.log(v)   # (+ log v: the log-scale walk's Jacobian)
    out = np.zeros((iters, p + 2))
    for t in range(iters):
        r = y - X @ beta
        w = rng.gamma(0.5 * (nu + 1), 1.0 / (0.5 * (nu + r * r / sigsq)))
        Xw = X * w[:, None]
        P = (prec + X.T @ Xw) / sigsq
        L = np.linalg.cholesky(P)
        m = np.linalg.solve(P, (Xw.T @ y) / sigsq)
        beta = m + np.linalg.solve(L.T, rng.standard_normal(p))
        r = y - X @ beta
        ss = np.sum(w * r * r) + prior_df * guess ** 2
        sigsq = 1.0 / rng.gamma(0.5 * (n + prior_df), 1.0 / (0.5 * ss))
        u = r * r / sigsq
        for _ in range(3):
            prop = nu * np.exp(0.3 * rng.standard_normal())
            if np.log(rng.uniform()) < lpost(prop, u) - lpost(nu, u):
                nu = prop
        out[t, :p], out[t, p], out[t, p + 1] = beta, sigsq, nu
    return out


def test_student_posterior_matches_independent_gibbs():
    # (threshold fixed before the first run: |z| < 5 on every quantity)
    n, p = 400, 3
    X, y, _ = make_data(n, p, 3, 11, df=3.0)
    prec = 0.01 * np.eye(p)
    chains, burn, keep = 1024, 60, 140
    eng = make_engine(chains, 9, X, y, np.zeros(p), prec, np.ones(p), np.ones(p, np.uint8))
    eng.student_sweep(burn)
    draws = np.zeros((keep, chains, p + 2))
    for t in range(keep):
        eng.student_sweep(1)
        g, b, s = eng.get_states()
        draws[t, :, :p], draws[t, :, p], draws[t, :, p + 1] = b, s, eng.student_get_nu()
    cm = draws.mean(axis=0)                     # chain means: independent across chains
    dev_mean, dev_se = cm.mean(axis=0), cm.std(axis=0, ddof=1) / np.sqrt(chains)
    ref = _gibbs_numpy(X, y, prec, 1.0, 1.0, (0.1, 100.0), 30000, 2024)[2000:]
    nb = 50
    bm = ref[: len(ref) // nb * nb].reshape(nb, -1, p + 2).mean(axis=1)
    ref_mean, ref_se = bm.mean(axis=0), bm.std(axis=0, ddof=1) / np.sqrt(nb)
    z = (dev_mean - ref_mean) / np.sqrt(dev_se ** 2 + ref_se ** 2)
    assert np.all(np.abs(z) < 5.0), (z, dev_mean, ref_mean)


def test_student_is_robust_to_outliers_and_learns_the_tails():
    import boom_amd
    n, p = 600, 6
    X, y, truth = make_data(n, p, 4, 21, df=np.inf, outliers=0.05)
    mu, prec, pi = np.zeros(p), 0.01 * np.eye(p), np.ones(p)
    g1 = np.ones(p, np.uint8)
    chains = 256
    eng = make_engine(chains, 3, X, y, mu, prec, pi, g1)
    eng.student_sweep(100)
    bs, nus = [], []
    for _ in range(100):
        eng.student_sweep(1)
        bs.append(eng.get_states()[1])
        nus.append(eng.student_get_nu())
    b_t, nu_t = np.mean(bs, axis=(0, 1)), np.mean(nus)
    gau = boom_amd.Engine(chains, seed=3)
    gau.build_suf_from_xy(X, y)
    gau.sss_set_slab(mu, prec, scales_with_sigsq=True)
    gau.set_spike(pi)
    gau.set_state(g1, sigsq=0.64)
    gau.sss_sweep(100)
    gb = []
    for _ in range(100):
        gau.sss_sweep(1)
        gb.append(gau.get_states()[1])
    b_g = np.mean(gb, axis=(0, 1))
    assert np.linalg.norm(b_t - truth) < np.linalg.norm(b_g - truth)
    assert nu_t < 10
    # Gaussian data: nu goes to the upper half of Uniform(0.1, 100)
    X2, y2, _ = make_data(n, p, 4, 22, df=np.inf)
    eng2 = make_engine(chains, 4, X2, y2, mu, prec, pi, g1)
    eng2.student_sweep(150)
    nu2 = []
    for _ in range(50):
        eng2.student_sweep(1)
        nu2.append(eng2.student_get_nu())
    assert np.mean(nu2) > 50.05


def test_student_recorded_draws_equal_single_sweeps():
    n, p = 500, 16
    X, y, _ = make_data(n, p, 4, 5)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.3)
    g0 = np.zeros(p, np.uint8)
    chains, seed, k = 8, 12, 9
    a = make_engine(chains, seed, X, y, mu, prec, pi, g0)
    a.enable_draws(k)
    a.student_sweep(k)
    b = make_engine(chains, seed, X, y, mu, prec, pi, g0)
    newX = np.random.default_rng(1).standard_normal((5, p))
    rows = []
    for s in range(k):
        b.student_sweep(1)
        rows.append((b.get_states(), b.student_get_nu()))
    pred = a.predict(newX, 0, k)
    # the summaries' sigma^2 moments are those of the recorded draws
    a2 = make_engine(chains, seed, X, y, mu, prec, pi, g0)
    a2.enable_draws(k)
    a2.student_sweep(3)
    a2.reset_summaries()
    a2.student_sweep(k)
    sm = a2.get_summaries()
    s2 = np.array([a2.get_draws(c, k)[2] for c in range(chains)])
    assert sm["sweeps"] == chains * k
    assert abs(sm["sigsq_sum"] - s2.sum()) <= 1e-12 * s2.sum()
    assert abs(sm["sigsq_sumsq"] - (s2 ** 2).sum()) <= 1e-12 * (s2 ** 2).sum()
    for c in (0, 3, chains - 1):
        g, bb, s2 = a.get_draws(c, k)
        nu = a.student_get_nu_draws(c, k)
        for s in range(k):
            (G, B, S), N = rows[s]
            assert np.array_equal(g[s], G[c]) and np.array_equal(bb[s], B[c])
            assert s2[s] == S[c] and nu[s] == N[c]
            assert np.allclose(pred[c, s], newX @ bb[s], rtol=1e-12, atol=1e-12)


def test_student_refusals():
    import boom_amd
    n, p = 200, 5
    X, y, _ = make_data(n, p, 2, 1)
    mu, prec, pi = np.zeros(p), np.eye(p), np.full(p, 0.5)
    eng = boom_amd.Engine(4, seed=1)
    with pytest.raises(boom_amd.BoomAmdError):
        eng.student_sweep(1)                               # no data
    for bad in ((0, 5.0, 1.0), (0, -1.0, 3.0), (1, 0.0, 1.0), (1, 2.0, -1.0), (2, 1.0, 2.0)):
        with pytest.raises(boom_amd.BoomAmdError):
            eng.student_set_nu_prior(*bad)
    eng.student_set_data(X, y)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=True)
    eng.set_spike(pi)
    eng.set_state(np.zeros(p, np.uint8))
    for nu in (0.0, -2.0, np.inf):
        with pytest.raises(boom_amd.BoomAmdError):
            eng.student_set_nu(nu)
    for call in (eng.sweep, eng.sss_sweep, eng.adaptive_sweep, eng.logit_sweep, eng.probit_sweep,
                 eng.poisson_sweep):
        with pytest.raises(boom_amd.BoomAmdError) as ei:
            call(1)
        assert "ba_student_sweep" in str(ei.value)
    eng.student_sweep(2)
    assert eng.student_get_nu(0) > 0 and np.all(eng.student_get_nu() != 30.0)
    # new data: a new model, nu back at 30, no slice margin yet
    eng.student_set_data(X, y)
    assert np.all(eng.student_get_nu() == 30.0) and np.all(np.isinf(eng.student_get_margin()))
    eng.set_state(np.zeros(p, np.uint8))
    # a fixed-precision slab is not this sampler's
    eng.sss_set_slab(mu, prec, scales_with_sigsq=False)
    with pytest.raises(boom_amd.BoomAmdError):
        eng.student_sweep(1)
    # the other families' modes refuse ba_student_sweep
    lg = boom_amd.Engine(4, seed=1)
    lg.logit_set_data(X, (y > 0).astype(float), np.ones(n))
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        lg.student_sweep(1)
    assert "ba_logit_sweep" in str(ei.value)
    pr = boom_amd.Engine(4, seed=1)
    pr.probit_set_data(X, (y > 0).astype(float), np.ones(n))
    with pytest.raises(boom_amd.BoomAmdError):
        pr.student_sweep(1)
    po = boom_amd.Engine(4, seed=1)
    po.poisson_set_data(X, np.ones(n), np.ones(n), dict(counts=np.array([1]), ncomp=np.array([1]),
                                                          mu=np.zeros(1), sigma=np.ones(1),
                                                          weight=np.ones(1), largest_index=100))
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        po.student_sweep(1)
    assert "ba_poisson_sweep" in str(ei.value)
    ss = boom_amd.Engine(4, seed=1)
    ss.ss_set_data(y[:50], X[:50])
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        ss.student_sweep(1)
    assert "ba_ss_sweep" in str(ei.value)
    # nu outside the Uniform prior's support: the slice sampler's error exit, reported
    eng.sss_set_slab(mu, prec, scales_with_sigsq=True)
    eng.student_set_nu_prior(0, 0.1, 100.0)
    eng.student_set_nu(150.0, chain=1)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.student_sweep(1)
    assert "slice sampler" in str(ei.value)


def test_student_pybind_sampler_equals_the_engine():
    import boom_amd._boom as boom
    n, p = 400, 8
    X, y, _ = make_data(n, p, 3, 8)
    mu, prec, pi = np.zeros(p), 0.1 * np.eye(p), np.full(p, 0.4)
    chains, seed = 4, 41
    model = boom.TRegressionModel(X, y, chains=chains, seed=seed)
    sampler = boom.TRegressionSpikeSlabSampler(model, boom.MvnGivenScalarSigma(mu, prec),
                                               boom.VariableSelectionPrior(pi), boom.ChisqModel(1.0, 1.0),
                                               boom.UniformModel(0.1, 100.0))
    model.set_method(sampler)
    eng = make_engine(chains, seed, X, y, mu, prec, pi, np.ones(p, np.uint8))
    for _ in range(10):
        model.sample_posterior()
        eng.student_sweep(1)
        g, b, s = eng.get_state(0)
        assert np.array_equal(np.asarray(model.inc, dtype=np.uint8), g)
        assert np.array_equal(model.Beta, b)
        assert model.sigsq == s and model.nu == eng.student_get_nu(0)
    # allow_model_selection(false): the model stays where it is, the other draws go on
    inc0 = list(model.inc)
    sampler.allow_model_selection(False)
    eng.student_allow_model_selection(False)
    for _ in range(5):
        model.sample_posterior()
        eng.student_sweep(1)
        assert list(model.inc) == inc0
        g, b, s = eng.get_state(0)
        assert np.array_equal(model.Beta, b) and model.sigsq == s and model.nu == eng.student_get_nu(0)
