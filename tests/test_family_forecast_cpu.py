"""The restatement of the observation families' forecasts (tests/family_forecast_ref.py), without a GPU:

  (a) with a Gaussian observation line it IS oracle.ssg_forecast, bit for bit, over two calls on one
      stream: the state advance the families share is pinned on what the reference goldens pin
  (b) rstudent is the reference's two calls at the same stream positions
  (c) rpois and rbinom against the exact pmf: 200 000 draws a point, chi-square over bins pooled to an
      expected count of at least 20, p-value >= 1e-4 at every point
  (d) the margin rule: at most 1 draw in 10 000 is "close"
  (e) the edge cases, which read no stream position
"""
import math

import numpy as np
import pytest
from scipy import stats

import family_forecast_ref as ffr
from cases import general_spec

SEED = 20261019
NDRAWS = 200_000
POISSON_POINTS = [0.001, 0.5, 3.0, 9.999, 10.0, 10.5, 37.0, 1e3, 1e6]
BINOMIAL_POINTS = [(1, .3), (5, .5), (40, .2), (40, .26), (100, .1), (100, .5), (1000, .37), (10 ** 5, .01),
                   (10 ** 5, .5), (40, .8), (1000, .63)]


# ---- (a) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc", [
    [("level",)],
    [("trend",), ("seasonal", 4, 1)],
    [("intercept",), ("seasonal", 4, 3, 2)],     # seasons of three steps: most steps draw no seasonal error
])
def test_gaussian_branch_is_the_oracles_forecast(oracle, desc):
    T, p, h, seed, chain = 37, 3, 9, 515, 4
    rs = np.random.Generator(np.random.PCG64(100 + 10 * len(desc) + len(desc[-1])))
    blocks = general_spec(rs.standard_normal(T), desc)
    m = sum(b["dim"] for b in blocks)
    sigsq = np.zeros((len(blocks), 2))
    for b, blk in enumerate(blocks):
        nv = len(blk["df"])
        sigsq[b, :nv] = rs.uniform(0.05, 0.6, nv)
    beta, final = rs.standard_normal(p), rs.standard_normal(m)
    phi = np.zeros((len(blocks), 16))
    rng = oracle.rng_philox(seed, chain, 5)
    s = ffr.Stream(oracle, seed, chain)
    for call in range(2):
        newX = rs.standard_normal((h, p))
        want = oracle.ssg_forecast(rng, T, newX, beta, 0.37, blocks, sigsq, phi, final)
        got = ffr.forecast(s, "gaussian", T, newX, beta, blocks, sigsq, final, sigsq_obs=0.37)
        assert np.array_equal(got, want), (desc, call)
        assert s.pos == int(rng.pos) > 0


# ---- (b) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", [0.7, 3.0, 60.0])
def test_rstudent_is_rgamma_then_rnorm(oracle, nu):
    mu, sigma = 1.25, 0.8
    a, b = ffr.Stream(oracle, SEED, 1), ffr.Stream(oracle, SEED, 1)
    for _ in range(200):
        got = ffr.rstudent(a, mu, sigma, nu)
        w = b.rgamma(nu / 2.0, nu / 2.0)
        z = b.norm_rand()
        assert got == mu + sigma / math.sqrt(w) * z
        assert a.pos == b.pos


# ---- (c), (d) ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def count_draws(oracle):
    """every point's draws, made once: point -> (values, number of close draws, branches seen)"""
    out = {}
    points = [("poisson", lam) for lam in POISSON_POINTS] + [("binomial", nq) for nq in BINOMIAL_POINTS]
    for chain, (kind, arg) in enumerate(points):
        s = ffr.Stream(oracle, SEED, chain)
        values, close, branches = np.zeros(NDRAWS), 0, set()
        for i in range(NDRAWS):
            d = ffr.rpois(s, arg) if kind == "poisson" else ffr.rbinom(s, arg[0], arg[1])
            values[i] = d.value
            close += d.close
            branches.add(d.branch)
        out[(kind, arg)] = (values, close, branches)
    return out


def pooled_chisq_pvalue(values, dist):
    """chi-square of the draws against the exact pmf, neighbouring values pooled from the left until a
    bin's expected count reaches 20 (the remainder joins the last bin); both tails belong to the end bins"""
    n = len(values)
    lo, hi = int(dist.ppf(1e-13)), int(dist.ppf(1.0 - 1e-13)) + 1
    ks = np.arange(lo, hi + 1)
    expect = n * dist.pmf(ks)
    expect[0] += n * dist.cdf(lo - 1)
    expect[-1] += n * dist.sf(hi)
    assert abs(expect.sum() - n) < 1e-6 * n
    seen = np.bincount(np.clip(values, lo, hi).astype(np.int64) - lo, minlength=len(ks)).astype(float)
    e_bins, o_bins, e, o = [], [], 0.0, 0.0
    for ei, oi in zip(expect, seen):
        e += ei
        o += oi
        if e >= 20.0:
            e_bins.append(e)
            o_bins.append(o)
            e, o = 0.0, 0.0
    if e_bins:
        e_bins[-1] += e
        o_bins[-1] += o
    else:
        e_bins, o_bins = [e], [o]
    e_bins, o_bins = np.array(e_bins), np.array(o_bins)
    if len(e_bins) < 2:
        return 1.0, 0
    chi2 = float(((o_bins - e_bins) ** 2 / e_bins).sum())
    return float(stats.chi2.sf(chi2, len(e_bins) - 1)), len(e_bins)


@pytest.mark.parametrize("lam", POISSON_POINTS)
def test_rpois_has_the_poisson_pmf(count_draws, lam):
    values, _, branches = count_draws[("poisson", lam)]
    assert np.all(values == np.floor(values)) and values.min() >= 0
    assert branches == ({"inversion"} if lam < 10.0 else {"ptrs"})
    pv, bins = pooled_chisq_pvalue(values, stats.poisson(lam))
    print("Poisson(%g): %d bins, p-value %.4f" % (lam, bins, pv))
    assert bins >= 2 and pv >= 1e-4


@pytest.mark.parametrize("n,p", BINOMIAL_POINTS)
def test_rbinom_has_the_binomial_pmf(count_draws, n, p):
    values, _, branches = count_draws[("binomial", (n, p))]
    assert np.all(values == np.floor(values)) and values.min() >= 0 and values.max() <= n
    want = ("inversion" if n * min(p, 1.0 - p) < 10.0 else "btrs") + ("+mirror" if p > 0.5 else "")
    assert branches == {want}
    pv, bins = pooled_chisq_pvalue(values, stats.binom(n, p))
    print("Binomial(%d, %g): %d bins, p-value %.4f" % (n, p, bins, pv))
    assert bins >= 2 and pv >= 1e-4


def test_close_draws_are_rare(count_draws):
    total = sum(len(v) for v, _, _ in count_draws.values())
    close = sum(c for _, c, _ in count_draws.values())
    for key, (_, c, _) in count_draws.items():
        if c:
            print("close draws at", key, ":", c)
    print("close draws: %d of %d (%.2e)" % (close, total, close / total))
    assert total == NDRAWS * (len(POISSON_POINTS) + len(BINOMIAL_POINTS))
    assert close <= total / 10_000


# ---- (e) ---------------------------------------------------------------------------------------------
def test_edge_cases_read_no_stream_position(oracle):
    s = ffr.Stream(oracle, SEED, 99)
    nan, inf = math.nan, math.inf
    for d, want in ((ffr.rpois(s, 0.0), 0.0), (ffr.rbinom(s, 0, 0.4), 0.0), (ffr.rbinom(s, 17, 0.0), 0.0),
                    (ffr.rbinom(s, 17, 1.0), 17.0), (ffr.rbinom(s, 10 ** 8, 1.0), 1e8)):
        assert d.value == want and d.margin == inf and not d.close
    for d in (ffr.rpois(s, nan), ffr.rpois(s, inf), ffr.rpois(s, -1.0), ffr.rbinom(s, 5, nan), ffr.rbinom(s, nan, 0.5),
              ffr.rbinom(s, 5, 1.5), ffr.rbinom(s, 5, -0.1), ffr.rbinom(s, inf, 0.5)):
        assert math.isnan(d.value)
    assert s.pos == 0
    # one uniform for an inversion, pairs for a transformed rejection
    ffr.rpois(s, 2.0)
    assert s.pos == 1
    ffr.rbinom(s, 8, 0.9)
    assert s.pos == 2
    ffr.rpois(s, 50.0)
    assert s.pos >= 4 and s.pos % 2 == 0
    # plogis saturates exactly, and a saturated probability reads nothing
    assert ffr.plogis(800.0) == 1.0 and ffr.plogis(-800.0) == 0.0 and math.isnan(ffr.plogis(nan))
    assert ffr.plogis(0.0) == 0.5
    before = s.pos
    assert ffr.rbinom(s, 30, ffr.plogis(-800.0)).value == 0.0 and ffr.rbinom(s, 30, ffr.plogis(800.0)).value == 30.0
    assert s.pos == before
