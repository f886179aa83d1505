"""The restatement of the hierarchical regression holiday's sampler (tests/ss_hier_regholiday_oracle.py) pinned
on things that do not depend on it, and the host arithmetic (tests/cpp/ssg_hier_regholiday_check.cpp, built
with the address and undefined-behaviour sanitizers by `make -C tests/cpp -f hier_regholiday.mk` and run as a
program).  No GPU, and the library is not loaded.

oracle/ cannot grow a driver for HierGaussianRegressionAsisSampler, so the restatement is pinned by these
checks and by reading, not by a compiled run."""
import os
import subprocess

import numpy as np
import pytest

import ss_hier_regholiday_cases as hrc
import ss_hier_regholiday_oracle as hro

HERE = os.path.dirname(os.path.abspath(__file__))


def zero():
    return 0.0


def test_host_arithmetic_check_runs_clean():
    exe = os.path.join(HERE, "cpp", "build", "ssg_hier_regholiday_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-f", "hier_regholiday.mk", "build/ssg_hier_regholiday_check"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failures" in out.stdout, out.stdout


@pytest.mark.parametrize("dt", [np.float64, np.longdouble])
def test_step_1_without_noise_is_the_augmented_regression(dt):
    """normals = 0: beta_h = (D'D / sigma^2 + Omega)^-1 (D'r / sigma^2 + Omega mu) for holiday h's dummies D (a row
    per observed active day, a 1 in the day's column) and responses r, by a dense solve of rows built the long
    way; within 1e-12"""
    rs = np.random.Generator(np.random.PCG64(2))
    H, d, sigsq = 4, 3, 0.8
    model = hro.hier_model(H, d, (rs.standard_normal(d), hrc.spd(rs, d)), (hrc.spd(rs, d), 5.0), None)
    mu, omega = rs.standard_normal(d), hrc.spd(rs, d)
    days = [rs.integers(0, d, size=rs.integers(2, 9)) for _ in range(H)]
    resp = [rs.standard_normal(len(x)) for x in days]
    counts = np.array([[np.sum(x == j) for j in range(d)] for x in days], dtype=np.float64)
    totals = np.array([[np.sum(r[x == j]) for j in range(d)] for x, r in zip(days, resp)])
    out = hro.draw(model, sigsq, totals, counts, mu, omega, zero, lambda a, s: a * s, dt)
    for h in range(H):
        D = np.zeros((len(days[h]), d))
        D[np.arange(len(days[h])), days[h]] = 1.0
        want = np.linalg.solve(D.T @ D / sigsq + omega, D.T @ resp[h] / sigsq + omega @ mu)
        assert np.max(np.abs(out["beta"][h].astype(np.float64) - want)) < 1e-12, h


@pytest.mark.parametrize("dt", [np.float64, np.longdouble])
def test_rwish_without_noise_is_c_diag_c(dt):
    """normals = 0 and rchisq(df) = df (rgamma(shape, scale) = shape x scale): the triangle is
    diag(sqrt(nu - i)), so rWish returns C diag(nu - i) C' with C the lower factor of V"""
    rs = np.random.Generator(np.random.PCG64(3))
    d, nu = 4, 7.5
    V = hrc.spd(rs, d)
    got = hro.rwish(nu, V.astype(dt), zero, lambda a, s: a * s, dt).astype(np.float64)
    Cf = np.linalg.cholesky(V)
    want = Cf @ np.diag(nu - np.arange(d)) @ Cf.T
    assert np.max(np.abs(got - want)) < 1e-12 * np.abs(want).max()


def test_bartlett_consumption_order():
    """d = 3: the calls in the reference's order, by hand"""
    calls = []

    def rnorm():
        calls.append(("rnorm",))
        return float(len(calls))

    def rgamma(shape, scale):
        calls.append(("rgamma", shape, scale))
        return float(len(calls)) ** 2

    T = hro.bartlett(3, 6.5, rnorm, rgamma)
    assert calls == [("rgamma", 3.25, 2.0),
                     ("rgamma", 2.75, 2.0), ("rnorm",),
                     ("rgamma", 2.25, 2.0), ("rnorm",), ("rnorm",)]
    assert np.array_equal(T, [[1.0, 0.0, 0.0], [3.0, 2.0, 0.0], [5.0, 6.0, 4.0]])


def test_a_holiday_never_observed_draws_from_the_prior():
    """counts 0 on every day: beta_h = mu + L'^-1 z with L L' = Omega"""
    rs = np.random.Generator(np.random.PCG64(4))
    H, d = 2, 3
    model = hro.hier_model(H, d, (np.zeros(d), np.eye(d)), (np.eye(d), 5.0), None)
    mu, omega = rs.standard_normal(d), hrc.spd(rs, d)
    z = rs.standard_normal(H * d + 2 * d + d * (d - 1))
    it = iter(z)
    counts = np.array([[2.0, 1.0, 3.0], [0.0, 0.0, 0.0]])
    totals = np.array([[0.5, -1.0, 2.0], [0.0, 0.0, 0.0]])
    out = hro.draw(model, 0.7, totals, counts, mu, omega, lambda: next(it), lambda a, s: a * s)
    L = np.linalg.cholesky(omega)
    want = mu + np.linalg.solve(L.T, z[d:2 * d])
    assert np.max(np.abs(out["beta"][1] - want)) < 1e-12
    assert np.max(np.abs(out["beta"][0] - want)) > 1e-3


def test_wishart_mean():
    """N = 4000 seeded draws of rWish(nu, V), d = 3: every entry's mean is nu V within 5 standard errors
    (Var W_ij = nu (V_ij^2 + V_ii V_jj)); about 2 s"""
    rs = np.random.Generator(np.random.PCG64(5))
    d, nu, N = 3, 6.5, 4000
    V = hrc.spd(rs, d)
    acc = np.zeros((d, d))
    for _ in range(N):
        acc += hro.rwish(nu, V, rs.standard_normal, lambda a, s: rs.gamma(a, s))
    se = np.sqrt(nu * (V * V + np.outer(np.diag(V), np.diag(V))) / N)
    assert np.all(np.abs(acc / N - nu * V) < 5 * se), (acc / N, nu * V, se)


@pytest.mark.parametrize("H,d", [(1, 1), (2, 3), (5, 3), (16, 16)])
def test_a_round_consumes_the_stated_count(H, d):
    n = [0]

    def rnorm():
        n[0] += 1
        return 0.0

    def rgamma(a, s):
        n[0] += 1
        return a * s

    model = hro.hier_model(H, d, (np.zeros(d), np.eye(d)), (np.eye(d), d + 1.0), None)
    hro.draw(model, 1.0, np.zeros((H, d)), np.ones((H, d)), np.zeros(d), np.eye(d), rnorm, rgamma)
    assert n[0] == H * d + 2 * d + 2 * (d + d * (d - 1) // 2) == hro.count_draws(H, d)


def test_step_3_centres_at_the_first_mean_and_keeps_beta():
    """mu is the coefficient draw of the centred regression by a dense solve (normals = 0), Omega's scale matrix
    is built from beta - mu', not beta - mu"""
    rs = np.random.Generator(np.random.PCG64(6))
    H, d, sigsq = 3, 2, 1.3
    model = hro.hier_model(H, d, (rs.standard_normal(d), hrc.spd(rs, d)), (hrc.spd(rs, d), 4.0), None)
    counts = rs.integers(1, 5, size=(H, d)).astype(np.float64)
    totals = rs.standard_normal((H, d)) * counts
    mu, omega = rs.standard_normal(d), hrc.spd(rs, d)
    out = hro.draw(model, sigsq, totals, counts, mu, omega, zero, lambda a, s: a * s)
    hy = hro.hyper(model)
    bbar = out["beta"].mean(0)
    I = H * omega + hy["sinv0"]
    assert np.allclose(out["mu1"], np.linalg.solve(I, H * omega @ bbar + hy["sinv0mu0"]), rtol=0, atol=1e-12)
    c = out["beta"] - out["mu1"]
    A = np.diag(counts.sum(0)) / sigsq + hy["sinv0"]
    b = (totals - counts * c).sum(0) / sigsq + hy["sinv0mu0"]
    assert np.allclose(out["mu"], np.linalg.solve(A, b), rtol=0, atol=1e-12)
    V = np.linalg.inv(c.T @ c + hy["s0"])
    Cf = np.linalg.cholesky(V)
    assert np.allclose(out["omega"], Cf @ np.diag(4.0 + H - np.arange(d)) @ Cf.T, rtol=1e-12, atol=0)
    assert np.allclose(hy["s0"], 4.0 * model["variance_prior"][0]) and np.allclose(hy["sinv0"] @ model["mean_prior"][1], np.eye(d))


def test_the_two_precisions_agree_on_the_ill_conditioned_case():
    """the probe's case with cond(Omega) = KAPPA = 1e6: the float64 and the long double restatement agree to
    better than 1e-6 relative per output, so a gate of 4 x their difference means something there"""
    case = [c for c in hrc.probe_cases() if "condition" in c["name"]][0]
    kappa = np.linalg.cond(case["omega"])
    assert 0.5 * hrc.KAPPA < kappa < 2 * hrc.KAPPA, kappa
    rs = np.random.Generator(np.random.PCG64(7))

    class Source:
        rnorm = staticmethod(rs.standard_normal)
        rgamma = staticmethod(lambda a, s: rs.gamma(a, s))

    lo, hi = hro.draw_both(case["model"], case["sigsq"], case["totals"], case["counts"], case["mu"], case["omega"], Source)
    for key in ("beta", "mu1", "mu", "omega"):
        rel = float(np.max(np.abs(lo[key] - hi[key])) / np.max(np.abs(hi[key])))
        print("%s: relative difference of the two precisions %.3e" % (key, rel))
        assert rel < 1e-6, (key, rel)
