"""CPU-side checks of the Student-t spike-and-slab path: the C-ABI and the bindings declare
it, and the restatement's slice sampler of nu (tests/student_oracle.py, the parity yardstick
of the device) draws from the right distribution."""
import os
import re

import numpy as np
import pytest
from scipy import stats
from scipy.special import gammaln

from student_oracle import nu_log_post, slice_draw_nu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ba_student_set_data", "ba_student_set_nu_prior", "ba_student_set_nu", "ba_student_get_nu",
           "ba_student_sweep", "ba_student_get_weights", "ba_student_get_nu_draws", "ba_student_get_margin")


def test_header_declares_and_capi_binds_the_student_entries():
    txt = open(os.path.join(ROOT, "include", "boom_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from boom_amd.capi import SIGNATURES
    import boom_amd
    lib = boom_amd.load_library()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in SIGNATURES, name
        assert hasattr(lib, name), name


def test_pybind_module_has_the_student_names():
    import boom_amd._boom as boom
    for name in ("TRegressionModel", "TRegressionSpikeSlabSampler", "UniformModel", "GammaModel"):
        assert hasattr(boom, name), name
    assert boom.UniformModel(0.1, 100.0).hi == 100.0
    assert boom.GammaModel(2.0, 0.1).alpha == 2.0


def _grid_cdf(u, n_log_sigma, prior, lo, hi):
    grid = np.linspace(lo, hi, 40001)
    lp = np.array([nu_log_post(v, u, n_log_sigma, prior) for v in grid])
    d = np.exp(lp - lp[np.isfinite(lp)].max())
    d[~np.isfinite(lp)] = 0.0
    c = np.concatenate([[0.0], np.cumsum(0.5 * (d[1:] + d[:-1]) * np.diff(grid))])
    c /= c[-1]
    return lambda x: np.interp(x, grid, c)


@pytest.mark.parametrize("prior", [(0, 0.1, 100.0), (1, 2.0, 0.1)])
def test_restated_nu_draws_follow_the_integrated_posterior(prior):
    # a fixed residual set (t with 4 degrees of freedom, scale 1.3); the KS threshold is fixed
    # before the first run: p > 1e-3 on 2000 draws thinned by 10
    rs = np.random.default_rng(4)
    r = 1.3 * rs.standard_t(4, 150)
    sigma = 1.3
    u = (r / sigma) ** 2
    nls = len(u) * np.log(sigma)
    logf = lambda v: nu_log_post(v, u, nls, prior)  # noqa: E731
    rng = np.random.default_rng(17)
    x, dx, draws = 30.0, 1.0, []
    for t in range(20000):
        x, dx, _ = slice_draw_nu(rng.random, rng.standard_exponential, logf, x, dx)
        if t % 10 == 9:
            draws.append(x)
    hi = 100.0 if prior[0] == 0 else 400.0
    cdf = _grid_cdf(u, nls, prior, 1e-3 if prior[0] else 0.1, hi)
    assert stats.kstest(np.array(draws), cdf).pvalue > 1e-3


def test_closed_form_dt_matches_scipy():
    x = np.linspace(-30, 30, 301)
    for nu in (0.3, 1.0, 3.0, 30.0, 99.0):
        mine = (gammaln((nu + 1) / 2) - gammaln(nu / 2) - 0.5 * np.log(nu * np.pi)
                - 0.5 * (nu + 1) * np.log1p(x * x / nu))
        assert np.max(np.abs(mine - stats.t.logpdf(x, nu)) / np.abs(stats.t.logpdf(x, nu))) < 1e-13
