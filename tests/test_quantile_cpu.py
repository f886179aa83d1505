"""CPU-side checks of the quantile regression spike-and-slab path: the C-ABI and the bindings
declare it, and the restatement's imputation (tests/quantile_oracle.py, the parity yardstick of
the device) draws inverse-Gaussian weights, evaluates the smaller root stably -- the one place
where it and the device kernel leave the reference's arithmetic -- and forms z without the
detour through 1 / w."""
import os
import re
from decimal import Decimal, getcontext

import numpy as np
import pytest
from scipy import stats

from quantile_oracle import impute_point, reference_root, rig, smaller_root

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ba_quantile_set_data", "ba_quantile_sweep", "ba_quantile_get_weights")


def test_header_declares_and_capi_binds_the_quantile_entries():
    txt = open(os.path.join(ROOT, "include", "boom_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from boom_amd.capi import SIGNATURES
    import boom_amd
    lib = boom_amd.load_library()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("quantile_set_data", "quantile_sweep", "quantile_get_weights"):
        assert hasattr(boom_amd.Engine, name), name


def test_pybind_module_has_the_quantile_names():
    import boom_amd._boom as boom
    for name in ("QuantileRegressionModel", "QuantileRegressionSpikeSlabSampler"):
        assert hasattr(boom, name), name
    for name in ("draw", "limit_model_selection"):
        assert hasattr(boom.QuantileRegressionSpikeSlabSampler, name), name


@pytest.mark.parametrize("mu", [0.05, 1.0, 40.0])
def test_restated_weights_are_inverse_gaussian(mu):
    # 20 000 draws of rig(mu, 1) against IG(mean mu, shape 1), which scipy writes
    # invgauss(mu / lambda, scale=lambda).  The bar is fixed before the first run: p > 1e-4
    # per case, 3e-4 family-wise over the three cases.
    rs = np.random.default_rng(1000 + int(100 * mu))
    w = rig(mu, 1.0, rs.standard_normal(20000), rs.random(20000))
    assert np.all(w > 0) and np.all(np.isfinite(w))
    assert stats.kstest(w, stats.invgauss(mu, scale=1.0).cdf).pvalue > 1e-4


def _exact_root(mu, y):
    """the smaller root at 60 digits from the float inputs mu and y (lambda = 1)"""
    mu, y = Decimal(float(mu)), Decimal(float(y))
    muy = mu * y
    return mu + muy * mu / 2 - mu / 2 * (muy * (4 + muy)).sqrt()


def test_stable_root_holds_where_the_reference_form_cancels():
    """18 000 draws (a 300 x 60-sweep run) at residuals |N(0, 1)|; on the 2 000 with the
    largest t = mu y / 2 the stable root is within 8 ulp of a 60-digit evaluation, while
    the reference's form is off by more than 1e-10 relative somewhere (measured on this sample:
    2.1e-7 at t = 2.0e4, the stable root within 2 ulp) -- the reason the kernel and the
    restatement deviate."""
    getcontext().prec = 60
    rs = np.random.default_rng(20261017)
    r = np.abs(rs.standard_normal(18000))
    y = rs.standard_normal(18000) ** 2
    mu = 1.0 / r
    t = mu * y / 2
    top = np.argsort(t)[-2000:]
    stable, ref = smaller_root(mu[top], y[top]), reference_root(mu[top], y[top])
    worst_ulp, worst_ref = 0.0, 0.0
    for k, i in enumerate(top):
        ex = _exact_root(mu[i], y[i])
        exf = float(ex)
        assert exf > 0
        worst_ulp = max(worst_ulp, float(abs(Decimal(float(stable[k])) - ex) / Decimal(float(np.spacing(exf)))))
        worst_ref = max(worst_ref, float(abs(Decimal(float(ref[k])) - ex) / ex))
    print("largest t %.3g: stable root %.2f ulp, reference form %.3g relative" % (t[top].max(), worst_ulp, worst_ref))
    assert worst_ulp <= 8.0, worst_ulp
    assert worst_ref > 1e-10, worst_ref


def test_z_is_formed_without_the_detour_and_zero_residuals_read_nothing():
    rs = np.random.default_rng(7)
    calls = [0]

    def norm():
        calls[0] += 1
        return rs.standard_normal()

    def unif():
        calls[0] += 1
        return rs.random()

    for q in (0.05, 0.25, 0.5, 0.9):
        shift = 1.0 - 2.0 * q          # = 2 (1 - q) - 1
        for _ in range(2000):
            y, eta = 3.0 * rs.standard_normal(), rs.standard_normal()
            before = calls[0]
            w, z, _ = impute_point(y, eta, shift, norm, unif)
            assert calls[0] == before + 2 and w > 0
            ystar = y - shift / w      # the reference's latent response
            larger = max(abs(w * y), abs(shift))
            assert abs(z - w * ystar) <= 4 * np.spacing(larger), (q, y, eta, w)
    # a zero residual, and one whose reciprocal overflows: out of the suf, nothing consumed
    before = calls[0]
    assert impute_point(1.25, 1.25, 0.5, norm, unif) == (0.0, 0.0, 0.0)
    assert impute_point(5e-324, 0.0, 0.5, norm, unif) == (0.0, 0.0, 0.0)
    assert calls[0] == before
