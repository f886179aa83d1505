"""The imputation kernels of probit_kernel.hip, launched directly (tests/cpp/imputer_probe.hip,
which includes the product's file itself) and compared per observation with the references of
tests/imputer_ref.py: probit_impute_kernel, logit_impute_kernel<false|true>,
logit_pg_impute_kernel, poisson_impute_kernel<false|true>, latent_ss_h_kernel and
latent_ss_suf_kernel.  The chain tests see these numbers only after a GEMM and a sweep, as a
coefficient at 1e-8 on two chains; here every observation of every chain is compared.

Cases (imputer_ref.case_names; tests/test_imputer_ref_cpu.py asserts, without a GPU, that each
reaches the paths it is there for): per kernel n = 1, 255, 256, 257, 513 of the family's table of
edge observations, slot indices that pass 2^32, a chain that is not CHAIN_OK at entry, p = 1100
with the eight columns at the lanes', waves' and rounds' edges, exactly 1024 columns, 1025
columns; for probit the scheduling edges (256 near-side, 256 far-side, 24 hulls a hair on the far
side at 1e-9 and at 1e-12 and below, a hull of more than 64 points, clt_threshold 0 and 5, slot limits 1, 2 and 6).

Bounds: per observation, 4 x the spread of the reference over 8 replays -- its math functions
moved by up to U ulp, its fusable expressions by one -- + 8 ulp of the value (imputer_ref's
docstring and bounded()).  Status words, the values of missing steps, Polya-Gamma's z, the
sentinels of everything a kernel must not write and the guard bands (imputer_probe_lib) are
compared bit for bit.  Every test prints the largest error / bound; on the MI355X the largest per
kernel were probit 0.33, logit 0.25, logit<true> 0.25, Polya-Gamma 0.50, Poisson 0.13,
Poisson<true> 0.25.

Phase (3) of the probit kernel is compared by value in probit-phase3: 256 far-side observations
of which 11 or 12 per chain, at cuts of 2e-10 .. 1e-9, need hulls of 17 to 19 points.  It showed
that the kernel's hull integrals, their exponent contracted into fused multiply-adds, took other
segments than the reference's; the kernel now rounds that exponent as the reference does.

Two things are not compared by value.  In the extra case probit-tiny24 (cuts of 1e-12 .. 1e-15,
hulls up to 26 points) the reference's own hull is rounding noise (imputer_ref.probit_cases): the
observations whose replays disagree must get a finite draw on the right side of zero, the status
must stay and the rest of the workgroup be exact.  And the one observation whose hull outgrows 64
points: the kernel must set CHAIN_RNG_BRANCH on its chain and leave the others exact."""
import numpy as np
import pytest

import imputer_probe_lib as P
import imputer_ref as R
from rng_probe_lib import SENT_BITS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = P.load()
    assert (lib.ip_chain_ok(), lib.ip_chain_rng_branch(), lib.ip_chain_forecast_variance(),
            lib.ip_chain_model_too_large(), lib.ip_kmax()) == (R.OK, R.RNG_BRANCH, R.FORECAST_VARIANCE,
                                                                R.MODEL_TOO_LARGE, R.KMAX)
    assert lib.ip_logit_missing_variance() == R.MISSING_VARIANCE["logit_ss"]
    assert lib.ip_poisson_missing_variance() == R.MISSING_VARIANCE["poisson_ss"]
    return lib


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check(name, case, ref, got):
    """every observation of every chain; returns the largest error / bound"""
    kind = case["kind"]
    assert list(got["status"]) == list(ref["status"]), (name, got["status"], ref["status"])
    # (an observation whose hull outgrew 64 points has no reference value: the kernel reports it
    # in the status word, compared above, and what it writes there is not specified)
    free = np.zeros_like(ref["written"])
    for c, i, ob in ref["facts"]:
        free[c, i] = ob.status == "rng_branch"
    worst = 0.0
    for arr in P.ARRAYS:
        g = got[arr]
        if arr not in R.OUTPUTS[kind]:
            assert np.all(g == SENT_BITS), "%s: %s was written" % (name, arr)
            continue
        w = ref["written"]
        loose = ref["loose"] != 0
        if loose.any():
            # (no reference value: a finite draw on its side of zero; imputer_ref.probit_cases)
            v = g.view(np.float64)[loose]
            assert not np.any(g[loose] == SENT_BITS) and np.all(np.isfinite(v)) and np.all(v * ref["loose"][loose] > 0)
            free = free | loose
        assert np.all(g[~w & ~free] == SENT_BITS), "%s: %s written where nothing belongs" % (name, arr)
        assert not np.any(g[w] == SENT_BITS), "%s: %s not written at %s" % (name, arr, np.argwhere(w & (g == SENT_BITS))[:4])
        want, bound, val = ref["want"][arr], ref["bound"][arr], g.view(np.float64)
        exact = ref["exact"] | (w if (kind == "pg" and arr == "z") else False)
        assert np.array_equal(g[exact], _bits(want[exact])), "%s: %s differs where it is exact" % (name, arr)
        m = w & ~exact
        if m.any():
            ratio = np.abs(val[m] - want[m]) / bound[m]
            worst = max(worst, float(ratio.max()))
            at = np.argwhere(m)[int(np.argmax(ratio))]
            assert np.all(ratio <= 1.0), "%s: %s[chain %d, %d] = %r, reference %r, bound %g (ratio %.3g)" % (
                name, arr, at[0], at[1], val[tuple(at)], want[tuple(at)], bound[tuple(at)], ratio.max())
    print("%s: largest error / bound %.3g" % (name, worst))
    return worst


@pytest.mark.parametrize("name", R.case_names())
def test_kernel_matches_reference(lib, name):
    case = R.case_of(name)
    assert case is not None
    check(name, case, R.ref_of(name), P.run(lib, case))


def _ss_frame(n, chains=3):
    """a state space frame for the two helpers: X, gamma, beta, y and trials are not read"""
    case = R.table_case("logit_ss", n)
    case["chains"] = chains
    return case


@pytest.mark.parametrize("family", ["poisson", "logit"])
@pytest.mark.parametrize("n", [1, 257, 513])
def test_latent_ss_h(lib, family, n):
    """h = 1 / q bit for bit, the family's variance at a missing step; nothing else is written"""
    case = _ss_frame(n)
    case["clt"] = 0 if family == "poisson" else 1           # (the probe's family switch)
    q = np.random.RandomState(n).uniform(1e-3, 50.0, (3, n))
    got = P.run(lib, case, "ss_h", inputs=dict(w=q))
    obs = case["observed"].astype(bool)
    want = np.where(obs, 1.0 / q, R.MISSING_VARIANCE[family + "_ss"])
    assert np.array_equal(got["h"], _bits(want))
    assert np.array_equal(got["w"], _bits(q)) and np.all(got["z"] == SENT_BITS) and np.all(got["value"] == SENT_BITS)
    assert list(got["status"]) == [R.OK] * 3


@pytest.mark.parametrize("bad", [0.0, -1.0, np.inf, np.nan])
def test_latent_ss_h_reports_a_precision_that_is_none(lib, bad):
    """q = 0, -1, inf or NaN at an observed step sets CHAIN_FORECAST_VARIANCE on that chain alone;
    a chain in error at entry is left alone.  (Seven steps: one wavefront, so that which steps of
    the failing chain are still written does not depend on timing)"""
    n = 7
    case = _ss_frame(n)
    case["clt"] = 1
    case["status0"][2] = R.MODEL_TOO_LARGE
    obs = case["observed"].astype(bool)
    assert list(obs) == [True, True, True, False, True, True, True]
    q = np.random.RandomState(3).uniform(0.5, 2.0, (3, n))
    q[1, 2] = bad
    q[1, 3] = bad                                            # (a missing step's precision is not read)
    q[0, 3] = bad
    got = P.run(lib, case, "ss_h", inputs=dict(w=q))
    assert list(got["status"]) == [R.OK, R.FORECAST_VARIANCE, R.MODEL_TOO_LARGE]
    want = _bits(np.where(obs, 1.0 / np.where(np.isfinite(q) & (q > 0), q, 1.0), R.MISSING_VARIANCE["logit_ss"]))
    want[1, 2] = SENT_BITS
    want[2, :] = SENT_BITS
    assert np.array_equal(got["h"], want)


@pytest.mark.parametrize("n", [1, 257, 513])
def test_latent_ss_suf(lib, n):
    """z = (value - offset) q, the same expression in double, bit for bit; 0 and weight 0 at a
    missing step"""
    case = _ss_frame(n)
    rs = np.random.RandomState(100 + n)
    q, v = rs.uniform(1e-3, 50.0, (3, n)), rs.normal(0.0, 3.0, (3, n))
    got = P.run(lib, case, "ss_suf", inputs=dict(w=q, value=v))
    obs = case["observed"].astype(bool)
    assert case["offset_stride"] > n
    off = case["offset"][:, :n]
    assert np.array_equal(got["z"], _bits(np.where(obs, (v - off) * q, 0.0)))
    assert np.array_equal(got["w"], _bits(np.where(obs, q, 0.0)))
    assert np.array_equal(got["value"], _bits(v)) and np.all(got["h"] == SENT_BITS)
    assert list(got["status"]) == [R.OK] * 3
