"""CPU-side checks of the multinomial logit spike-and-slab path (MLVS): the C-ABI and the bindings
declare it, the restatement (tests/mlogit_oracle.py, the parity yardstick of the device) unmixes
and imputes with the right laws, every parity case of the GPU test meets the condition on its
inputs, and the restatement's posterior agrees with a quadrature of the exact posterior."""
import math
import os
import re

import numpy as np
import pytest
from scipy import stats

import mlogit_cases as mc
import mlogit_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ba_mlogit_set_data", "ba_mlogit_set_flip_order", "ba_mlogit_allow_model_selection", "ba_mlogit_sweep",
           "ba_mlogit_get_latent", "ba_mlogit_get_wss")
TEXTS = ("call ba_mlogit_set_data first", "multinomial logit data are set: use ba_mlogit_sweep",
         "MLVS did not start with a legal configuration.",
         "The multinomial logit sampler holds models of up to 64 included variables; a chain needs more.",
         "the multinomial logit sampler takes a fixed-precision slab (scales_with_sigsq = 0)",
         "the number of choices must be between 2 and 16", "exceeds 8 GiB")
# the 0.001-level critical value of the one-sample Kolmogorov-Smirnov statistic, sqrt(-ln(alpha / 2) / 2) / sqrt(n)
KS_001 = math.sqrt(-math.log(0.0005) / 2.0)


def test_header_declares_and_capi_binds_the_mlogit_entries():
    txt = open(os.path.join(ROOT, "include", "boom_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from boom_amd.capi import SIGNATURES
    import boom_amd
    lib = boom_amd.load_library()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("mlogit_set_data", "mlogit_set_flip_order", "mlogit_allow_model_selection", "mlogit_sweep",
                 "mlogit_get_latent", "mlogit_get_wss"):
        assert hasattr(boom_amd.Engine, name), name


def test_library_holds_the_refusal_texts():
    import boom_amd
    boom_amd.load_library()
    blob = open(os.path.join(ROOT, "boom_amd", "libboomamd.so"), "rb").read()
    for t in TEXTS:
        assert t.encode() in blob, t


def test_pybind_module_has_the_mlogit_names():
    import boom_amd._boom as boom
    for name in ("MultinomialLogitModel", "MLVS", "mlvs_flip_order"):
        assert hasattr(boom, name), name
    for name in ("draw", "suppress_model_selection", "allow_model_selection", "limit_model_selection", "max_nflips",
                 "logpri"):
        assert hasattr(boom.MLVS, name), name


@pytest.mark.parametrize("n", [1, 2, 9, 520])
def test_flip_order_is_a_permutation_and_the_facades(n):
    import boom_amd._boom as boom
    a, b = boom.mlvs_flip_order(n), boom.mlvs_flip_order(n)
    assert sorted(a) == list(range(n)) and a == b      # (a fresh engine every call: the same order)
    # the facade's MLVS hands the engine this very order (include/boom_amd.hpp calls the same function)
    src = open(os.path.join(ROOT, "include", "boom_amd.hpp")).read()
    assert "std::shuffle(v.begin(), v.end(), std::default_random_engine())" in src
    assert "mlvs_flip_order(model_->beta_size())" in src


def test_mixture_tables():
    assert abs(mo.MIX_WEIGHT.sum() - 1.0) < 1e-12
    assert np.allclose(mo.MIX_SD ** 2, mo.MIX_VAR, rtol=1e-15) and np.allclose(mo.MIX_PREC * mo.MIX_VAR, 1.0, rtol=1e-15)
    # the mixture approximates the law of -log(Exp(1)): mean Euler's constant, variance pi^2 / 6
    mean = float(mo.MIX_WEIGHT @ mo.MIX_MU)
    var = float(mo.MIX_WEIGHT @ (mo.MIX_VAR + mo.MIX_MU ** 2)) - mean ** 2
    assert abs(mean - 0.5772156649) < 0.01 and abs(var - math.pi ** 2 / 6) < 0.02


@pytest.mark.parametrize("v", [-3.0, -0.7, 0.0, 0.4, 2.5, 6.0, 11.0])
def test_unmix_posterior_against_direct_evaluation(v):
    direct = mo.MIX_WEIGHT * stats.norm.pdf(v, loc=mo.MIX_MU, scale=np.sqrt(mo.MIX_VAR))
    direct /= direct.sum()
    got = np.array(mo.unmix_posterior(v))
    assert np.allclose(got, direct, rtol=1e-12, atol=1e-300)
    # ... and rmulti's scan picks the first k with tmp <= psum
    cum = np.cumsum(got)
    for u in (1e-9, 0.2, 0.5, 0.8, 1 - 1e-9):
        k, margin = mo.unmix(v, lambda: u)
        assert k == int(np.argmax(u * cum[-1] <= cum)) and margin >= 0


def test_utilities_have_the_right_law():
    """fixed eta: z_y = exp(-u_y) is the minimum, Exp(rate sum_m exp(eta_m)); for m != y,
    exp(-u_m) - exp(-u_y) is Exp(rate exp(eta_m)) (the utilities before the mixture shift).
    20 000 draws; the Kolmogorov-Smirnov statistic below the 0.001-level critical value."""
    eta, y, ndraw = [0.3, -0.8, 1.1], 1, 20000
    rs = np.random.default_rng(48)
    U = np.array([mo.impute_point(eta, y, rs.random, shift=False)[0] for _ in range(ndraw)])
    z = np.exp(-U)
    crit = KS_001 / math.sqrt(ndraw)
    lam = sum(math.exp(e) for e in eta)
    d = [stats.kstest(z[:, y], stats.expon(scale=1.0 / lam).cdf).statistic]
    for m in (0, 2):
        assert np.all(z[:, m] > z[:, y])
        d.append(stats.kstest(z[:, m] - z[:, y], stats.expon(scale=math.exp(-eta[m])).cdf).statistic)
    print("KS statistics", d, "critical value", crit)
    assert max(d) < crit, (d, crit)
    # 2 M uniforms an observation, in the reference's order
    calls = [0]

    def unif():
        calls[0] += 1
        return rs.random()
    mo.impute_point(eta, y, unif)
    assert calls[0] == 2 * len(eta)


def test_batch_imputer_is_the_scalar_one():
    """impute_batch (the statistical tests' imputer) on the uniforms impute_point reads, in its order"""
    rs = np.random.default_rng(3)
    n, M = 40, 4
    eta = rs.standard_normal((n, M))
    y = rs.integers(0, M, n)
    U0, U1, U2 = rs.random(n), rs.random((n, M)), rs.random((n, M))
    ub, wb, kb = mo.impute_batch(eta, y, U0, U1, U2)
    for i in range(n):
        seq = [U0[i]]
        for m in range(M):
            if m != y[i]:
                seq.append(U1[i, m])
            seq.append(U2[i, m])
        it = iter(seq)
        u, w = mo.impute_point(eta[i].tolist(), int(y[i]), lambda: next(it))
        assert np.array_equal(w, wb[i]) and np.allclose(u, ub[i], rtol=0, atol=1e-12)


def test_expanded_design_layout():
    n, M, psub, pch = 3, 3, 2, 1
    Xs = np.arange(1, 7, dtype=float).reshape(n, psub)
    Xc = 10.0 + np.arange(n * M, dtype=float).reshape(n * M, pch)
    X = mo.expand_design(Xs, Xc, n, M)
    assert X.shape == (9, 5)
    for i in range(n):
        assert np.all(X[i * M, :4] == 0)                       # the baseline choice has no subject block
        assert np.array_equal(X[i * M + 1, :2], Xs[i]) and np.all(X[i * M + 1, 2:4] == 0)
        assert np.array_equal(X[i * M + 2, 2:4], Xs[i]) and np.all(X[i * M + 2, :2] == 0)
    assert np.array_equal(X[:, 4], Xc[:, 0])


def test_parity_cases_meet_the_condition_on_inputs(oracle):
    """every parity case of tests/test_mlogit_gpu.py: in every compared sweep the restatement's
    smallest flip margin is above 1e-8 and its smallest unmix margin above 1e-9"""
    for name in sorted(mc.PARITY):
        if name in ("D520", "chains1024"):
            continue                      # (checked when the seeds were chosen; the GPU test asserts it again)
        case = mc.PARITY[name]()
        ora = mc.make_oracles(oracle, case)
        oracle.set_slot_limit(case.get("slot_limit", 0))
        try:
            for _ in range(case["nsweeps"] + (1 if name == "empty" else 0)):
                for o in ora.values():
                    o.draw()
        finally:
            oracle.set_slot_limit(0)
        assert mc.margins_ok(ora), name
        if name == "empty":
            assert all(o.gamma.sum() == 0 for o in ora.values())


def test_restatement_posterior_matches_quadrature():
    """selection off, M = 3, intercepts only (D = 2), n = 200: the restatement's posterior mean
    over 4000 draws after 500 against the 2-D quadrature.  Allowed per coordinate: 4 Monte-Carlo
    standard errors (batch means of the run itself) plus the mixture approximation's own bias
    (mlogit_cases.MIXTURE_BIAS, measured once)."""
    case = mc.intercept_case()
    exact = mc.intercept_quadrature(case)
    d = mc.restatement_run(case, 500, 4000, 4000)
    nb = 40
    bm = d.reshape(nb, -1, 2).mean(axis=1)
    mean, se = d.mean(axis=0), bm.std(axis=0, ddof=1) / math.sqrt(nb)
    print("restatement", mean, "quadrature", exact, "se", se, "bias allowance", mc.MIXTURE_BIAS)
    assert np.all(np.abs(mean - exact) <= 4 * se + mc.MIXTURE_BIAS), (mean, exact, se)
