"""MLVS -- multinomial logit spike and slab -- on the device (ba_mlogit_*): the imputation of the
utilities and mixture components, weighted_sum_of_squares and the sweep's mode 3, against the
Python restatement of draw() on the same substreams (tests/mlogit_oracle.py), against a
quadrature of the exact posterior, and on its behaviour.

Bars: inclusion indicators bit-exact, the mixture component (through w) exact, u within 1e-9
absolute, wss within 1e-9 relative, beta within 1e-8 relative (the project's bar for every GLM
family).  Condition on the inputs, asserted in every parity case: in every compared sweep the
restatement's smallest flip margin |delta - logit(u)| is above 1e-8 and its smallest unmix
margin |tmp - psum_k| / probsum above 1e-9 -- a decision closer than that to its threshold may
fall either way with the two sides' rounding.  The seeds were chosen on the CPU to satisfy it
(mlogit_cases.py lists every case).
"""
import numpy as np
import pytest

import mlogit_cases as mc
from mlogit_oracle import MlogitOracle

pytestmark = pytest.mark.gpu
USE_M = "multinomial logit data are set: use ba_mlogit_sweep"
M_FIRST = "call ba_mlogit_set_data first"
LEGAL = "MLVS did not start with a legal configuration."


@pytest.mark.parametrize("name", sorted(mc.PARITY))
def test_mlogit_sweeps_match_restatement(oracle, name):
    case = mc.PARITY[name]()
    eng = mc.make_engine(case)
    ora = mc.make_oracles(oracle, case)
    if case.get("slot_limit"):
        eng.set_slot_limit(case["slot_limit"])
        oracle.set_slot_limit(case["slot_limit"])
    try:
        mc.check_parity(eng, ora, case["nsweeps"], each=case.get("each"))
    finally:
        oracle.set_slot_limit(0)
    if case.get("after"):
        case["after"](eng, ora)


def test_mlogit_forced_spill_changes_the_draws(oracle):
    """(the switch of the forced-spill parity case does something)"""
    case = mc.PARITY["spill"]()
    a, b = mc.make_engine(case), mc.make_engine(case)
    a.set_slot_limit(case["slot_limit"])
    a.mlogit_sweep(3)
    b.mlogit_sweep(3)
    assert not np.array_equal(a.get_states()[1], b.get_states()[1])


def test_mlogit_several_sweeps_in_one_call():
    case = mc.PARITY["n256_M3_p3_2"]()
    a, b = mc.make_engine(case), mc.make_engine(case)
    a.mlogit_sweep(4)
    for _ in range(4):
        b.mlogit_sweep(1)
    sa, sb = a.get_states(), b.get_states()
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    assert a.mlogit_get_wss(1) == b.mlogit_get_wss(1)        # (bit for bit: no atomics in the sum)


def test_mlogit_max_flips_visits_the_head_of_the_order(oracle):
    """max_flips = 3 with a non-identity order: only the first three entries ever change"""
    case = mc.PARITY["maxflips3"]()
    eng = mc.make_engine(case)
    ora = mc.make_oracles(oracle, case)
    head = set(int(j) for j in case["order"][:3])
    assert head != {0, 1, 2}
    g0 = case["g0"]
    moved = np.zeros(case["D"], bool)

    def each(s, gam, beta):
        moved[:] |= (gam != g0[None, :]).any(axis=0)
    mc.check_parity(eng, ora, case["nsweeps"], each=each)
    eng.mlogit_sweep(20)
    moved |= (eng.get_states()[0] != g0[None, :]).any(axis=0)
    assert moved.any() and set(np.flatnonzero(moved)) <= head, np.flatnonzero(moved)


def test_mlogit_illegal_start_is_reported():
    """a start whose prior value is -inf: no make_valid, the reference's report_error"""
    import boom_amd
    case = mc.PARITY["n37_M3_p5_0"]()
    case["pi"] = case["pi"].copy()
    case["pi"][2] = 0.0
    case["g0"] = case["g0"].copy()
    case["g0"][2] = 1                      # included, with prior probability 0
    eng = mc.make_engine(case)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.mlogit_sweep(1)
    assert LEGAL in str(ei.value) and ei.value.code == -5      # BA_E_ILLEGAL_START


def test_mlogit_reaches_the_empty_model(oracle):
    """no forced variable: the chain reaches the empty model, whose value adds wss / 2; gamma = 0,
    beta = 0, the device's wss is the restatement's and the sweep that follows is bit-equal"""
    case = mc.PARITY["empty"]()
    eng = mc.make_engine(case)
    ora = mc.make_oracles(oracle, case)
    mc.check_parity(eng, ora, case["nsweeps"])
    gam, beta, _ = eng.get_states()
    for c, o in ora.items():
        assert o.gamma.sum() == 0 and gam[c].sum() == 0 and np.all(beta[c] == 0.0)
        assert abs(eng.mlogit_get_wss(c) - o.wss) <= 1e-9 * o.wss
    mc.check_parity(eng, ora, 1)


def test_mlogit_mode3_is_not_mode2(oracle):
    """the same data, latent draws and stream under BinomialLogitSpikeSlabSampler's rules (what
    the sweep's mode 2 does: its shuffle, log(u) <= delta, no wss) give another chain: the
    device follows the MLVS restatement and not that one"""
    case = mc.PARITY["n256_M3_p3_2"]()
    eng = mc.make_engine(case)
    c = 0
    mlvs = mc.make_oracles(oracle, case)[c]
    other = mc.make_oracles(oracle, case, rules="logit")[c]
    same = True
    for s in range(case["nsweeps"]):
        eng.mlogit_sweep(1)
        g, b = mlvs.draw()
        g2, b2 = other.draw()
        gam, beta, _ = eng.get_states()
        assert np.array_equal(gam[c], g)
        same = same and np.array_equal(gam[c], g2) and np.allclose(beta[c], b2, rtol=1e-6, atol=0)
    assert not same


def test_mlogit_more_than_64_variables_stops():
    import boom_amd
    rng = np.random.default_rng(70)
    n, M, psub = 120, 2, 70
    Xs = rng.standard_normal((n, psub))
    Xs[:, 0] = 1.0
    y = rng.integers(0, M, n)
    case = dict(y=y, Xs=Xs, Xc=None, M=M, D=psub, mu=np.zeros(psub), prec=np.eye(psub), pi=np.ones(psub),
                g0=np.ones(psub, np.uint8), chains=2, seed=3, order=None, max_flips=-1)
    eng = mc.make_engine(case)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.mlogit_sweep(1)
    assert "up to 64 included variables" in str(ei.value) and ei.value.code == -8   # BA_E_MODEL_TOO_LARGE


def test_mlogit_recorded_draws_summaries_and_latent(oracle):
    case = mc.PARITY["n256_M3_p3_2"]()
    k, chains = 6, case["chains"]
    a = mc.make_engine(case)
    a.enable_draws(k)
    a.mlogit_sweep(k)
    b = mc.make_engine(case)
    rows = []
    for s in range(k):
        b.mlogit_sweep(1)
        rows.append(b.get_states())
    for c in (0, chains - 1):
        g, bb, s2 = a.get_draws(c, k)
        for s in range(k):
            G, B, S = rows[s]
            assert np.array_equal(g[s], G[c]) and np.array_equal(bb[s], B[c])
            assert s2[s] == 1.0 and S[c] == 1.0
        ua, wa = a.mlogit_get_latent(c)
        ub, wb = b.mlogit_get_latent(c)
        assert np.array_equal(ua, ub) and np.array_equal(wa, wb)
        assert ua.shape == (case["y"].shape[0] * case["M"],) and np.all(wa > 0)
    a.reset_summaries()
    a.mlogit_sweep(k)
    sm = a.get_summaries()
    assert sm["sweeps"] == chains * k
    assert np.all(sm["inclusion_count"] <= chains * k) and sm["inclusion_count"][0] == chains * k   # (0 is forced)


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
    elif kind == "quantile":
        eng.quantile_set_data(X, y, 0.5)
    else:
        eng.student_set_data(X, y)


def test_mlogit_refusals():
    import boom_amd
    rng = np.random.default_rng(1)
    n, M, psub = 200, 3, 2
    Xs = rng.standard_normal((n, psub))
    Xs[:, 0] = 1.0
    yc = rng.integers(0, M, n)
    D = (M - 1) * psub
    mu, prec, pi = np.zeros(D), np.eye(D), np.full(D, 0.5)
    eng = boom_amd.Engine(4, seed=1)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.mlogit_sweep(1)                                    # no data
    assert str(ei.value) == M_FIRST
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.mlogit_set_flip_order(np.arange(D))
    assert str(ei.value) == M_FIRST
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.mlogit_set_data(yc, Xs, None, 17)
    assert "between 2 and 16" in str(ei.value)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.mlogit_set_data(np.full(n, 3), Xs, None, 3)
    assert "responses" in str(ei.value)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.mlogit_set_data(yc, None, None, 3)
    assert "not both zero" in str(ei.value)
    eng.mlogit_set_data(yc, Xs, None, M)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.mlogit_set_flip_order(np.array([0, 1, 1, 3]))
    assert "permutation" in str(ei.value)
    eng.set_spike(pi)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=True)
    eng.set_state(np.ones(D, np.uint8))
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.mlogit_sweep(1)
    assert "fixed-precision slab" in str(ei.value)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=False)
    with pytest.raises(boom_amd.BoomAmdError):
        eng.set_state(np.ones(D, np.uint8), sigsq=2.0)         # sigma^2 is 1
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.mlogit_get_latent(0)                               # no imputation yet
    assert "ba_mlogit_sweep" in str(ei.value)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.mlogit_get_wss(0)
    assert "ba_mlogit_sweep" in str(ei.value)
    # every other sweep names this one
    for call in (eng.sweep, eng.sss_sweep, eng.adaptive_sweep, eng.probit_sweep, eng.logit_sweep,
                 eng.poisson_sweep, eng.student_sweep, eng.quantile_sweep, eng.ss_sweep):
        with pytest.raises(boom_amd.BoomAmdError) as ei:
            call(1)
        assert str(ei.value) == USE_M and ei.value.code == -9, call
    eng.mlogit_sweep(2)
    u, w = eng.mlogit_get_latent(3)
    assert np.all(np.isfinite(u)) and np.all(w > 0) and eng.mlogit_get_wss(3) > 0
    # ... and this one asks for its data while the engine holds another kind
    X = rng.standard_normal((n, 5))
    yr = rng.standard_normal(n)
    for kind in ("regression", "probit", "logit", "poisson", "student", "quantile", "state_space"):
        other = boom_amd.Engine(4, seed=1)
        _install(other, kind, X, yr)
        with pytest.raises(boom_amd.BoomAmdError) as ei:
            other.mlogit_sweep(1)
        # (quantile data send every other sweep to their own: that kind's rule, test_quantile_gpu.py)
        want = "quantile regression data are set: use ba_quantile_sweep" if kind == "quantile" else M_FIRST
        assert str(ei.value) == want and ei.value.code == -9, kind
        with pytest.raises(boom_amd.BoomAmdError) as ei:
            other.mlogit_get_latent(0)
        assert str(ei.value) == M_FIRST, kind
        other.close()
    # new data of another kind on the same engine: its sweep runs again
    eng.student_set_data(X, yr)
    eng.sss_set_slab(np.zeros(5), np.eye(5), scales_with_sigsq=True)
    eng.set_spike(np.full(5, 0.5))
    eng.set_state(np.zeros(5, np.uint8))
    eng.student_sweep(1)
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.mlogit_sweep(1)
    assert str(ei.value) == M_FIRST


def test_mlogit_pybind_sampler_equals_the_engine():
    import boom_amd._boom as boom
    case = mc.PARITY["n256_M3_p3_2"]()
    M, D, chains, seed = case["M"], case["D"], case["chains"], case["seed"]
    order = np.asarray(boom.mlvs_flip_order(D))
    assert sorted(order.tolist()) == list(range(D))
    model = boom.MultinomialLogitModel(M, case["Xs"].shape[1], case["Xc"].shape[1], chains=chains, seed=seed)
    assert model.Nchoices == M and model.subject_nvars == 3 and model.choice_nvars == 2 and model.beta_size == D
    model.set_data(case["y"], case["Xs"], case["Xc"])
    sampler = boom.MLVS(model, boom.MvnModel(case["mu"], case["prec"], True), boom.VariableSelectionPrior(case["pi"]))
    assert sampler.max_nflips() == D
    model.set_method(sampler)
    for j in range(D):
        if not case["g0"][j]:
            model.drop(j)
    case = dict(case, order=order)
    eng = mc.make_engine(case)
    for _ in range(6):
        model.sample_posterior()
        eng.mlogit_sweep(1)
        g, b, s = eng.get_state(0)
        assert np.array_equal(np.asarray(model.inc, dtype=np.uint8), g)
        assert np.array_equal(model.beta, b)
    sampler.limit_model_selection(2)
    assert sampler.max_nflips() == 2
    eng.sss_set_slab(case["mu"], case["prec"], scales_with_sigsq=False, max_flips=2)
    for _ in range(3):
        sampler.draw()
        eng.mlogit_sweep(1)
        g, b, s = eng.get_state(0)
        assert np.array_equal(np.asarray(model.inc, dtype=np.uint8), g) and np.array_equal(model.beta, b)
    sampler.suppress_model_selection()
    eng.mlogit_allow_model_selection(False)
    sampler.draw()
    eng.mlogit_sweep(1)
    g, b, s = eng.get_state(0)
    assert np.array_equal(np.asarray(model.inc, dtype=np.uint8), g) and np.array_equal(model.beta, b)
    with pytest.raises(Exception):
        sampler.logpri()


def test_mlogit_intercepts_posterior_matches_quadrature():
    """M = 3, intercepts only (D = 2), selection off: the device's posterior means against a 2-D
    quadrature of the exact multinomial logit posterior.  Allowed per coordinate: 4 Monte-Carlo
    standard errors (from the spread of the independent chains' means) plus the mixture
    approximation's own bias, the constant measured on the CPU (mlogit_cases.MIXTURE_BIAS)."""
    case = mc.intercept_case()
    exact = mc.intercept_quadrature(case)
    chains, burn, keep = 1024, 500, 400      # (the CPU test's burn-in: the chain forgets its start slowly)
    case = dict(case, chains=chains, seed=33)
    eng = mc.make_engine(case)
    eng.mlogit_allow_model_selection(False)
    eng.mlogit_sweep(burn)
    draws = np.zeros((keep, chains, 2))
    for t in range(keep):
        eng.mlogit_sweep(1)
        draws[t] = eng.get_states()[1]
    cm = draws.mean(axis=0)
    mean, se = cm.mean(axis=0), cm.std(axis=0, ddof=1) / np.sqrt(chains)
    print("device", mean, "quadrature", exact, "se", se, "bias allowance", mc.MIXTURE_BIAS)
    assert np.all(np.abs(mean - exact) <= 4 * se + mc.MIXTURE_BIAS), (mean, exact, se)
