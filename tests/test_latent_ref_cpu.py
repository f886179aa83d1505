"""The references of tests/latent_ref.py, pinned here without a GPU: each case of
tests/test_latent_kernels_gpu.py reaches the path it is there for, the observations without a
reference value (LOOSE: their replays disagree) are none in the edge tables and at most 1 % of any
case, and the references themselves are held to something higher -- the oracle's own functions bit
for bit on the host's math, mpmath at 60 digits, math.fsum."""
import ctypes as C
import math

import mpmath
import numpy as np
import pytest

import imputer_ref as ir
import latent_ref as R
import mlogit_oracle as mo
import quantile_oracle as qo
import student_oracle as so

mpmath.mp.dps = 60
EDGE_TABLES = [n for n in R.case_names() if n.split("-")[1][0] == "n" or n.split("-")[1] in ("tiny160", "huge300", "infbeta")]


def _facts(name):
    return R.ref_of(name)["facts"]


@pytest.mark.parametrize("name", R.case_names())
def test_loose_share(name):
    """at most 1 % of a case's observations have no reference value, none in the edge tables"""
    ref = R.ref_of(name)
    live = ref["written"].sum()
    share = ref["loose"].sum() / max(1, live)
    assert share <= R.LOOSE_CAP, (name, share)
    if name in EDGE_TABLES:
        assert not ref["loose"].any(), name


@pytest.mark.parametrize("name", sorted(R.sigma_nu_cases()))
def test_sigma_nu_chains_have_a_reference(name):
    ref = R.sigma_nu_ref(name)
    for ch in ref["chains"]:
        assert ch is None or ch[2], name


def test_statuses():
    ok = [R.OK] * 3
    for kind in R.KINDS:
        chains = 7 if kind.startswith("student") else 3
        for n in R.SIZES:
            assert list(R.ref_of("%s-n%d" % (kind, n))["status"]) == [R.OK] * chains
        for what in ("crossing", "offset7", "model1024", "slot1"):
            assert list(R.ref_of("%s-%s" % (kind, what))["status"]) == ok, (kind, what)
        assert list(R.ref_of(kind + "-parked")["status"]) == [R.OK, R.FORECAST_VARIANCE, R.OK]
        ref = R.ref_of(kind + "-model1025")
        assert list(ref["status"]) == [R.OK, R.MODEL_TOO_LARGE, R.OK] and not ref["written"][1].any()
        assert not R.ref_of(kind + "-parked")["written"][1].any()
        case = R.case_of(kind + "-model1024")
        assert all(int(g.sum()) == R.KMAX for g in case["gamma"]) and case["p"] == 1100 and case["n"] == 257
        assert int(R.case_of(kind + "-model1025")["gamma"][1].sum()) == R.KMAX + 1
        assert R.case_of(kind + "-offset7")["chain_offset"] == 7
    assert list(R.ref_of("quantile-tiny160")["status"]) == [R.OK, R.OK, R.QUANTILE_WEIGHT_ERROR]
    assert list(R.ref_of("quantile-huge300")["status"]) == [R.QUANTILE_WEIGHT_ERROR, R.OK, R.OK]
    assert list(R.ref_of("mlogit-infbeta")["status"]) == [R.OK, R.OK, R.MLOGIT_IMPUTE_ERROR]


def test_default_models():
    """chain 0 two coefficients, chain 1 an empty model, chain 2 one; products that round only where
    the case's linear predictor is moved by the replays"""
    for kind in R.KINDS:
        case = R.case_of(kind + "-n257")
        assert [int(g.sum()) for g in case["gamma"][:3]] == [2, 0, 1]
        assert bool(case.get("exact_eta")) == (kind == "quantile")


def test_slots_cross_2_32_and_spill():
    for kind in R.KINDS:
        case = R.case_of(kind + "-crossing")
        lo, hi = case["sweep"] * case["n"], case["sweep"] * case["n"] + case["n"] - 1
        assert lo < 2 ** 32 <= hi
        # a slot that serves one uniform: every observation that reads two or more ends in its spill stream
        wheres = [ob.facts["where"] for _, _, ob in _facts(kind + "-slot1") if ob.facts.get("where")]
        streams = {w[0] for w in wheres}
        assert any(s & 0x80000000 for s in streams), kind
        plain = [ob.facts["where"] for _, _, ob in _facts(kind + "-n257") if ob.facts.get("where")]
        assert not any(w[0] & 0x80000000 for w in plain)


# ---- Student -----------------------------------------------------------------------------------------
def test_student_table_reaches_its_paths():
    arms, exits, deltas = set(), set(), set()
    for n in R.SIZES:
        for c, i, ob in _facts("student-n%d" % n):
            arms.update(ob.sig[0])
        for c, i, ob in _facts("student_ss-n%d" % n):
            exits.add((ob.facts["exit"], ob.sig[0] == "missing"))
    # the gamma sampler's algorithms: GS (shape (0.11 + 1) / 2 < 1) and GD with its rejection loop
    assert {"gs_low", "gs_high", "gd_immediate", "gd_squeeze", "gd_quotient", "loop_round"} <= arms, arms
    # H_t: sigsq / w at an observed step; at a missing step the marginal variance (nu > 2) and sigsq 1e8 (nu <= 2)
    assert exits == {("weight", False), ("marginal", True), ("floor", True)}
    case = R.case_of("student_ss-n513")
    assert [i for i in range(513) if not case["observed"][i]] == [0, 63, 64, 255, 256, 512]
    assert case["offset_stride"] > case["n"] and tuple(case["nu"]) == R.CHAIN_NUS
    _assert_full_cross("student-n513", range(7), set(R.NUS))
    _assert_full_cross("student_ss-n513", range(7), set(R.NUS))
    # the three-chain cases: the table's first two nu, 0.11 and 1, on the chains that have a model
    for what in ("crossing", "offset7", "parked", "slot1"):
        _assert_full_cross("student-" + what, range(3), {0.11, 1.0})


def _assert_full_cross(name, chains, nus):
    """every delta of the table meets every nu of `nus` on a chain that has a model -- no chain left
    out but the empty model's, whose nu is a repeat --, and every response meets every delta.  A
    delta is met to the rounding of eta = y - offset - delta sigma: every number that enters is
    below 4 + |delta| sigma, a handful of roundings at that size, divided by sigma"""
    case = R.case_of(name)
    assert int(case["gamma"][1].sum()) == 0
    # (of the whole table, the empty model's nu is one that a chain with a model has too)
    assert len(chains) < 7 or case["nu"][1] in [case["nu"][c] for c in chains if c != 1]
    met = set()
    for c in chains:
        if c == 1:
            continue
        assert int(case["gamma"][c].sum()) >= 1
        sigma = math.sqrt(case["sigsq"][c])
        yi = case["y"] - (case["offset"][c, :case["n"]] if "offset" in case else 0.0)
        d = (yi - R.eta_rows(case, c)) / sigma
        live = case["observed"].astype(bool) if "observed" in case else np.ones(case["n"], bool)
        for want in R.DELTAS:
            tol = 8 * math.ulp(4.0 + abs(want) * sigma) / sigma
            hit = live & (np.abs(d - want) <= tol)
            assert {float(v) for v in case["y"][hit]} == set(R.STUDENT_Y), (name, c, want)
            met.add((float(case["nu"][c]), want))
    assert met == {(nu, want) for nu in nus for want in R.DELTAS}, name


def test_student_weight_is_the_oracles():
    """on the host's functions the reference's weight is bo_rgamma's, bit for bit and to the stream
    position, as StudentOracle.impute draws it; the rate against mpmath"""
    o = ir.oracle()
    case = R.case_of("student-n255")
    for c in range(case["chains"]):
        eta = R.eta_rows(case, c)
        nu, sigsq = float(case["nu"][c]), float(case["sigsq"][c])
        for i in range(0, 255, 7):
            ob = R.student_obs(case["seed"], case["chain_offset"] + c, case["sweep"], i, 255, float(eta[i]), float(case["y"][i]),
                               sigsq, nu)
            rng = ir.slot_rng(case["seed"], case["chain_offset"] + c, R.STUDENT_STREAM, R.STUDENT_STRIDE, case["sweep"] * 255 + i)
            delta = (case["y"][i] - eta[i]) / np.sqrt(sigsq)
            rate = 0.5 * (nu + delta * delta)
            w = o.gammas(rng, 0.5 * (nu + 1), rate, 1)[0]
            assert ob.out[("w", 0)] == w and ob.facts["where"] == ir._where(rng)
            assert ob.out[("z", 0)] == w * case["y"][i]
            exact = (mpmath.mpf(nu) + (mpmath.mpf(float(case["y"][i])) - mpmath.mpf(float(eta[i]))) ** 2 / mpmath.mpf(sigsq)) / 2
            assert abs(mpmath.mpf(ob.facts["rate"]) - exact) <= 4 * mpmath.mpf(math.ulp(rate))


# ---- quantile ----------------------------------------------------------------------------------------
def test_quantile_table_reaches_its_paths():
    branches, seen = set(), set()
    for n in R.SIZES:
        case = R.case_of("quantile-n%d" % n)
        assert case["shift"] == 1.0 - 2.0 * R.QUANTILES[n]
        for c, i, ob in _facts("quantile-n%d" % n):
            branches.add(ob.facts["branch"])
            if c != 1:
                seen.add(abs(float(case["y"][i]) - float(R.eta_rows(case, c)[i])))
    assert branches == {"none", "smaller", "larger"}
    assert {R.QUANTILES[n] for n in R.SIZES} == {0.05, 0.5, 0.95}
    # 0, 5e-324 and 1e-310 exactly (no number is read there); the others to the rounding of y - d
    assert {0.0, 5e-324, 1e-310, 1.0, 1e6} <= seen
    assert any(abs(r - 1e-12) < 1e-15 for r in seen) and any(abs(r - 1e-6) < 1e-15 for r in seen)
    for r, none in ((0.0, True), (5e-324, True), (1e-310, True), (1e-12, False)):
        ob = R.quantile_obs(R.SEED, 5, 3, 0, 1, -r, 0.0, 0.9)
        assert (ob.facts["branch"] == "none") == none
        if none:
            assert ob.out == {("w", 0): 0.0, ("z", 0): 0.0} and ob.facts["where"][1] == 3 * R.QUANTILE_STRIDE   # (the slot's start: nothing read)


def test_quantile_extremes():
    """1e-160: the root's t (2 + t) overflows, the draw is 0 and the kernel's rule makes that
    QUANTILE_WEIGHT_ERROR -- on every slot, by the smaller root: u > mu / (mu + x) cannot hold where
    mu / (mu + x) rounds to 1, so NO slot takes the larger root there (searched below); the larger
    root's own failure, mu mu / x = 0 / x, is the case at 1e300, where half the slots take it"""
    larger = errors = 0
    for i in range(256):
        ob = R.quantile_obs(R.SEED, R.CHAIN_OFFSET + 2, R.SWEEP, i, 257, 1e-160, 0.0, 0.9)
        larger += ob.facts["branch"] == "larger"
        errors += ob.status == "weight_error"
        assert ob.out == {("w", 0): 0.0, ("z", 0): 0.0}
    assert larger == 0 and errors == 256
    facts = [ob for c, i, ob in _facts("quantile-tiny160") if ob.status == "weight_error"]
    assert facts and all(ob.facts["branch"] == "smaller" and ob.facts["t"] > 1e154 for ob in facts)
    facts = [ob for c, i, ob in _facts("quantile-huge300") if ob.status == "weight_error"]
    assert facts and all(ob.facts["branch"] == "larger" for ob in facts)
    assert all(c == 0 for c, i, ob in _facts("quantile-huge300") if ob.status)
    assert all(c == 2 for c, i, ob in _facts("quantile-tiny160") if ob.status)


def test_quantile_reference_is_the_oracles_and_the_root_exact():
    o = ir.oracle()
    case = R.case_of("quantile-n257")
    for c in range(3):
        eta = R.eta_rows(case, c)
        for i in range(257):
            ob = R.quantile_obs(case["seed"], case["chain_offset"] + c, case["sweep"], i, 257, float(eta[i]), float(case["y"][i]),
                                case["shift"])
            rng = ir.slot_rng(case["seed"], case["chain_offset"] + c, R.QUANTILE_STREAM, R.QUANTILE_STRIDE, case["sweep"] * 257 + i)
            with np.errstate(all="ignore"):
                w, z, t = qo.impute_point(float(case["y"][i]), float(eta[i]), case["shift"], lambda: o.norms(rng, 1)[0],
                                          lambda: o.uniforms(rng, 1)[0])
            assert ob.out[("w", 0)] == w and ob.out[("z", 0)] == z and ob.facts["where"] == ir._where(rng)
    # the stable root against 60 digits, over the table's residuals and far into the cancelling regime
    for mu in (1e-6, 1.0, 1e6, 1e12, 1e100):
        for yy in (1e-12, 1e-3, 1.0, 9.0):
            x = float(qo.smaller_root(mu, yy))
            m, t = mpmath.mpf(mu), mpmath.mpf(mu) * mpmath.mpf(yy) / 2
            exact = m / (1 + t + mpmath.sqrt(t * (2 + t)))
            assert abs(mpmath.mpf(x) - exact) <= 4 * mpmath.mpf(math.ulp(x)), (mu, yy)


# ---- multinomial logit ---------------------------------------------------------------------------------
def test_mlogit_table_reaches_its_paths():
    comps, choices, ys, kinds = set(), set(), set(), set()
    for n in R.SIZES:
        case = R.case_of("mlogit-n%d" % n)
        choices.add(case["M"])
        assert sorted(set(case["y"])) == list(range(min(n, case["M"])))
        for c, i, ob in _facts("mlogit-n%d" % n):
            comps.update(ob.facts["comps"])
            eta = R.eta_rows(case, c)[i * case["M"]:(i + 1) * case["M"]]
            kinds.add("zero" if not eta.any() else "+700" if eta.max() > 600 else "-700" if eta.min() < -600 else "spread")
            ys.add((case["M"], int(case["y"][i])))
    assert choices == {2, 3, 16} and {0, 9} <= comps, comps
    assert kinds == {"zero", "+700", "-700", "spread"}
    assert {(16, 0), (16, 15), (2, 0), (2, 1), (3, 2)} <= ys
    ref = R.ref_of("mlogit-infbeta")
    assert all(ob.status == "impute_error" for c, i, ob in ref["facts"] if c == 2)
    assert np.all(ref["want"]["u"][2] == 0.0) and np.all(ref["want"]["w"][2] == 0.0) and ref["exact"][2].all()


def test_mlogit_functions_against_mpmath():
    rs = np.random.RandomState(5)
    for _ in range(40):
        eta = [float(v) for v in rs.normal(0, rs.choice([1.0, 30.0, 300.0]), rs.randint(2, 17))]
        exact = mpmath.log(sum(mpmath.exp(mpmath.mpf(e)) for e in eta))
        got = mo.lse(eta)
        assert abs(mpmath.mpf(got) - exact) <= 4 * mpmath.mpf(math.ulp(got)) + mpmath.mpf(2.0 ** -52), eta
        x, y = eta[0], eta[1]
        exact = mpmath.log(mpmath.exp(mpmath.mpf(x)) + mpmath.exp(mpmath.mpf(y)))
        # (x + log1p(.): the sum carries the ulp of its larger operand, whatever cancels)
        assert abs(mpmath.mpf(mo.lse2(x, y)) - exact) <= 4 * mpmath.mpf(math.ulp(max(abs(x), abs(y), 1.0)))
    for v in (-8.0, -1.06, 0.0, 0.4, 2.0, 5.09, 12.0):
        terms = [mpmath.mpf(float(mo.MIX_LOGW[c])) - (mpmath.mpf(mo.LN_SQRT_2PI) + ((mpmath.mpf(v) - mpmath.mpf(float(mo.MIX_MU[c])))
                 / mpmath.mpf(float(mo.MIX_SD[c]))) ** 2 / 2 + mpmath.mpf(float(mo.MIX_LOGSD[c]))) for c in range(10)]
        tot = sum(mpmath.exp(t) for t in terms)
        for c, got in enumerate(mo.unmix_posterior(v)):
            exact = mpmath.exp(terms[c]) / tot
            # (an exponent of size E carries E ulp of itself into the term; a term below the format's
            # range is 0, within the smallest subnormal)
            assert abs(mpmath.mpf(got) - exact) <= exact * (8 + 2 * abs(terms[c])) * mpmath.mpf(2.0 ** -52) + mpmath.mpf(5e-324), (v, c)


def test_wss_tree_against_fsum():
    """the fixed tree, restated in numpy, is a sum: within n ulp of math.fsum, fused or not; lanes
    past n add 0 and the blocks come in order"""
    for n, nch in ((1, 2), (255, 3), (257, 16), (513, 2)):
        rs = np.random.RandomState(n)
        w, u = rs.choice(mo.MIX_PREC, n * nch), rs.normal(0, 3, n * nch)
        exact = math.fsum(w * u * u)
        for fma in (True, False):
            part, total = R.wss_tree(w, u, n, nch, fma=fma)
            assert part.size == (n + 255) // 256
            assert abs(total - exact) <= n * nch * math.ulp(exact)
        blocks = [math.fsum((w * u * u)[b * 256 * nch:(b + 1) * 256 * nch]) for b in range(part.size)]
        assert all(abs(p - b) <= 256 * nch * math.ulp(b) for p, b in zip(part, blocks))   # (positive terms: n ulp)


def test_expand_cases():
    assert R.EXPAND_SHAPES == ((1, 2, 1, 0), (5, 3, 0, 2), (257, 16, 3, 1), (300, 4, 2, 2))
    for n, nch, psub, pch in R.EXPAND_SHAPES:
        Xs, Xc, X = R.expand_case(n, nch, psub, pch)
        assert X.shape == (n * nch, (nch - 1) * psub + pch)
        assert not X[0::nch, :(nch - 1) * psub].any()            # (the baseline choice has no subject columns)


# ---- sigma^2 and nu -------------------------------------------------------------------------------------
def test_sigma_nu_cases_reach_their_paths():
    cases = R.sigma_nu_cases()
    assert {cases[k]["n"] for k in cases if "-n" in k} == {1, 255, 256, 257, 1000}
    assert {cases[k]["nu_prior"][0] for k in cases} == {0, 1}
    doublings = shrinks = 0
    for tag in ("sn", "sn_ss"):
        ref = R.sigma_nu_ref(tag + "-sliceerror")
        assert list(ref["status"]) == [R.SLICE_ERROR, R.OK, R.OK]
        assert ref["chains"][0][0].out[("nu", 0)] == 0.5 and ref["chains"][0][0].out[("dx", 0)] == 1.0
        ref = R.sigma_nu_ref(tag + "-sigmamax")
        assert all("below_mode" not in ch[0].facts["path"] and ch[0].out[("sigsq", 0)] <= 0.25 for ch in ref["chains"])
        ref = R.sigma_nu_ref(tag + "-n257")
        assert all("sigma_max_infinite" in ch[0].facts["path"] for ch in ref["chains"])
        for name in cases:
            if name.startswith(tag + "-"):
                for ch in R.sigma_nu_ref(name)["chains"]:
                    if ch is not None:
                        doublings += ch[0].facts["doublings"] > 3
                        shrinks += ch[0].facts["shrinks"] > 0
        assert list(R.sigma_nu_ref(tag + "-parked")["status"]) == [R.OK, R.FORECAST_VARIANCE, R.OK]
    assert list(R.sigma_nu_ref("sn-model1025")["status"]) == [R.OK, R.MODEL_TOO_LARGE, R.OK]
    assert doublings > 10 and shrinks > 10
    case = cases["sn_ss-n1000"]
    assert not case["observed"][[0, 63, 64, 255, 256, 999]].any() and case["observed"].sum() == 994
    assert R.sigma_nu_ref("sn_ss-n1000")["chains"][0][0].facts["nobs"] == 994.0
    assert [tuple(cases[k]["trace_idx"]) for k in ("sn-trace0", "sn-trace5")] == [(0, 1, 4), (5, 4, 1)]
    assert cases["sn-n255"]["acc"] is None and cases["sn-n256"]["acc"] is not None
    assert tuple(cases["sn-n257"]["nu"]) == (0.5, 3.0, 60.0) and tuple(cases["sn-n257"]["dx"]) == (1.0, 1e-3, 1.0)


def test_sigma_nu_reference_is_the_oracles():
    """on the host's functions: the target is student_oracle.nu_log_post's to rounding, the variance
    is the oracle's gamma draw bit for bit (wsse against math.fsum), and the whole chain is
    StudentOracle's sigma^2 and nu on the same stream"""
    o = ir.oracle()
    case = R.sigma_nu_cases()["sn-n257"]
    for c in range(3):
        base = R.sigma_nu_chain(case, c)
        eta = R.eta_rows(case, c)
        r = case["y"] - eta
        wsse = math.fsum(case["w_in"][c] * r * r)
        assert abs(base.facts["wsse"] - wsse) <= 257 * math.ulp(wsse)
        rng = ir.slot_rng(case["seed"], case["chain_offset"] + c, R.SN_STREAM, R.SN_STRIDE, case["sweep"])
        sigsq = 1.0 / o.gammas(rng, (257 + case["prior_df"]) / 2, (base.facts["wsse"] + case["prior_ss"]) / 2, 1)[0]
        assert base.out[("sigsq", 0)] == sigsq
        sigma = np.sqrt(sigsq)
        u = (r / sigma) ** 2
        assert all(base.out[("u", i)] == u[i] for i in range(257))
        logf = R.nu_logf(R.HOST, case["nu_prior"], 257.0, 257 * math.log(sigma), u)
        for nu in (0.05, 0.5, 1.0, 2.0, 3.0, 60.0, 99.9, 101.0):
            a, b = logf(nu), so.nu_log_post(nu, u, 257 * np.log(sigma), case["nu_prior"])
            # the same expression but for math.lgamma against scipy's gammaln, two libraries' values of
            # the two lgammas, each taken LGAMMA_ULPS ulp of max(|lgamma|, 1) apart and multiplied by
            # n; and a handful of roundings of the largest term
            lg = max(1.0, abs(math.lgamma(0.5 * (nu + 1))), abs(math.lgamma(0.5 * nu)))
            s = float(np.sum(np.log1p(u / nu)))
            size = 257 * (2 * lg + abs(0.5 * math.log(nu * math.pi))) + abs(257 * math.log(sigma)) + 0.5 * (nu + 1) * s
            assert a == b or abs(a - b) <= 2 * R.LGAMMA_ULPS * 257 * math.ulp(lg) + 8 * math.ulp(size), (nu, a, b)
        unif = lambda: o.lib.bo_unif(C.byref(rng))             # noqa: E731
        rexp1 = lambda: 1.0 * o.lib.bo_exp_rand(C.byref(rng))  # noqa: E731
        nu, dx, mg = so.slice_draw_nu(unif, rexp1, lambda v: so.nu_log_post(v, u, 257 * np.log(sigma), case["nu_prior"]),
                                      float(case["nu"][c]), float(case["dx"][c]))
        assert abs(base.out[("nu", 0)] - nu) <= 8 * math.ulp(nu) and abs(base.out[("dx", 0)] - dx) <= 8 * math.ulp(dx)
        assert base.sig[-1] == ir._where(rng)
