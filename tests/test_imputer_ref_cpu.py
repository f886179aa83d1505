"""The references of tests/imputer_ref.py, pinned without a GPU: the Python restatement of
TnSampler on the oracle's bo_rtrun_norm (same stream, equal values) and on the compiled
reference's truncated-normal draws (tests/golden/kat_trun_norm.npz), the Polya-Gamma moments on
bo_test_rpg -- and, for every case the GPU test runs, the conditions on its inputs: no replay of
any observation takes another branch than the unperturbed run, every recorded margin is above
1e-9, every output is finite, and each table reaches the paths it is there for."""
import ctypes as C

import numpy as np
import pytest

import imputer_ref as R
from test_oracle_golden import load

MARGIN = 1e-9


def test_tn_sampler_restatement_matches_reference_draws():
    o = R.oracle()
    g = load("kat_trun_norm")
    hulls = []
    for (mu, sg, cut, ab), want in zip(g["cases"], g["draws"]):
        rng, tr = o.rng_mt(int(g["seed"])), R.Trace()
        got = np.array([R.rtrun_norm(o.lib, R.HOST, rng, float(mu), float(sg), float(cut), int(ab), tr)
                        for _ in range(want.shape[0])])
        assert np.array_equal(got, want), (mu, sg, cut, ab)
        hulls += tr.hulls
    assert max(hulls) >= 5          # (the adaptive sampler ran, and rejected)


@pytest.mark.parametrize("a", [30.0, 2.5, 0.3, 1e-3, 1e-9, 1e-12, 1e-15])
def test_tn_sampler_restatement_matches_oracle_on_the_same_stream(a):
    o = R.oracle()
    L = o.lib
    for gt in (1, 0):
        for i in range(40):
            r1 = R.slot_rng(7, 2, R.PROBIT_STREAM, R.PROBIT_STRIDE, 1000 + i)
            r2, st, tr = R._copy(r1), C.c_int(0), R.Trace()
            mu = -a if gt else a
            want = L.bo_rtrun_norm(C.byref(r1), mu, 1.0, 0.0, gt, C.byref(st))
            got = R.rtrun_norm(L, R.HOST, r2, mu, 1.0, 0.0, gt, tr)
            assert st.value == 0 and got == want and R._where(r1) == R._where(r2)
            assert len(tr.hulls) == 1 and 1 <= tr.hulls[0] <= R.HULL_CAP


def test_pg_restatement_matches_oracle():
    L = R.oracle().lib
    for nt in (1, 3, 5, 6, 40, 1000):
        for eta in R.PG_ETA + [9.9e-5, 1.0e-4, 0.3, 7.0]:
            for i in range(8):
                got = R.pg_obs(11, 3, 2, i, 50, eta, 1, nt, 5)
                rng, st = R.slot_rng(11, 3, R.PG_STREAM, R.PG_STRIDE, 2 * 50 + i), C.c_int(0)
                want = L.bo_test_rpg(C.byref(rng), nt, eta, 5, C.byref(st))
                assert st.value == 0 and got.out["w"] == want and got.sig[1] == R._where(rng)


def test_math_table_moves_results_by_whole_ulps():
    import math
    seen = set()
    for replay in range(R.REPLAYS):
        M = R.MathTable(replay)
        for k in range(100):
            x = 0.1 + 0.01 * k
            for name, U in R.ULPS.items():
                v, real = getattr(M, name)(x), getattr(math, name)(x)
                steps = round((v - real) / math.ulp(real))
                assert abs(steps) <= U and v == real + steps * math.ulp(real) and v == getattr(M, name)(x)
                seen.add((name, steps))
            assert abs(M.fused(x) - x) <= R.FUSED_ULPS * math.ulp(x)
    assert all((name, s) in seen for name, U in R.ULPS.items() for s in (-U, U))
    assert R.HOST.exp(1.25) == math.exp(1.25) and R.HOST.fused(1.25) == 1.25


@pytest.mark.parametrize("name", R.case_names())
def test_case_conditions(name):
    """no replay takes another branch, margins above 1e-9, finite outputs"""
    case = R.case_of(name)
    ref = R.ref_of(name)
    assert ref["same"], "a replay took another branch"
    # (only tiny24 may hold observations without a reference value, and only among its 24)
    assert not ref["loose"][:, 24 if name == "probit-tiny24" else 0:].any()
    assert ref["margin"] > MARGIN, ref["margin"]
    for k, v in ref["want"].items():
        assert np.all(np.isfinite(v[ref["written"]])), k
        assert np.all(np.isfinite(ref["bound"][k])) and np.all(ref["bound"][k][ref["written"] & ~ref["exact"]] > 0), k
    for c in range(case["chains"]):
        assert np.all(np.isfinite(R.case_eta(case, c)))


def _routes(name):
    return R.ref_of(name)["routes"]


def _hulls(name, c):
    return [(i, ob.facts["hulls"]) for cc, i, ob in R.ref_of(name)["facts"] if cc == c]


def test_probit_paths_are_reached():
    for name in ("probit-n257", "probit-n513", "probit-clt5"):
        assert {"hit", "miss_u1", "miss_cut", "far", "queued"} <= set(_routes(name)), name
    # the fast path is off at clt_threshold 0 and where a slot serves one uniform
    for name in ("probit-clt0", "probit-slot1"):
        assert not {"hit", "miss_u1", "miss_cut"} & set(_routes(name)), name
    for name in ("probit-slot2", "probit-slot6"):
        assert {"hit", "miss_u1", "miss_cut"} <= set(_routes(name)), name
    assert _routes("probit-near256") == ["queued"] * (256 * R.CHAINS)           # > 192: wave 0's second chunk
    assert _routes("probit-far256") == ["far"] * (256 * R.CHAINS)               # four rounds of 64
    # the coefficients' memory becomes the hulls: far-side observations under a 1024-variable model
    assert _routes("probit-model1024").count("far") >= 3 * R.CHAINS
    # every kind of observation of the table, on either side
    case = R.case_of("probit-n257")
    for c in range(R.CHAINS):
        eta = R.case_eta(case, c)
        seen = {(int(case["nt"][i]), int(case["y"][i]), float(np.sign(eta[i]))) for i in range(257)}
        assert {(nt, y, s) for nt, y in R.PROBIT_OBS for s in (-1.0, 1.0)} <= seen
        assert np.abs(eta).max() == 30.0


def test_probit_phase_three_is_reached():
    """of the 24 observations a hair on the far side at least 9 per chain need more than 16 and at
    most 64 hull points: phase (3) in three rounds of four, more than 4 overflows of phase (2)"""
    case = R.case_of("probit-tiny24")
    assert case["n"] <= 256                       # (one workgroup)
    largest = 0
    for c in range(R.CHAINS):
        tiny = [h[0] for i, h in _hulls("probit-tiny24", c) if i < 24]
        assert len(tiny) == 24 and all(len(h) == 1 for i, h in _hulls("probit-tiny24", c) if i < 24)
        again = [h for h in tiny if 16 < h <= 64]
        assert len(again) >= 9, (c, tiny)
        assert max(tiny) <= 64
        largest = max(largest, max(tiny))
        eta = R.case_eta(case, c)[:24]
        assert np.all((np.abs(eta) <= 1e-12) & (np.abs(eta) >= 1e-15))   # (see probit_cases)
    print("largest hull of probit-tiny24:", largest)


def test_probit_phase_three_case_has_a_reference():
    """the case whose phase (3) values are compared: per chain at least 9 observations -- in one
    workgroup, with 64 far-side observations or more so that phase (2) runs in rounds -- whose hull
    needs more than 16 and at most 64 points, every one with the same branches in all replays
    (test_case_conditions) and none without a reference value"""
    case, ref = R.case_of("probit-phase3"), R.ref_of("probit-phase3")
    assert case["n"] == 256 and ref["routes"] == ["far"] * (256 * R.CHAINS)
    assert ref["same"] and not ref["loose"].any() and ref["written"].all() and ref["margin"] > MARGIN
    sizes = []
    for c in range(R.CHAINS):
        hulls = dict(_hulls("probit-phase3", c))
        again = {i: hulls[i][0] for i in range(256) if 16 < hulls[i][0] <= 64}
        assert set(again) == set(R.PHASE3[c]) and len(again) >= 9, (c, again)
        assert all(len(h) == 1 and h[0] <= 64 for h in hulls.values())
        eta = R.case_eta(case, c)
        assert all(abs(eta[i]) == a for i, a in R.PHASE3[c].items())
        sizes += again.values()
    print("hulls of probit-phase3 redone in phase (3):", sorted(sizes))


def test_contracting_the_hull_integrals_exponent_changes_the_draw():
    """The expression a phase (3) draw hangs on.  With update_cdf's exponent y - d z + d knot
    rounded once per multiply-add (Fused(["integral"]): what a contracting compiler makes of it)
    an observation of probit-phase3 takes 19 hull points instead of 17 and gives another value
    -- bit for bit the one the kernel gave before its exponent was kept from being contracted;
    the other fusable expressions of the sampler leave the draw where it is"""
    case = R.case_of("probit-phase3")
    c, i = 2, 68
    eta = float(R.case_eta(case, c)[i])
    host = R._obs_of(case, c, i, eta)
    assert host.facts["hulls"] == [17] and host.out["z"] == -0.18208490171121036
    fused = R._obs_of(case, c, i, eta, R.Fused(["integral"]))
    assert fused.facts["hulls"] == [19] and fused.out["z"] == -0.18689263925262276
    others = R._obs_of(case, c, i, eta, R.Fused(["trun_exp", "candidate", "hull", "knot"]))
    assert others.facts["hulls"] == [17] and others.out["z"] == host.out["z"]


def test_probit_overflow_observation():
    """an observation for which the oracle itself reports BO_ERR_UNSUPPORTED_RNG_BRANCH -- a hull
    of more than 64 points --, the same in every replay, alone in its chain"""
    usable, degenerate = R.overflow_search()
    assert usable, "no hull of more than 64 points below a = 1e-15 (%d degenerate ones)" % len(degenerate)
    a, at = usable[0]
    assert a < 1e-15
    ref = R.ref_of("probit-overflow")
    assert list(ref["status"]) == [R.OK, R.RNG_BRANCH, R.OK]
    assert [(c, i) for c, i, ob in ref["facts"] if ob.status == "rng_branch"] == [(1, at)]
    assert ref["written"].sum() == 3 * 64 - 1


def test_logit_binomial_paths_are_reached():
    case = R.case_of("logit-n257")
    total = dict(inversion=0, btpe=0, pp_high=0, early=0)
    for c in range(R.CHAINS):
        eta = R.case_eta(case, c)
        for i in range(257):
            if case["nt"][i] > case["clt"]:
                f = R.logit_binomial_facts(case["seed"], case["chain_offset"] + c, case["sweep"], i, 257, float(eta[i]),
                                           case["y"][i], case["nt"][i], case["clt"])
                for k in total:
                    total[k] += f[k]
    print("logit-n257 binomial draws:", total)
    assert all(v >= 1 for v in total.values()), total
    assert sum(ob.facts["btpe"] for _, _, ob in R.ref_of("logit-n257")["facts"]) == total["btpe"]
    seen = {(int(case["nt"][i]), int(case["y"][i]), float(R.case_eta(case, 0)[i])) for i in range(257)}
    assert {(nt, y, e) for nt, y in R.LOGIT_OBS for e in R.LOGIT_ETA} <= seen


def test_logit_ss_missing_steps_and_stride():
    case, ref = R.case_of("logit_ss-n257"), R.ref_of("logit_ss-n257")
    assert case["offset_stride"] > case["n"] and 0 < ref["exact"].sum() < ref["written"].sum()
    assert np.all(ref["want"]["h"][ref["exact"]] == R.slo.MISSING_VARIANCE)


def test_pg_arms_are_reached():
    ref, case = R.ref_of("pg-n257"), R.case_of("pg-n257")
    arms = [ob.facts["arm"] for _, _, ob in ref["facts"]]
    assert {"sum", "series", "moments"} <= set(arms)
    eta = np.abs(R.case_eta(case, 0))
    small, large = case["nt"] <= case["clt"], case["nt"] > case["clt"]
    assert {0.0, 1.0, 3.125, 3.2, 20.0} <= set(eta[small]) and {0.0, 5e-5, 2e-4, 3.0} <= set(eta[large])
    # the proposal's exponential tail and both arms of pg_rtigauss, counted per |eta|: the arm of
    # exponentials below z = |eta| / 2 = 1 / t, the arm of normals from z = 1 / t on (3.125 is
    # the boundary itself, and takes the arm of normals)
    assert 0.5 * 3.125 == 1.0 / 0.64
    seen = {}
    for c, i, ob in ref["facts"]:
        seen.setdefault(abs(float(R.case_eta(case, c)[i])), set()).update(ob.facts["arms"])
    for e in (0.0, 1.0):
        assert {"tail", "tigauss_exp"} <= seen[e] and "tigauss_normal" not in seen[e], (e, seen[e])
    for e in (3.125, 3.2, 20.0):
        assert "tigauss_normal" in seen[e] and "tigauss_exp" not in seen[e], (e, seen[e])
    print("pg-n257 arms by |eta|:", {e: sorted(a) for e, a in seen.items() if a})


def test_poisson_no_last_event_at_the_end_of_the_interval():
    """The kernel's `delta == 0` arm needs a beta draw of exactly 1.  Cheng's BC returns
    w / (1 + w) with w = y u1 / (1 - u1): 1.0 only where u1 is within about y 2^-53 of 1, one draw
    in 1e14 at the table's largest count.  A bounded search -- every count of the cases, 4000
    slots each -- finds none, so the arm has no case"""
    L = R.oracle().lib
    _, counts = R.poisson_table()
    largest = 0.0
    for y in counts[1:]:
        for i in range(4000):
            rng = R.slot_rng(R.SEED, R.CHAIN_OFFSET, R.POISSON_STREAM, R.POISSON_STRIDE, i)
            largest = max(largest, L.bo_test_rbeta_a1(C.byref(rng), float(y)))
    assert largest < 1.0
    print("largest beta draw of the search: 1 - %.3g" % (1.0 - largest))


def test_poisson_arms_are_reached():
    _, counts = R.poisson_table()
    for kind in ("poisson", "poisson_ss"):
        case = R.case_of(kind + "-n513")
        eta = R.case_eta(case, 0)
        live = np.ones(513, bool) if kind == "poisson" else case["observed"].astype(bool)
        seen = {(int(case["y"][i]), float(case["nt"][i]), float(eta[i])) for i in range(513) if live[i]}
        assert {(y, ex, e) for y in counts for ex in R.POISSON_EXPOSURE for e in R.POISSON_ETA} <= seen
        assert np.all(case["obs_mix"][case["y"] == counts[-1]] == -1) and np.all(case["obs_mix"][case["y"] == counts[-2]] >= 0)
