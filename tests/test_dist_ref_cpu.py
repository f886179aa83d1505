"""The references of tests/dist_ref.py, pinned without a GPU, on every case of
tests/test_dist_samplers_gpu.py:

  * with replay = None a restatement IS the oracle's function -- bo_rgamma, bo_rtrun_gamma (and the
    variance draw around them), bo_rtrun_norm_2, bo_runif, bo_norm_rand, bo_exp_rand -- bit for bit,
    with the same stream position and the same status (the rule imputer_ref.pg_obs follows for
    bo_test_rpg; the oracle's functions are pinned on the compiled reference's goldens);
  * every case reaches the branches it is listed for in at least 16 draws that are compared by value,
    and every branch the samplers have is listed by some case or named below as one the reference
    reaches at no input tried;
  * at most 0.5 % of a case's draws are set aside (their replays disagree), but for the one case named
    loose -- all from the reference alone."""
import numpy as np
import pytest

import dist_ref as dr

CASES = list(dr.cases())
# (d_rtrun_exp's restatement is imputer_ref's, pinned there through bo_rtrun_norm; the oracle does not
# export its own)
PINNED = [n for n in CASES if dr.cases()[n]["fn"] != "rtrun_exp"]


@pytest.mark.parametrize("name", PINNED)
def test_restatement_is_the_oracle(name):
    case, ref = dr.cases()[name], dr.ref_of(name)
    for i in range(case["n"]):
        x, where, failed = dr.oracle_draw(case["fn"], case["args"][i], case["seed"], case["chain"], case["index0"] + i,
                                          case["slot_limit"])
        assert failed == (ref["status"][i] != 0), (name, i)
        assert where == (int(ref["stream"][i]), int(ref["pos"][i])), (name, i)
        if not failed:
            assert np.float64(x).tobytes() == np.float64(ref["want"][i]).tobytes(), (name, i, x, ref["want"][i])


@pytest.mark.parametrize("name", CASES)
def test_listed_branches_are_reached(name):
    case, counts = dr.cases()[name], dr.reached(name)
    short = {a: counts.get(a, 0) for a in case["listed"] if counts.get(a, 0) < dr.MIN_COMPARED}
    assert not short, (name, short)


@pytest.mark.parametrize("name", CASES)
def test_set_aside_cap(name):
    case, ref = dr.cases()[name], dr.ref_of(name)
    aside = int((~ref["same"]).sum())
    if case["loose"]:
        assert name == "tn2-tail-1e-9"
        # the loose half is exactly the rows 3 and 8 sigma from the mean; the rest is compared
        # (dist_ref._window_rows: offsets 0.1, 3, 8, 30 sigma, each above and below the mean)
        far = np.array([i % 8 in (2, 3, 4, 5) for i in range(case["n"])])
        assert np.array_equal(~ref["same"], far)
        return
    assert aside <= dr.SET_ASIDE_CAP * case["n"], (name, aside)


def test_spill_cases_spill():
    for name, case in dr.cases().items():
        spilled = int((dr.ref_of(name)["stream"] & np.uint64(0x80000000) != 0).sum())
        if case["slot_limit"]:
            assert spilled >= dr.MIN_COMPARED, name
        else:
            assert spilled == 0, name
    # one case per sampler that reads more than one number
    fns = {case["fn"] for case in dr.cases().values() if case["slot_limit"]}
    assert fns == {"rgamma_scale", "draw_variance", "rtrun_norm_2", "norm_rand", "exp_rand"}


# the branches the samplers have, by the names dist_ref's paths give them
NAMED = {"small_exp", "small_pow", "small_reject", "gs_high", "gs_low", "gs_reject", "gd_immediate", "gd_squeeze",
         "gd_quotient", "quotient_v_small", "quotient_v_large", "loop_round", "loop_once", "loop_three_or_more",
         "loop_retry", "loop_v_small", "loop_v_large", "coef_low", "coef_mid", "coef_high", "sigma_max_zero",
         "sigma_max_infinite", "below_mode", "below_mode_reject", "ars_at_mode", "ars_one_point", "ars_grown", "ars_tail",
         "ars_inner", "slice", "slice_newton", "slice_newton_gave_up", "slice_first_point", "wide", "wide_round", "narrow",
         "narrow_round", "tail_above", "tail_below", "tn2_two_points", "tn2_grown", "tn2_exp", "tn2_uniform",
         "trun_exp_point", "trun_exp_draw", "runif_point"}
# ... and those the reference reaches in no draw of any case (nor at the other inputs tried while the
# cases were chosen: hulls of the gamma tail stay under 10 points and of the two-sided normal under 6,
# no candidate leaves [x0, x_last], GS never returns 0, the slice sampler's first point is always
# inside the slice).  Should a change of the cases reach one, it has to be listed.
UNREACHED = {"ars_cap", "tn2_cap", "tn2_left_the_hull", "tn2_past_cdf", "gs_zero", "slice_shrink", "slice_gave_up"}


def test_every_branch_is_listed_by_some_case():
    listed = set()
    for case in dr.cases().values():
        listed |= set(case["listed"])
    assert NAMED <= listed, NAMED - listed


def test_unreached_branches_and_hull_sizes():
    seen, ars, tn2 = set(), 0, 0
    for name, case in dr.cases().items():
        ref = dr.ref_of(name)
        for names in ref["arms"]:
            seen |= names
        if case["fn"] == "draw_variance":
            ars = max(ars, int(ref["hull"].max()))
        if case["fn"] == "rtrun_norm_2":
            tn2 = max(tn2, int(ref["hull"].max()))
    assert not seen & UNREACHED, seen & UNREACHED
    print("largest hull at acceptance: gamma tail %d points, two-sided normal %d points" % (ars, tn2))
    # (the device's two-sided hull holds 63 points, the oracle's 64: no case comes near either)
    assert 2 <= ars < 16 and 2 <= tn2 < 16 and tn2 < dr.TN2_CAP_DEVICE


def test_status_cases():
    ref = dr.ref_of("variance-at-mode")
    assert np.all(ref["status"] == dr.BAD_ARS) and np.all(ref["pos"] == np.uint64(dr.STRIDE) * (np.arange(64, dtype=np.uint64) + np.uint64(3)))
    ref = dr.ref_of("variance-zero")
    assert np.all(ref["want"] == 0.0) and np.all(ref["pos"] == np.uint64(dr.STRIDE) * (np.arange(64, dtype=np.uint64) + np.uint64(3)))
    case, ref = dr.cases()["runif"], dr.ref_of("runif")
    for i, a in enumerate(case["args"]):
        if a[0] == a[1]:                      # no number read
            assert int(ref["pos"][i]) == dr.STRIDE * (case["index0"] + i)
            assert np.float64(ref["want"][i]).tobytes() == np.float64(a[0]).tobytes()


def test_chained_draws_reach_every_branch():
    """2^18 consecutive draws of one stream: every branch of d_norm_rand and d_exp_rand hundreds of times"""
    counts = dr.norm_rand_branches()
    print(counts)
    assert all(v >= 200 for v in counts.values()), counts
    counts = dr.exp_rand_branches()
    print(counts)
    assert all(v >= 200 for v in counts.values()), counts
    x, pos = dr.chained_ref("norm_rand")
    assert np.all(np.isfinite(x)) and np.all(np.diff(pos.astype(np.int64)) >= 2)


def test_random_int_rows():
    L = dr.lib()
    for j, (lo, hi) in enumerate(dr.INT_ROWS):
        x, where, failed = dr.oracle_draw("random_int", (lo, hi), dr.SEEDS[0], dr.CHAINS[1], 100 + j)
        assert not failed and lo <= x <= hi and where == (dr.STREAM, dr.STRIDE * (100 + j) + 1)
    assert L is not None
