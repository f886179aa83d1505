"""The references and bounds of tests/big_ref.py, checked without a GPU: plain f64 numpy
(numpy.linalg.cholesky, f64 forward substitution, the formulas in f64) stays inside every bound
the GPU test (test_big_kernel_probe_gpu.py) holds the large-model kernel to, on every case; the
Python restatements of the two layouts agree with a hand count; and the cases have the lanes the
GPU test is written for."""
import numpy as np
import pytest

import big_ref as R
import fill_ref as F


def test_layouts_agree_with_a_hand_count():
    # capacity 128: 16 block rows -> 136 blocks of 64 doubles per factor
    S = F.layout(128)
    assert S["Lv"] == 0 and S["La"] == 8704 and S["rdv"] == 17408 and S["rda"] == 17536
    assert S["w"] == 17664 and S["bg"] == 17792 and S["g"] == 17920 and S["scal"] == 17984
    assert S["iv"] == 17992 and S["ia"] == 20040 and S["total"] == 22088
    # p = 1100, capacity 256: tile 18432, rdt 512, four k-vectors of 2048, control 512, two lists of
    # 512, six permutation arrays of 2208 ((1101 * 2 + 15) & ~15), three byte vectors of 1104
    L = R.big_lds_layout(1100, 256)
    assert L["tile"] == 0 and L["rdt"] == 18432 and L["w"] == 18944 and L["y"] == 20992 and L["rd"] == 23040
    assert L["bst"] == 25088 and L["ctrl"] == 27136 and L["g"] == 27648 and L["gst"] == 28160
    assert L["perm0"] == 28672 and L["perm1"] == 30880 and L["oth"] == 33088 and L["last"] == 35296
    assert L["pred"] == 39712 and L["gam"] == 41920 and L["gam0"] == 43024 and L["nbr"] == 44128
    assert L["total"] == 45232
    assert R.big_lds_layout(R.P_BIG, 1024)["total"] <= 160 * 1024


def test_packing_round_trip():
    rng = np.random.default_rng(3)
    L = np.tril(rng.standard_normal((21, 21)))
    buf = np.full(F.bidx(23, 23) + 1, np.nan)
    R.pack_into(buf, L)
    assert np.array_equal(R.unpack(buf, 21), L)
    for m, n in ((0, 0), (7, 3), (8, 0), (20, 19)):
        assert buf[F.bidx(m, n)] == L[m, n]


def test_exact_gram_is_exact():
    rng = np.random.default_rng(5)
    L = np.tril(rng.standard_normal((40, 40))) * np.exp(rng.uniform(-8, 1, (40, 40)))
    G, left = R.gram_exact(L)
    want = L.astype(R.LD) @ L.astype(R.LD).T
    assert float(np.abs(G - want).max()) <= left + 40 * 2.0 ** -63 * float(np.abs(want).max())


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("kcap,k", R.BUILD_CASES)
def test_f64_numpy_build_is_inside_every_bound(kcap, k, kind):
    c = R.build_case(k, kind)
    assert c["b"][c["g"][-1]] != 0.0 and np.count_nonzero(c["b"]) == min(3, len({0, k // 2, k - 1}))
    assert c["sx"] != 1.0 and k <= kcap == R.kcap_of(k)
    ratios = R.check_build(c, R.numpy_build(c))
    print(f"k={k} {kind}: " + " ".join(f"{n} {v:.3g}" for n, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("kcap,k", R.MODE1_CASES)
def test_f64_numpy_build_in_mode_1(kcap, k):
    c = R.build_case(k, "ill", 1)
    ratios = R.check_build(c, R.numpy_build(c))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("kcap,k", R.SOLVE_CASES)
def test_f64_numpy_solve_is_inside_its_bound(kcap, k):
    c = F.case(R.P_BIG, k, "ill")
    ref = F.reference(R.P_BIG, k, "ill", 0)
    for L, B, X in ((c["Lv"], ref["bv"], ref["xv"]), (c["La"], ref["ba"], ref["xa"])):
        got = F.forward(L, B, np.float64)
        err = np.linalg.norm((got.astype(R.LD) - X).astype(np.float64), axis=0)
        bound = R.solve_bounds(L, X)
        live = bound > 0
        assert np.all(err[~live] == 0.0) and np.all(err[live] <= bound[live])
        assert R.solve_residual_ratio(L, B, got) <= 1.0


@pytest.mark.parametrize("kcap,k", R.EVAL_CASES + [(128, 1)])
def test_eval_windows_hold_the_lanes_the_gpu_test_needs_and_f64_numpy_is_inside_the_bound(kcap, k):
    c = R.eval_case(k)
    for jbase in R.eval_windows(k):
        want, bound, kind = R.eval_reference(c, jbase)
        assert kind.count("add") >= 1, (k, jbase)
        if k > 1:
            assert kind.count("drop") >= 1 and kind.count("slow") >= 1, (k, jbase)
        assert kind.count("none") == (52 if jbase == 1088 else 0)
        got = R.numpy_eval(c, jbase)
        fast = np.array([x in ("add", "drop", "empty") for x in kind])
        assert np.all(np.isfinite(want[fast].astype(np.float64)))
        assert np.all(np.abs(got[fast].astype(R.LD) - want[fast]) <= bound[fast])
        assert np.all(got[~fast] == -np.inf)
    if k == 1024:
        kinds = R.eval_reference(c, 1024)[2]
        assert kinds.count("add") == 4 and kinds.count("drop") == 53


@pytest.mark.parametrize("k", (65, 129))
def test_the_special_lane_cases_have_their_lanes(k):
    """window 0 of the two sizes the GPU test's special lanes run at: an add and a drop to kill under
    the prior; with SS = 1 for the current model, adds whose SS' is negative by more than its bound
    and drops that stay fast; the third included variable's column to copy"""
    c = R.eval_case(k)
    kind = R.eval_reference(c, 0)[2]
    assert "add" in kind and "drop" in kind and len(c["g"]) > 3
    assert R.copy_lane_verdict(c, kind.index("add"), 3) in ("notpd", "dead")
    small = dict(c, ss0q=float(c["model"][4] - c["model"][5] + 1.0))
    want, bound, kind = R.eval_reference(small, 0)
    assert any(kd == "bad" and abs(want[x]) > bound[x] for x, kd in enumerate(kind)) and "drop" in kind
    f64 = R.numpy_build(R.build_case(200, "well"))
    assert f64["Q"] - f64["c"] > 1.0        # the build's negative-SS verdict at ss0q = 1e-3


def test_the_model_of_one_variable_has_its_drop_in_the_first_window():
    c = R.eval_case(1)
    kind = R.eval_reference(c, 512)[2]
    assert kind[int(c["g"][0]) - 512] == "empty"


def test_a_hip_error_latches_the_loader():
    """a probe call that returns a hipError_t raises ProbeHipError, and every later call raises without
    calling anything"""
    import big_probe_lib as P
    calls = []

    def call(a):
        calls.append(1)
        return 700
    assert not P.FAULTED
    try:
        with pytest.raises(P.ProbeHipError):
            P._twice(call, lambda: (np.zeros(1),))
        assert P.FAULTED and len(calls) == 1
        with pytest.raises(P.ProbeHipError):
            P._twice(call, lambda: (np.zeros(1),))
        assert len(calls) == 1
        with pytest.raises(AssertionError):
            P.FAULTED = False
            P._twice(lambda a: -1, lambda: (np.zeros(1),))      # a refused request is no HIP error
    finally:
        P.FAULTED = False
