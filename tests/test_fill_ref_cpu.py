"""The reference and the cases of tests/test_fill_mfma_gpu.py, pinned without a GPU
(tests/fill_ref.py): the longdouble substitution solves its systems to rounding, the cases are
what they claim to be (condition numbers, a mix of all four kinds of lane in every window),
and -- so that the inputs, not the kernel, are shown to fit the GPU test's tolerance -- a plain
f64 forward substitution and an f64 emulation of the device's blocked order (inverse diagonal
blocks by substitution with the reciprocal diagonal, X_I = inv(L_II)(B_I - sum L_IJ X_J)) both
stay inside it for every case."""
import numpy as np
import pytest

import fill_ref as R

CASES = sorted({(k, kind) for _, _, k in R.SUMS_CASES for kind in R.KINDS})


def test_layout_and_block_rows():
    S = R.layout(48)
    assert S["Lv"] == 0 and S["La"] == 21 * 64 and S["rdv"] == 2 * 21 * 64 and S["total"] % 8 == 0
    assert S["ia"] - S["iv"] == 48 * 16 and S["total"] >= S["ia"] + 48 * 16
    assert [R.block_rows(k) for k in (1, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 128)] == \
        [2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 8, 8]
    seen = {R.bidx(m, n) for m in range(128) for n in range(m + 1)}
    assert len(seen) == 128 * 129 // 2 and max(seen) < 16 * 17 // 2 * 64


@pytest.mark.parametrize("k,kind", CASES)
def test_condition_numbers_are_what_the_cases_claim(k, kind):
    for p in (R.P_FULL, R.P_ODD):
        c = R.case(p, k, kind)
        assert np.array_equal(c["Lv"], np.tril(c["Lv"])) and np.all(np.diag(c["Lv"]) > 0)
        if kind == "well":
            assert c["kv"] < 30 and c["ka"] < 30
        elif k >= 7:       # (a 1 x 1 factor has condition number 1 whatever the matrix)
            assert 1e2 < c["kv"] < 1e4 and 1e2 < c["ka"] < 1e4


@pytest.mark.parametrize("p,jbase", R.WINDOWS)
def test_every_window_mixes_the_kinds_of_lane(p, jbase):
    for k in (9, 48, 65, 128):
        c = R.case(p, k, "well")
        fl = R.flags(c, jbase)
        live = np.arange(64) + jbase < p
        assert np.all(fl[~live] == 0)
        assert (p == R.P_ODD) == bool(np.any(~live))          # the odd p's window overruns it
        kinds = {int(f) for f in fl[live]}
        assert {R.FAST, R.FAST | R.ADD} <= kinds                # fast drops and fast adds
        assert kinds & {0, R.ADD}                               # and proposals that are not fast
    c = R.case(R.P_FULL, 41, "ill")
    assert R.flags(c, 0)[c["g"][0]] == R.FAST                   # the first variable's drop is fast


@pytest.mark.parametrize("k,kind", CASES)
def test_reference_solves_its_systems_and_f64_orders_fit_the_tolerance(k, kind):
    for p, jbase in R.WINDOWS:
        c = R.case(p, k, kind)
        ref = R.reference(p, k, kind, jbase)
        fast = (ref["flags"] & R.FAST) != 0
        assert fast.any()
        for L, B, X in ((c["Lv"], ref["bv"], ref["xv"]), (c["La"], ref["ba"], ref["xa"])):
            # residual of the longdouble solution at longdouble's rounding level
            Ll = L.astype(R.LD)
            res = np.abs(Ll @ X - B).max(0)
            bound = 4 * k * np.finfo(R.LD).eps * (np.abs(Ll) @ np.abs(X)).max(0)
            assert np.all(res <= bound)
        tol = R.tolerances(c, ref)
        for solve in (lambda L, B: R.forward(L, B, np.float64), lambda L, B: R.blocked(L, B, k)):
            xv, xa = solve(c["Lv"], ref["bv"]), solve(c["La"], ref["ba"])
            got = R.sums(xv, xa, ref["ba"], c["w"], c["bg"])
            for s in range(4):
                err = np.abs(got[s].astype(R.LD) - ref["sums"][s]).astype(np.float64)
                assert np.all(err[fast] <= tol[s][fast]), (s, (err[fast] / tol[s][fast]).max())


@pytest.mark.parametrize("k,kind", [(7, "well"), (17, "ill"), (41, "ill"), (113, "ill")])
def test_inverse_blocks_in_device_order_fit_their_tolerance(k, kind):
    c = R.case(R.P_FULL, k, kind)
    for L in (c["Lv"], c["La"]):
        exact = R.exact_inverse_blocks(L, k)
        got = R.diag_inverse_blocks(L, k, R.block_rows(k))
        for I in range(R.block_rows(k)):
            o = 16 * I
            kk = min(max(k - o, 0), 16)
            assert np.all(got[I][kk:] == 0) and np.all(got[I][:, kk:] == 0) and np.all(np.triu(got[I], 1) == 0)
            if kk:
                kap = np.linalg.cond(L[o:o + kk, o:o + kk])
                err = np.abs(got[I].astype(R.LD) - exact[I]).max()
                assert err <= 16 * R.U * kap * np.abs(exact[I]).max()


def test_block_holds_what_the_product_leaves_and_nan_elsewhere():
    c = R.case(R.P_FULL, 41, "well")
    S, b = R.layout(48), R.block(c, 48)
    assert b[S["Lv"] + R.bidx(40, 3)] == c["Lv"][40, 3]
    assert all(b[S["La"] + R.bidx(m, n)] == 0.0 for m in range(41, 48) for n in range(m + 1))   # kpad8 = 48
    assert np.isnan(b[S["Lv"] + R.bidx(8, 8) + 1])              # above a diagonal block's diagonal
    assert np.all(b[S["rdv"] + 41:S["rdv"] + 48] == 0.0)
    assert np.all(np.isnan(b[S["w"] + 41:S["bg"]])) and np.all(np.isnan(b[S["iv"]:]))
    z = R.block(c, 48, zero_pad=True)
    assert np.all(z[S["w"] + 41:S["w"] + 48] == 0.0) and np.all(z[S["bg"] + 41:S["bg"] + 48] == 0.0)
    c9 = R.case(R.P_FULL, 9, "well")
    b9 = R.block(c9, 48)
    assert np.isnan(b9[S["Lv"] + R.bidx(16, 0)]) and np.isnan(b9[S["rdv"] + 16])   # rows >= kpad8 = 16
