"""The large-model kernel's pieces (boom_amd/csrc/ssvs_big_kernel.hip) launched directly through
tests/cpp/big_probe.hip and held to the bounds of tests/big_ref.py: the 64 x 64 tile
factorisations, big_solve, big_build_body with one wavefront and with two, a REUSE rebuild,
the build's verdicts, and big_eval's fast and special lanes.  The conditions on the cases are
asserted on the CPU (test_big_ref_cpu.py)."""
import numpy as np
import pytest

import big_probe_lib as P
import big_ref as R
import fill_ref as F

pytestmark = pytest.mark.gpu

NINF = -np.inf
CHAIN_NEGATIVE_SS = 2


@pytest.fixture(scope="module")
def lib():
    return P.load()


@pytest.fixture(autouse=True)
def _stop_after_a_hip_error():
    """a probe call that returned a HIP error has latched big_probe_lib.FAULTED: the session ends
    before the next test starts anything on that device"""
    if P.FAULTED:
        pytest.exit("a probe call returned a HIP error", returncode=3)
    yield


def _is_sentinel(a):
    return a.view(np.uint64) == P.SENT_BITS


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_layouts_are_the_products(lib):
    for kcap in (128, 256, 512, 1024):
        S, want = P.layout(lib, kcap), F.layout(kcap)
        assert {n: S[n] for n in want} == want
        assert P.lds_layout(lib, R.P_BIG, kcap) == R.big_lds_layout(R.P_BIG, kcap)


def test_bad_requests_are_refused_on_the_host(lib):
    c = R.build_case(65, "well")
    with pytest.raises(AssertionError):
        P.build(lib, 3, 0, c, 128)                      # no such wave count
    with pytest.raises(AssertionError):
        P.build(lib, 1, 0, R.build_case(129, "well"), 128)   # more variables than the capacity
    with pytest.raises(AssertionError):
        P.build(lib, 1, 0, c, 96)                       # not a capacity of the product's
    e = R.eval_case(65)
    with pytest.raises(AssertionError):
        P.evaluate(lib, e, 128, R.block(e, 128), 32)    # a window that is no multiple of 64
    with pytest.raises(AssertionError):
        P.evaluate(lib, e, 128, R.block(e, 128), 0, g=e["g"][::-1].copy())


# ---- tiles --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("kk", R.TILE_KK)
def test_tile_in_registers_is_bitwise_the_tile_in_lds(lib, kk, kind):
    """chol_tile_regs' header: "the factor is bitwise chol_tile's" -- lower triangle, rd, ok and the
    log-determinant sum; and the factor is inside Higham's bound"""
    M = R.tile_input(kk, kind)
    o = P.chol_tiles(lib, kk, M)
    assert o["ok1"] and o["ok2"]
    i = np.tril_indices(kk)
    assert _same(o["t1"][:kk, :kk][i], o["t2"][:kk, :kk][i])
    assert _same(o["rd1"], o["rd2"]) and np.all(o["rd2"][kk:] == 0.0)
    assert _same(np.float64(o["ld1"]), np.float64(o["ld2"]))
    assert np.all(o["t2"][kk:, :kk] == 0.0)
    assert np.all(_is_sentinel(o["t1"][kk:])), "chol_tile wrote a row the tile does not have"
    L = np.tril(o["t2"][:kk, :kk])
    ratios = dict(L=R.factor_ratio(M[:kk, :kk], L), rd=R.rd_ratio(L, o["rd2"][:kk]),
                  ld=R.logdet_ratio(L, 2.0 * o["ld2"]))
    print(f"tile kk={kk} {kind}: " + " ".join(f"{n} {v:.3g}" for n, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("col", (0, 5, 63))
def test_tile_with_a_non_positive_pivot(lib, col):
    M = R.tile_input(64, "well").copy()
    M[col, col] = 0.0
    o = P.chol_tiles(lib, 64, M)
    assert not o["ok1"] and not o["ok2"]
    assert o["ld1"] == 0.0 and o["ld2"] == 0.0
    # the columns before the pivot are finished in both, and the same
    assert _same(np.tril(o["t1"])[:, :col], np.tril(o["t2"])[:, :col])


# ---- big_solve ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kcap,k", R.SOLVE_CASES)
def test_per_lane_solve_over_panels(lib, kcap, k):
    c = F.case(R.P_BIG, k, "ill")
    ref = F.reference(R.P_BIG, k, "ill", 0)
    blk = R.block(c, kcap)
    npan, kpad8 = (k + 63) // 64, (k + 7) & ~7
    worst, resid = {}, {}
    for which, L, B, X in ((0, c["Lv"], ref["bv"], ref["xv"]), (1, c["La"], ref["ba"], ref["xa"])):
        rhs = np.zeros((64, npan * 64))
        rhs[:, :k] = B.T
        xs = P.solve(lib, kcap, k, which, blk, rhs)
        assert np.all(xs[k:npan * 64] == 0.0), "rows behind k are not zero"
        assert np.all(_is_sentinel(xs[npan * 64:])), "parked a panel the system does not have"
        err = np.linalg.norm((xs[:k].astype(R.LD) - X).astype(np.float64), axis=0)
        bound = R.solve_bounds(L, X)
        live = bound > 0
        assert np.all(err[~live] == 0.0)
        worst[which] = float((err[live] / bound[live]).max())
        resid[which] = R.solve_residual_ratio(L, B, xs[:k])
        assert kpad8 <= npan * 64
    print(f"big_solve k={k}: largest error / bound: forward V {worst[0]:.3g} A {worst[1]:.3g}, "
          f"residual V {resid[0]:.3g} A {resid[1]:.3g}")
    assert max(worst.values()) <= 1.0 and max(resid.values()) <= 1.0


# ---- the build ----------------------------------------------------------------------------------
def _written_mask(S, kcap, k):
    """which doubles of a factor's area a build of k variables writes: rows below kpad8, whole 8 x 8
    blocks up to the row's own"""
    kpad8 = (k + 7) & ~7
    nb = kcap // 8
    mask = np.zeros(nb * (nb + 1) // 2 * 64, bool)
    for I in range(kpad8 // 8):
        mask[(I * (I + 1)) // 2 * 64:((I * (I + 1)) // 2 + I + 1) * 64] = True
    return mask


def _check_block_shape(c, kcap, o):
    """everything about a finished build's block that is exact: padding, sentinels, copies"""
    S, b, k, g = o["S"], o["block"], c["k"], c["g"]
    kpad8 = (k + 7) & ~7
    fac = S["La"] - S["Lv"]
    mask = _written_mask(S, kcap, k)
    for name in ("Lv", "La"):
        area = b[S[name]:S[name] + fac]
        assert np.all(_is_sentinel(area[~mask])), "a row >= kpad8 of the factor was written"
        assert not np.any(np.isnan(area[mask]))
        Lp = R.unpack(area, kpad8)
        assert np.all(Lp[k:] == 0.0), "padding rows of the factor are not zero"
        m, n = np.triu_indices(kpad8, 1)           # the upper triangles of the diagonal blocks: zeros
        keep = (m >> 3) == (n >> 3)
        I = n[keep] >> 3
        off = ((I * (I + 1)) // 2 + I) * 64 + (m[keep] & 7) * 8 + (n[keep] & 7)
        assert np.all(area[off] == 0.0)
    for name in ("rdv", "rda", "w", "bg"):
        assert np.all(b[S[name] + k:S[name] + kcap] == 0.0), name + " behind k is not zero"
    assert _same(b[S["bg"]:S["bg"] + k], c["b"][g])
    glist = b[S["g"]:S["g"] + kcap // 2].view(np.int32)
    assert np.array_equal(glist[:k], g) and np.all(glist[k:] == 0)
    assert _same(b[S["scal"]:S["scal"] + 8],
                 np.array([o[n] for n in ("logp", "lp", "ldv", "lda", "Q", "c", "SS", "pd")]))
    assert _same(o["w_lds"][:k], b[S["w"]:S["w"] + k]) and np.all(o["w_lds"][k:] == 0.0)
    assert _same(o["rdv_lds"][:k], b[S["rdv"]:S["rdv"] + k]) and np.all(o["rdv_lds"][k:] == 0.0)
    assert np.all(_is_sentinel(b[S["ia"] + 16 * kcap:])), "the block's tail was written"


def _check_inverses(c, kcap, o):
    """S.iv / S.ia: filled for k <= 128, within test_inverse_blocks' bound (16 u kappa(L_II) of the exact
    inverse of the block's own factor, relative to the largest entry); untouched beyond"""
    S, b, k = o["S"], o["block"], c["k"]
    worst = 0.0
    for name, fname in (("iv", "Lv"), ("ia", "La")):
        area = b[S[name]:S[name] + 16 * kcap]
        if k > 128:
            assert np.all(_is_sentinel(area)), "inverses written for a model the matrix cores do not serve"
            continue
        nI = F.block_rows(k)
        L = R.unpack(b[S[fname]:], k)
        got = area[:256 * nI].reshape(nI, 16, 16)
        exact = F.exact_inverse_blocks(L, k)
        for I in range(nI):
            kk = min(max(k - 16 * I, 0), 16)
            assert np.all(got[I][kk:] == 0.0) and np.all(got[I][:, kk:] == 0.0) and np.all(np.triu(got[I], 1) == 0.0)
            if kk:
                kap = np.linalg.cond(L[16 * I:16 * I + kk, 16 * I:16 * I + kk])
                err = float(np.abs(got[I].astype(R.LD) - exact[I]).max())
                worst = max(worst, err / (16 * R.U * kap * float(np.abs(exact[I]).max())))
        assert np.all(_is_sentinel(area[256 * nI:]))
    return worst


def _build_both(lib, c, kcap, **over):
    """one-wave and two-wave build of the same case: the block, the scalars and the LDS vectors have to
    be the same bytes"""
    o1, o2 = P.build(lib, 1, 0, c, kcap, **over), P.build(lib, 2, 0, c, kcap, **over)
    assert _same(o1["block"], o2["block"]), "the two-wave build's block differs from the one-wave build's"
    for n in P.SCALARS:
        assert _same(np.float64(o1[n]), np.float64(o2[n])), n
    assert _same(o1["w_lds"], o2["w_lds"]) and _same(o1["rdv_lds"], o2["rdv_lds"])
    return o1


def _run_build_case(lib, kcap, k, kind, mode):
    c = R.build_case(k, kind, mode)
    o = _build_both(lib, c, kcap)
    assert o["k"] == k and o["pd"] == 1.0 and o["bad"] == 0.0
    _check_block_shape(c, kcap, o)
    ratios = R.check_build(c, P.build_fields(o, k))
    ratios["inverses"] = _check_inverses(c, kcap, o)
    print(f"build k={k} {kind} mode {mode}: " + " ".join(f"{n} {v:.3g}" for n, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("kcap,k", R.BUILD_CASES)
def test_build_with_one_wave_and_with_two(lib, kcap, k, kind):
    _run_build_case(lib, kcap, k, kind, 0)


@pytest.mark.parametrize("kcap,k", R.MODE1_CASES)
def test_build_in_mode_1(lib, kcap, k):
    _run_build_case(lib, kcap, k, "ill", 1)


@pytest.mark.parametrize("waves", (1, 2))
def test_reuse_rebuild_equals_a_fresh_build(lib, waves):
    kcap, k = 256, 193
    c = R.build_case(k, "ill")
    first = P.build(lib, waves, 0, c, kcap)
    S = first["S"]
    xty2 = np.ascontiguousarray(c["xty"] * 1.03 + 0.01)
    new = dict(xty=xty2, ss0q=c["ss0q"] + 7.5)
    again = P.build(lib, waves, 1, c, kcap, block=first["block"], **new)
    fresh = P.build(lib, waves, 0, c, kcap, **new)
    assert _same(again["block"][:S["w"]], first["block"][:S["w"]]), "a REUSE rebuild touched the factors"
    assert not _same(again["block"][S["w"]:S["w"] + k], first["block"][S["w"]:S["w"] + k])
    assert _same(again["block"], fresh["block"])
    for n in P.SCALARS:
        assert _same(np.float64(again[n]), np.float64(fresh[n])), n
    assert _same(again["w_lds"], fresh["w_lds"]) and _same(again["rdv_lds"], fresh["rdv_lds"])


# ---- the build's verdicts ---------------------------------------------------------------------
VK, VKCAP = 200, 256


def _without_variable(M, j):
    M = M.copy()
    M[j, :] = 0.0
    M[:, j] = 0.0
    return M


@pytest.mark.parametrize("pos", (3, 64, 130))
def test_verdict_v_not_positive_definite(lib, pos):
    c = R.build_case(VK, "well")
    o = _build_both(lib, c, VKCAP, V=_without_variable(c["V"], c["g"][pos]))
    assert o["pd"] == 0.0 and o["logp"] == NINF and o["bad"] == 0.0 and o["k"] == VK


def test_verdict_a_without_a_factor(lib):
    c = R.build_case(VK, "well")
    zero = np.zeros_like(c["A"])
    o = _build_both(lib, c, VKCAP, A=zero)
    assert o["lda"] == NINF and o["logp"] == NINF and o["pd"] == 1.0 and o["bad"] == 0.0
    ratios = R.check_build(dict(c, A=zero, Ma=np.zeros((VK, VK))), P.build_fields(o, VK), a_ok=False)
    print("A = 0: " + " ".join(f"{n} {v:.3g}" for n, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_verdict_both_fail(lib):
    c = R.build_case(VK, "well")
    o = _build_both(lib, c, VKCAP, V=_without_variable(c["V"], c["g"][64]), A=np.zeros_like(c["A"]))
    assert o["pd"] == 0.0 and o["logp"] == NINF and o["bad"] == 0.0


@pytest.mark.parametrize("what", ("max_model_size", "l1"))
def test_verdict_impossible_under_the_prior(lib, what):
    c = R.build_case(VK, "well")
    if what == "l1":
        l1 = c["l1"].copy()
        l1[c["g"][5]] = NINF
        over = dict(l1=l1)
    else:
        over = dict(max_model_size=VK - 1)
    o = _build_both(lib, c, VKCAP, **over)
    S = o["S"]
    assert o["logp"] == NINF and o["lp"] == NINF and o["bad"] == 0.0 and o["k"] == VK
    assert np.all(_is_sentinel(o["block"][:S["rdv"]])), "the factors were touched"


def test_verdict_empty_model(lib):
    c = R.build_case(VK, "well")
    o = _build_both(lib, c, VKCAP, gamma=np.zeros(R.P_BIG, np.uint8))
    lp = R.LD(c["l0"][0]) * R.P_BIG
    h = R.LD(c["DF"]) / 2 - 1
    want = lp - h * np.log(R.LD(c["ss0q"]))
    # lp: 18 additions in a lane and six across; then the logarithm, the product, the subtraction
    bound = R.gamma_n(24) * abs(lp) + 4 * R.U * (abs(lp) + h * abs(np.log(R.LD(c["ss0q"]))))
    assert o["k"] == 0.0 and o["bad"] == 0.0 and o["SS"] == c["ss0q"]
    assert abs(R.LD(o["logp"]) - want) <= bound
    assert np.all(_is_sentinel(o["block"][:o["S"]["scal"]])), "an empty model wrote a factor"


def test_verdict_negative_ss(lib):
    c = R.build_case(VK, "well")
    f64 = R.numpy_build(c)
    assert f64["Q"] - f64["c"] > 1.0
    o = _build_both(lib, c, VKCAP, ss0q=1e-3)
    assert o["bad"] == CHAIN_NEGATIVE_SS and o["logp"] == NINF and o["SS"] < 0.0


# ---- proposals ------------------------------------------------------------------------------------
def _eval_block(c, kcap):
    """the case's block with, up to 128 variables, the inverse diagonal blocks the matrix cores multiply by"""
    S, k = F.layout(kcap), c["k"]
    b = R.block(c, kcap)
    if k <= 128:
        nI = F.block_rows(k)
        for name, L in (("iv", c["Lv"]), ("ia", c["La"])):
            b[S[name]:S[name] + 256 * nI] = F.diag_inverse_blocks(L, k, nI).ravel()
    return b


def _check_window(c, out, want, bound, kind, skip=()):
    """every fast lane inside its bound, slow lanes flagged, wave 1 the same bits as wave 0; returns the
    largest error / bound"""
    assert _same(out[0], out[1]), "the two wavefronts' proposals differ"
    logp, slow, bad = out[0]
    worst = 0.0
    for lane, kd in enumerate(kind):
        if lane in skip or kd == "none":
            continue
        if kd == "slow":
            assert slow[lane] == 1.0 and logp[lane] == NINF and bad[lane] == 0.0, lane
        elif kd == "bad":
            if abs(want[lane]) > bound[lane]:
                assert bad[lane] == 1.0 and logp[lane] == NINF and slow[lane] == 0.0, lane
        else:
            assert slow[lane] == 0.0 and bad[lane] == 0.0 and np.isfinite(logp[lane]), (lane, kd)
            r = float(abs(R.LD(logp[lane]) - want[lane]) / bound[lane])
            assert r <= 1.0, (lane, kd, r)
            worst = max(worst, r)
    return worst


@pytest.mark.parametrize("kcap,k", R.EVAL_CASES)
def test_proposals_of_a_window(lib, kcap, k):
    c = R.eval_case(k)
    blk = _eval_block(c, kcap)
    worst = {}
    for jbase in R.eval_windows(k):
        out = P.evaluate(lib, c, kcap, blk, jbase)
        worst[jbase] = _check_window(c, out, *R.eval_reference(c, jbase))
    print(f"big_eval k={k}: largest error / bound per window " + " ".join(f"{j}: {v:.3g}" for j, v in worst.items()))


def _first(kind, what):
    return kind.index(what)


@pytest.mark.parametrize("kcap,k", ((128, 65), (256, 129)))
def test_proposals_dead_under_the_prior(lib, kcap, k):
    c = R.eval_case(k)
    blk = _eval_block(c, kcap)
    want, bound, kind = R.eval_reference(c, 0)
    base = P.evaluate(lib, c, kcap, blk, 0)
    a, d = _first(kind, "add"), _first(kind, "drop")
    l1, l0 = c["l1"].copy(), c["l0"].copy()
    l1[a] = NINF
    l0[d] = NINF
    out = P.evaluate(lib, c, kcap, blk, 0, l1=l1, l0=l0)
    for lane in (a, d):
        assert out[0, 0, lane] == NINF and out[0, 1, lane] == 0.0 and out[0, 2, lane] == 0.0
    others = [x for x in range(64) if x not in (a, d)]
    assert _same(out[:, :, others], base[:, :, others])
    # max_model_size = k: every add is dead, the drops are what they were
    out = P.evaluate(lib, c, kcap, blk, 0, max_model_size=k)
    adds = [x for x in range(64) if not c["gamma"][x]]
    drops = [x for x in range(64) if c["gamma"][x]]
    assert np.all(out[:, 0, adds] == NINF) and np.all(out[:, 1:, adds] == 0.0)
    assert _same(out[:, :, drops], base[:, :, drops])


def test_proposals_of_a_model_of_one_variable(lib):
    """its drop is the empty model's closed form, within 2 u of the two terms' magnitudes"""
    c = R.eval_case(1)
    blk = _eval_block(c, 128)
    want, bound, kind = R.eval_reference(c, 512)
    assert kind.count("empty") == 1
    out = P.evaluate(lib, c, 128, blk, 512)
    print(f"big_eval k=1: largest error / bound {_check_window(c, out, want, bound, kind):.3g}")


@pytest.mark.parametrize("kcap,k", ((128, 65), (256, 129)))
def test_proposal_of_a_copy_of_an_included_variable(lib, kcap, k):
    """d2 is 0 in exact arithmetic.  big_ref.copy_lane_verdict shows from the long-double solve and the
    sums' bounds that every admissible device value ends at -inf: d2 <= 0 (no flag), or a d2 so small
    that SS' < 0 (bad_ss).  Asserted: logp is -inf, never NaN or finite, the flags agree with the
    verdict, and every other lane is within its bound."""
    c = R.eval_case(k)
    blk = _eval_block(c, kcap)
    want, bound, kind = R.eval_reference(c, 0)
    lane, pos = _first(kind, "add"), 3
    gi = int(c["g"][pos])
    verdict = R.copy_lane_verdict(c, lane, pos)
    assert verdict in ("notpd", "dead")
    V = c["V"].copy()
    V[lane, :] = V[gi, :]
    V[:, lane] = V[:, gi]
    V[lane, lane] = V[gi, gi]
    out = P.evaluate(lib, c, kcap, blk, 0, V=V)
    assert out[0, 0, lane] == NINF and out[0, 1, lane] == 0.0
    if verdict == "notpd":
        assert out[0, 2, lane] == 0.0
    print(f"copy of an included column, k={k}: {verdict}, bad_ss {out[0, 2, lane]:.0f}")
    _check_window(c, out, want, bound, kind, skip=(lane,))


@pytest.mark.parametrize("kcap,k", ((128, 65), (256, 129)))
def test_proposals_with_a_negative_ss(lib, kcap, k):
    c = R.eval_case(k)
    blk = _eval_block(c, kcap)
    small = dict(c, ss0q=float(c["model"][4] - c["model"][5] + 1.0))     # SS of the current model: 1
    want, bound, kind = R.eval_reference(small, 0)
    decided = [x for x in range(64) if kind[x] == "bad" and abs(want[x]) > bound[x]]
    assert decided and kind.count("drop") >= 1
    out = P.evaluate(lib, small, kcap, blk, 0)
    _check_window(small, out, want, bound, kind)
