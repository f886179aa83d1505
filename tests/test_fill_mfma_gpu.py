"""The table fill's triangular solves, launched directly (tests/cpp/fill_probe.hip) and compared
with forward substitution in numpy.longdouble on the same f64 factor (tests/fill_ref.py):
diag_inverses and mf_proposal_sums on the f64 matrix cores (ssvs_fill_mfma.h) in the three
instances the product has -- <3> at capacity 48, <4> at 64, <8> in the large-model kernel's
block of capacity 128 -- and the per-lane solve_blocks they replaced.  Chain parity sees these
numbers only through accept / reject decisions; here a relative error of 1e-11 fails.

Model sizes k at every edge of mf_block_rows and of kpad8, windows jbase = 0, 64, 128 (the last
also at a p it overruns), a well-conditioned and an ill-conditioned factor.  The model block
holds NaN wherever the fill's header says a thing is not there (fill_ref.block), so a NaN in a
fast lane's sums is a mask that failed.  Assertions are on FAST lanes only: the contract leaves
the others unspecified, beyond writing nothing outside the output (guards: fill_probe_lib).

Tolerances, u = 2^-53, kappa = kappa_2(L) by numpy (fill_ref.tolerances): the forward error of
substitution, gamma_k cond, times 8 for the block-inverse variant and the squared norm:
  |nv - ref| <= 8 k u kappa ref (na alike), |dv - ref| <= 8 k u kappa |x_V| |w|,
  |ab - ref| <= 8 k u |rhs_A| |b_g|.
tests/test_fill_ref_cpu.py shows that f64 substitution in either order stays inside them.
Every test prints the largest observed ratio to its bound."""
import numpy as np
import pytest

import fill_probe_lib as P
import fill_ref as R

pytestmark = pytest.mark.gpu

LANE_CASES = ([(2, 16, k) for k in (1, 8, 9, 16)] + [(6, 48, k) for k in (7, 17, 40, 41, 48)] +
              [(8, 64, k) for k in (49, 56, 57, 64)])
NAMES = ("nv", "dv", "na", "ab")


@pytest.fixture(scope="module")
def lib():
    return P.load()


def _check_sums(got, c, ref, what):
    """fast lanes within the bounds; returns the largest error / bound"""
    fast = (ref["flags"] & R.FAST) != 0
    tol = R.tolerances(c, ref)
    worst = 0.0
    for s in range(4):
        g = got[s][fast]
        assert np.all(np.isfinite(g)), f"{what}: {NAMES[s]} is not finite in a fast lane: a mask let NaN through"
        err = np.abs(g.astype(R.LD) - ref["sums"][s][fast]).astype(np.float64)
        t = tol[s][fast]
        ratio = float(np.max(np.where(t > 0, err / np.where(t > 0, t, 1.0), np.where(err > 0, np.inf, 0.0))))
        assert ratio <= 1.0, f"{what}: {NAMES[s]} misses its bound by a factor {ratio:.3g}"
        worst = max(worst, ratio)
    return worst


def test_layout_is_the_products(lib):
    for kcap in (16, 48, 64, 128):
        S = R.layout(kcap)
        assert P.layout(lib, kcap) == {n: S[n] for n in ("Lv", "La", "rdv", "rda", "w", "bg", "iv", "ia", "total")}
    assert [lib.fp_block_rows(k) for k in range(1, 129)] == [R.block_rows(k) for k in range(1, 129)]


def test_requests_out_of_range_are_refused_without_a_launch(lib):
    c = R.case(R.P_FULL, 41, "well")
    b = R.block(c, 48)
    out = np.zeros(256)
    fl = np.ascontiguousarray(R.flags(c, 0))
    V, A, g = c["V"], c["A"], np.ascontiguousarray(c["g"])

    def sums(maxni, kcap, gl, p=R.P_FULL, jbase=0, blk=b):
        return lib.fp_sums(maxni, P._p(V), P._p(A), p, R.SV, R.SA, P._p(blk), blk.size, kcap, P._p(gl), len(gl), jbase,
                           P._p(fl), P._p(out), out.size)
    assert sums(3, 48, np.arange(49, dtype=np.int32)) == P.BAD_REQUEST            # k > 16 MAXNI, k > kcap
    assert sums(3, 64, np.arange(49, dtype=np.int32), blk=R.block(c, 64)) == P.BAD_REQUEST   # k > 16 MAXNI
    assert sums(4, 48, np.arange(49, dtype=np.int32)) == P.BAD_REQUEST            # k > kcap
    bad = g.copy()
    bad[-1] = R.P_FULL
    assert sums(3, 48, bad) == P.BAD_REQUEST                                      # g[i] >= p
    assert sums(3, 48, g, p=R.P_ODD, jbase=128) == P.BAD_REQUEST                  # a fast lane past p
    assert sums(3, 48, g, blk=b[:-8]) == P.BAD_REQUEST                            # a block too short
    assert lib.fp_inverses(48, 49, P._p(b), b.size) == P.BAD_REQUEST
    assert lib.fp_lane_solve(6, P._p(b), b.size, 64, 41, 0, P._p(np.zeros(64 * 48)), 64 * 48) == P.BAD_REQUEST


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("maxni,kcap,k", R.SUMS_CASES)
def test_proposal_sums_match_longdouble_substitution(lib, maxni, kcap, k, kind):
    worst = 0.0
    for p, jbase in R.WINDOWS:
        c = R.case(p, k, kind)
        ref = R.reference(p, k, kind, jbase)
        got, _ = P.sums(lib, maxni, c["V"], c["A"], c["sv"], c["sa"], R.block(c, kcap), kcap, c["g"], jbase,
                        ref["flags"])
        worst = max(worst, _check_sums(got, c, ref, f"<{maxni}> k={k} {kind} p={p} jbase={jbase}"))
    print(f"fill <{maxni}> k={k} {kind}: kappa V {R.case(R.P_FULL, k, kind)['kv']:.3g}, "
          f"largest error / bound {worst:.3g}")


@pytest.mark.parametrize("maxni,kcap,k", [(3, 48, 7), (3, 48, 41), (4, 64, 57), (8, 128, 97), (8, 128, 113)])
def test_inverse_blocks(lib, maxni, kcap, k):
    """every entry within 16 u kappa(L_II) of the exact inverse, relative to the block's largest
    entry; rows and columns >= k and the upper triangle exactly zero; nothing else in the block
    touched; byte for byte what the sums kernel leaves in its block"""
    c = R.case(R.P_FULL, k, "ill")
    S, b0 = R.layout(kcap), R.block(c, kcap)
    b = P.inverses(lib, kcap, k, b0)
    nI = R.block_rows(k)
    worst = 0.0
    for name, L in (("iv", c["Lv"]), ("ia", c["La"])):
        got = b[S[name]:S[name] + 256 * nI].reshape(nI, 16, 16)
        exact = R.exact_inverse_blocks(L, k)
        for I in range(nI):
            kk = min(max(k - 16 * I, 0), 16)
            assert np.all(got[I][kk:] == 0.0) and np.all(got[I][:, kk:] == 0.0)
            assert np.all(np.triu(got[I], 1) == 0.0)
            if kk:
                kap = np.linalg.cond(L[16 * I:16 * I + kk, 16 * I:16 * I + kk])
                err = float(np.abs(got[I].astype(R.LD) - exact[I]).max())
                bound = 16 * R.U * kap * float(np.abs(exact[I]).max())
                assert err <= bound, (name, I, err / bound)
                worst = max(worst, err / bound)
        # the part of S.iv / S.ia no block row of this model has stays as it was
        assert np.all(np.isnan(b[S[name] + 256 * nI:S[name] + 16 * kcap]))
    assert b[:S["iv"]].tobytes() == b0[:S["iv"]].tobytes()
    ref = R.reference(R.P_FULL, k, "ill", 0)
    _, bs = P.sums(lib, maxni, c["V"], c["A"], c["sv"], c["sa"], b0, kcap, c["g"], 0, ref["flags"])
    assert bs.tobytes() == b.tobytes()
    print(f"inverses <{maxni}> k={k}: largest error / bound {worst:.3g}")


def _lane_rhs(B, nb):
    """the fill's right-hand sides as the per-lane route's caller forms them: rows >= k zero"""
    out = np.zeros((64, nb * 8))
    out[:, :B.shape[0]] = B.T
    return out


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("nb,kcap,k", LANE_CASES)
def test_per_lane_solve_matches_reference_and_the_matrix_core_route(lib, nb, kcap, k, kind):
    """solve_blocks<NB>: |x - ref| <= 8 k u kappa |x| per right-hand side; at the capacities the
    matrix-core route serves, the sums formed from its solutions in longdouble agree with
    mf_proposal_sums on the same block within twice the sums' bounds"""
    p, jbase = R.P_FULL, 64
    c = R.case(p, k, kind)
    ref = R.reference(p, k, kind, jbase)
    fast = (ref["flags"] & R.FAST) != 0
    blk = R.block(c, kcap, zero_pad=True)
    xs = []
    worst = 0.0
    for which, B, X, kap in ((0, ref["bv"], ref["xv"], c["kv"]), (1, ref["ba"], ref["xa"], c["ka"])):
        x = P.lane_solve(lib, nb, blk, kcap, k, which, _lane_rhs(B, nb))
        kpad8 = (k + 7) & ~7
        assert np.all(x[:, k:kpad8] == 0.0)                      # zero rows, rd = 0: x stays 0
        assert np.all(x[:, kpad8:] == 0.0)                       # blocks the model does not have: untouched
        x = x[:, :k].T
        assert np.all(np.isfinite(x))
        err = np.linalg.norm((x.astype(R.LD) - X).astype(np.float64), axis=0)
        bound = 8 * k * R.U * kap * np.linalg.norm(X.astype(np.float64), axis=0)
        assert np.all(err[fast] <= bound[fast]), (which, float((err[fast] / bound[fast]).max()))
        worst = max(worst, float((err[fast] / bound[fast]).max()))
        xs.append(x.astype(R.LD))
    print(f"solve_blocks<{nb}> k={k} {kind}: largest error / bound {worst:.3g}")
    if nb >= 6:
        maxni = nb // 2
        got, _ = P.sums(lib, maxni, c["V"], c["A"], c["sv"], c["sa"], blk, kcap, c["g"], jbase, ref["flags"])
        lane = R.sums(xs[0], xs[1], ref["ba"], c["w"], c["bg"])
        tol = R.tolerances(c, ref)
        for s in range(4):
            d = np.abs(got[s].astype(R.LD) - lane[s]).astype(np.float64)
            assert np.all(d[fast] <= 2 * tol[s][fast]), (NAMES[s], float((d[fast] / tol[s][fast]).max()))


@pytest.mark.parametrize("maxni,kcap,k", [(3, 48, 9), (3, 48, 41), (4, 64, 57), (8, 128, 81), (8, 128, 113)])
def test_drop_of_the_first_listed_variable(lib, maxni, kcap, k):
    """k no multiple of 16: the padded rows of the column gather g[0] again, so for the drop of
    j = g[0] they receive the drop's e = 1 as well -- rows that are not the model's, which the
    zero rows and columns of inv(L_II) and the weights' mask must keep out of the sums"""
    for kind in R.KINDS:
        c = R.case(R.P_FULL, k, kind)
        ref = R.reference(R.P_FULL, k, kind, 0)
        lane = int(c["g"][0])
        assert lane < 64 and ref["flags"][lane] == R.FAST
        only = np.zeros(64, np.int32)
        only[lane] = R.FAST
        got, _ = P.sums(lib, maxni, c["V"], c["A"], c["sv"], c["sa"], R.block(c, kcap), kcap, c["g"], 0, only)
        one = dict(flags=only, ba=ref["ba"], sums=ref["sums"])
        _check_sums(got, c, one, f"drop of g[0], <{maxni}> k={k} {kind}")


@pytest.mark.parametrize("k", [1, 9, 17, 33, 41, 48])
def test_capacities_48_and_64_give_the_same_bytes(lib, k):
    """the <3> and <4> instances run the same mf_pass<NI> on the same numbers, placed at each
    capacity's own layout offsets: identical sums, identical inverse blocks"""
    for kind in R.KINDS:
        c = R.case(R.P_FULL, k, kind)
        ref = R.reference(R.P_FULL, k, kind, 64)
        a, ba = P.sums(lib, 3, c["V"], c["A"], c["sv"], c["sa"], R.block(c, 48), 48, c["g"], 64, ref["flags"])
        b, bb = P.sums(lib, 4, c["V"], c["A"], c["sv"], c["sa"], R.block(c, 64), 64, c["g"], 64, ref["flags"])
        fast = (ref["flags"] & R.FAST) != 0
        assert a[:, fast].tobytes() == b[:, fast].tobytes()
        Sa, Sb, n = R.layout(48), R.layout(64), 256 * R.block_rows(k)
        for name in ("iv", "ia"):
            assert ba[Sa[name]:Sa[name] + n].tobytes() == bb[Sb[name]:Sb[name] + n].tobytes()
