"""The kernels of student_kernel.hip, quantile_kernel.hip and mlogit_kernel.hip, launched directly
(tests/cpp/latent_probe.hip, which includes the product's files themselves) and compared per
observation with the references of tests/latent_ref.py: student_impute_kernel<false|true>,
student_ss_h_kernel, student_ss_suf_kernel, student_sigma_nu_kernel<false|true>,
quantile_impute_kernel, mlogit_expand_kernel, mlogit_impute_kernel and mlogit_wss_kernel.  The
chain tests see these numbers only after a GEMM and a sweep, as a coefficient at 1e-8 on two chains;
here every observation of every chain is compared.

Cases (latent_ref.case_names and sigma_nu_cases; tests/test_latent_ref_cpu.py asserts, without a
GPU, that each reaches the paths it is there for): per imputation kernel n = 1, 255, 256, 257, 513
of the family's edge table, slot indices that pass 2^32, chain_offset 7, a chain that is not
CHAIN_OK at entry, p = 1100 with exactly 1024 and with 1025 columns, and a slot that serves one
uniform.  That last case is NOT an overrun: a draw that outlives its slot goes on in the slot's
spill stream, on the device and in the oracle alike (device_rng.h), and CHAIN_RNG_BRANCH needs 2^20
uniforms there, which no draw of these kernels takes; the case holds the kernel to the oracle's
spill stream, status CHAIN_OK.

The quantile table's residuals of 1e-160 and 1e300 sit in cases of their own, on one chain each:
both set QUANTILE_WEIGHT_ERROR there and leave the other chains exact.  At 1e-160 it is the
smaller root that fails (t (2 + t) overflows and the draw is 0) -- no slot takes the larger root
there, mu / (mu + x) rounds to 1 --; the larger root's failure, mu mu underflowing to 0, is the
case at 1e300 (tests/test_latent_ref_cpu.py::test_quantile_extremes).

Bounds: per value 4 x the spread of the reference over 8 replays + 8 ulp (latent_ref's docstring,
imputer_ref.bounded()).  Status words, missing steps, observations left out, the mixture's
precisions w, H_t from given weights, student_ss_suf_kernel's z, the expanded design, the
sentinels of everything a kernel must not write and the guard bands (latent_probe_lib) are compared
bit for bit; so are wss_part and wss, recomputed from the kernel's own u and w by the fixed tree
(latent_ref.wss_tree).  The Student table gives every nu of the issue a chain with a model, which
meets every delta; chain 1, the empty model, repeats a nu (latent_ref.CHAIN_NUS).  No case is built in which two different error codes arise on one chain:
threads write the status word unordered, and the winner is not specified.

Every test prints the largest error / bound; on the MI355X the largest per kernel were
student_impute_kernel 0.16, <true> 0.16, quantile_impute_kernel 0.50, mlogit_impute_kernel 0.17,
wss against the reference's 0.006, student_sigma_nu_kernel 0.10, <true> 0.09; everything compared
bit for bit matched (wss_part with each lane's w * (u * u) fused into its running sum: the fixed
tree is accepted with that product fused or rounded on its own, the source does not say which)."""
import math

import numpy as np
import pytest

import latent_probe_lib as P
import latent_ref as R
from rng_probe_lib import SENT_BITS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = P.load()
    assert (lib.lp_chain_ok(), lib.lp_chain_rng_branch(), lib.lp_chain_model_too_large()) == (R.OK, R.RNG_BRANCH,
                                                                                            R.MODEL_TOO_LARGE)
    assert (lib.lp_student_slice_error(), lib.lp_student_bad_weight(), lib.lp_quantile_weight_error(),
            lib.lp_mlogit_impute_error()) == (R.SLICE_ERROR, R.BAD_WEIGHT, R.QUANTILE_WEIGHT_ERROR, R.MLOGIT_IMPUTE_ERROR)
    assert [lib.lp_kmax(f) for f in range(3)] == [R.KMAX] * 3 and lib.lp_max_choices() == R.MAX_CHOICES
    assert [(lib.lp_stream(k), lib.lp_stride(k)) for k in range(4)] == [
        (R.STUDENT_STREAM, R.STUDENT_STRIDE), (R.SN_STREAM, R.SN_STRIDE), (R.QUANTILE_STREAM, R.QUANTILE_STRIDE),
        (R.MLOGIT_STREAM, R.MLOGIT_STRIDE)]
    assert (lib.lp_acc_count(), lib.lp_acc_sigsq(), lib.lp_acc_sigsq2()) == (R.ACC_COUNT, R.ACC_SIGSQ, R.ACC_SIGSQ2)
    return lib


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check(name, case, ref, got):
    """every row of every chain; returns the largest error / bound"""
    kind = case["kind"]
    assert list(got["status"]) == list(ref["status"]), (name, got["status"], ref["status"])
    w, loose = ref["written"], ref["loose"]
    worst = 0.0
    for arr in ("z", "w", "u", "h"):
        if arr not in got:
            continue
        g = got[arr]
        if arr not in R.OUTPUTS[kind]:
            assert np.all(g == SENT_BITS), "%s: %s was written" % (name, arr)
            continue
        assert np.all(g[~w] == SENT_BITS), "%s: %s written where nothing belongs" % (name, arr)
        assert not np.any(g[w] == SENT_BITS), "%s: %s not written at %s" % (name, arr, np.argwhere(w & (g == SENT_BITS))[:4])
        val = g.view(np.float64)
        if loose.any():
            # (no reference value: a finite number that is not negative -- a weight, a variance --
            # or, for u and z, just finite)
            v = val[loose]
            assert np.all(np.isfinite(v)) and (arr in ("u", "z") or np.all(v >= 0.0))
        want, bound = ref["want"][arr], ref["bound"][arr]
        exact = (ref["exact"] | (w if (kind == "mlogit" and arr == "w") else False)) & ~loose
        assert np.array_equal(g[exact], _bits(want[exact])), "%s: %s differs where it is exact" % (name, arr)
        m = w & ~exact & ~loose
        if m.any():
            ratio = np.abs(val[m] - want[m]) / bound[m]
            worst = max(worst, float(ratio.max()))
            at = np.argwhere(m)[int(np.argmax(ratio))]
            assert np.all(ratio <= 1.0), "%s: %s[chain %d, %d] = %r, reference %r, bound %g (ratio %.3g)" % (
                name, arr, at[0], at[1], val[tuple(at)], want[tuple(at)], bound[tuple(at)], ratio.max())
    print("%s: largest error / bound %.3g" % (name, worst))
    return worst


def check_wss(name, case, ref, got):
    """wss_part and wss from the kernel's own u and w by the fixed tree, bit for bit; wss against the
    reference's within the summed bounds; a chain that is not CHAIN_OK keeps its wss unwritten"""
    n, nch = case["n"], case["M"]
    entry_ok = case["status0"] == R.OK
    worst = 0.0
    live = [c for c in range(case["chains"]) if entry_ok[c] and ref["status"][c] != R.MODEL_TOO_LARGE]
    # A lane's `wss += w * (u * u)` is one rounding where the compiler contracts it, two where not;
    # the source does not say which, so either is the fixed tree -- the same one in every chain
    trees = {fma: {c: R.wss_tree(got["w"][c].view(np.float64), got["u"][c].view(np.float64), n, nch, fma) for c in live}
             for fma in (True, False)}
    fits = [fma for fma in (True, False) if all(np.array_equal(got["wss_part"][c], _bits(trees[fma][c][0])) for c in live)]
    assert fits, ("%s: the shares are not the fixed tree's, neither with each lane's w * (u * u) fused into its sum nor "
                  "with it rounded on its own (a compiler that contracts otherwise, e.g. only some of a lane's steps, "
                  "would fail here without a kernel fault)" % name)
    for c, (want, bound) in enumerate(R.wss_reference(case, ref)):
        if c not in live:
            assert np.all(got["wss_part"][c] == SENT_BITS) and got["wss"][c] == SENT_BITS
            continue
        total = trees[fits[0]][c][1]
        if ref["status"][c] != R.OK:
            assert got["wss"][c] == SENT_BITS, "%s: wss of a chain in error was written" % name
            continue
        assert got["wss"][c] == _bits(np.array([total]))[0], "%s: chain %d's wss is not its shares in order" % (name, c)
        if not ref["loose"][c].any():
            ratio = abs(float(got["wss"][c:c + 1].view(np.float64)[0]) - want) / bound
            worst = max(worst, ratio)
            assert ratio <= 1.0, "%s: wss[%d] off the reference's by %.3g of its bound" % (name, c, ratio)
    print("%s: wss largest error / bound %.3g" % (name, worst))


@pytest.mark.parametrize("name", R.case_names())
def test_kernel_matches_reference(lib, name):
    case = R.case_of(name)
    ref = R.ref_of(name)
    if case["kind"] == "quantile":
        check(name, case, ref, P.run_quantile(lib, case))
    elif case["kind"] == "mlogit":
        # (the mixture table passed in is mlogit_oracle's, the reference's own: nothing here ties it to
        # the table the engine fills, which is local to engine_glm.hip -- tests/test_mlogit_gpu.py
        # holds the engine's draws to the same oracle)
        got = P.run_mlogit(lib, case, P.mix_table())
        check(name, case, ref, got)
        check_wss(name, case, ref, got)
    else:
        got = P.run_student(lib, case)
        check(name, case, ref, got)
        for k in ("sigsq", "nu", "dx", "margin"):        # (read, never written)
            want = _bits(case[k]) if k in case else SENT_BITS
            assert np.all(got[k] == want), "%s: %s was written" % (name, k)


# ---- student_ss_h_kernel, student_ss_suf_kernel ---------------------------------------------------------
def _ss_frame(n):
    """a state space frame for the two helpers: X, gamma and beta are not read"""
    return R.student_table("student_ss", n, chains=3)


@pytest.mark.parametrize("n", [1, 257, 513])
def test_student_ss_h(lib, n):
    """H_t from given weights bit for bit, at the rule's three exits: sigsq / w; the marginal variance
    at nu > 2; sigsq 1e8 at nu <= 2, exactly 2 included.  Nothing else is written"""
    case = _ss_frame(n)
    case["nu"] = np.array([2.0, 2.0000001, 0.11])
    w = np.array([0.0, 1e-300, 1.0, 1e300])[(np.arange(3 * n).reshape(3, n) * 5 // 3) % 4]
    got = P.run_student(lib, case, "ss_h", inputs=dict(w=w))
    obs = case["observed"].astype(bool)
    want = np.empty((3, n))
    exits = set()
    for c in range(3):
        for i in range(n):
            want[c, i], e = R.h_of(w[c, i] if obs[i] else 0.0, float(case["sigsq"][c]), float(case["nu"][c]))
            exits.add(e)
    assert n == 1 or exits == {"weight", "marginal", "floor"}
    with np.errstate(over="ignore"):
        assert np.array_equal(got["h"], _bits(want))
    assert np.array_equal(got["w"], _bits(w)) and np.all(got["z"] == SENT_BITS) and np.all(got["u"] == SENT_BITS)
    assert list(got["status"]) == [R.OK] * 3


@pytest.mark.parametrize("bad", [-1.0, np.inf, np.nan])
def test_student_ss_h_reports_a_bad_weight(lib, bad):
    """a weight of -1, inf or NaN at an observed step sets STUDENT_BAD_WEIGHT on that chain alone; at a
    missing step it is not read; a chain in error at entry is left alone.  (Seven steps: one
    wavefront, so that which steps of the failing chain are still written does not depend on timing)"""
    n = 7
    case = _ss_frame(n)
    case["observed"] = np.array([1, 1, 1, 0, 1, 1, 1], np.uint8)
    case["status0"][2] = R.MODEL_TOO_LARGE
    obs = case["observed"].astype(bool)
    w = np.random.RandomState(3).uniform(0.5, 2.0, (3, n))
    w[1, 2] = bad
    w[1, 3] = bad
    w[0, 3] = bad
    got = P.run_student(lib, case, "ss_h", inputs=dict(w=w))
    assert list(got["status"]) == [R.OK, R.BAD_WEIGHT, R.MODEL_TOO_LARGE]
    want = np.array([[R.h_of(w[c, i] if obs[i] and np.isfinite(w[c, i]) and w[c, i] > 0 else 0.0, float(case["sigsq"][c]),
                             float(case["nu"][c]))[0] for i in range(n)] for c in range(3)])
    want = _bits(want)
    want[1, 2] = SENT_BITS
    want[2, :] = SENT_BITS
    assert np.array_equal(got["h"], want)


@pytest.mark.parametrize("n", [1, 257, 513])
def test_student_ss_suf(lib, n):
    """z = w (y - offset), the same expression in double, bit for bit; z = w = 0 at a missing step"""
    case = _ss_frame(n)
    w = np.random.RandomState(100 + n).uniform(1e-3, 50.0, (3, n))
    got = P.run_student(lib, case, "ss_suf", inputs=dict(w=w))
    obs = case["observed"].astype(bool)
    assert case["offset_stride"] > n
    want = w * (case["y"] - case["offset"][:, :n])
    assert np.array_equal(got["z"], _bits(np.where(obs, want, 0.0)))
    assert np.array_equal(got["w"], _bits(np.where(obs, w, 0.0)))
    assert np.all(got["h"] == SENT_BITS) and np.all(got["u"] == SENT_BITS)
    assert list(got["status"]) == [R.OK] * 3


# ---- student_sigma_nu_kernel --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.sigma_nu_cases()))
def test_sigma_nu(lib, name):
    """u per observation, sigsq, nu and dx within their bounds; margin within the bound of its two
    operands, or the smaller one it entered with, bit for bit; the two sigma^2 moments of acc within
    theirs and the rest of acc untouched; the trace row holds the kernel's own sigsq and nu; a parked
    chain and one whose model is too large write nothing"""
    case = R.sigma_nu_cases()[name]
    ref = R.sigma_nu_ref(name)
    n, chains, ts = case["n"], case["chains"], case["trace_stride"]
    got = P.run_student(lib, case, inputs=dict(w=case["w_in"]))
    assert list(got["status"]) == list(ref["status"]), (name, got["status"], ref["status"])
    assert np.array_equal(got["w"], _bits(case["w_in"])) and np.all(got["z"] == SENT_BITS) and np.all(got["h"] == SENT_BITS)
    worst = 0.0

    def near(what, value, want, bound):
        nonlocal worst
        ratio = abs(value - want) / bound
        worst = max(worst, ratio)
        assert ratio <= 1.0, "%s: %s = %r, reference %r, bound %g (ratio %.3g)" % (name, what, value, want, bound, ratio)
    f = lambda a: a.view(np.float64)   # noqa: E731
    for c in range(chains):
        entry = {k: _bits(case[k])[c] for k in ("sigsq", "nu", "dx", "margin")}
        if ref["chains"][c] is None:
            assert all(got[k][c] == entry[k] for k in entry) and np.all(got["u"][c] == SENT_BITS)
            assert np.all(got["trace_sigsq"][c] == SENT_BITS) and np.all(got["trace_nu"][c] == SENT_BITS)
            assert got["acc"] is None or np.array_equal(got["acc"][c], _bits(case["acc"][c]))
            continue
        base, bnd, same = ref["chains"][c]
        assert same, "%s: chain %d has no reference (its replays disagree)" % (name, c)
        for k in ("sigsq", "nu", "dx"):
            if base.status == "slice_error" and k != "sigsq":
                assert got[k][c] == entry[k], "%s: %s changed on a slice error" % (name, k)
            else:
                near("%s[%d]" % (k, c), float(f(got[k])[c]), base.out[(k, 0)], bnd[(k, 0)])
        m_in = float(case["margin"][c])
        if ("margin", 0) not in base.out or m_in < base.out[("margin", 0)] - bnd[("margin", 0)]:
            assert got["margin"][c] == entry["margin"], "%s: the running minimum was lost" % name
        else:
            assert m_in > base.out[("margin", 0)] + bnd[("margin", 0)]
            near("margin[%d]" % c, float(f(got["margin"])[c]), base.out[("margin", 0)], bnd[("margin", 0)])
        gu = f(got["u"])[c]
        assert not np.any(got["u"][c] == SENT_BITS)
        for i in range(n):
            if base.out[("u", i)] == 0.0 and "observed" in case and not case["observed"][i]:
                assert got["u"][c, i] == 0, "%s: u at a missing step" % name
            else:
                near("u[%d, %d]" % (c, i), float(gu[i]), base.out[("u", i)], bnd[("u", i)])
        if got["acc"] is not None:
            keep = np.ones(R.ACC_COUNT, bool)
            keep[[R.ACC_SIGSQ, R.ACC_SIGSQ2]] = False
            assert np.array_equal(got["acc"][c][keep], _bits(case["acc"][c])[keep]), "%s: acc written elsewhere" % name
            for k in (R.ACC_SIGSQ, R.ACC_SIGSQ2):
                near("acc[%d, %d]" % (c, k), float(f(got["acc"])[c, k]), base.out[("acc", k)], bnd[("acc", k)])
        row = int(case["trace_idx"][c]) - 1
        for t in range(ts):
            if t == row:
                assert got["trace_sigsq"][c, t] == got["sigsq"][c] and got["trace_nu"][c, t] == got["nu"][c]
            else:
                assert got["trace_sigsq"][c, t] == SENT_BITS and got["trace_nu"][c, t] == SENT_BITS
    print("%s: largest error / bound %.3g" % (name, worst))


# ---- mlogit_expand_kernel -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.EXPAND_SHAPES)
def test_mlogit_expand(lib, shape):
    """X and its element-wise square, bit for bit with mlogit_oracle.expand_design"""
    n, nch, psub, pch = shape
    Xs, Xc, want = R.expand_case(n, nch, psub, pch)
    X, Xsq = P.run_expand(lib, n, nch, psub, pch, Xs, Xc)
    assert np.array_equal(X, _bits(want)), "the expanded design differs"
    assert np.array_equal(Xsq, _bits(want * want)), "its square differs"
    assert math.isfinite(float(np.abs(want).max()))
