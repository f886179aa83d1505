"""The device's scalar samplers -- d_exp_rand, d_norm_rand, d_runif, d_random_int, d_rtrun_exp,
d_rgamma_scale, d_draw_variance (device_rng.h) and ar_rtrun_norm_2 (ar_trunc_device.h) -- called
directly through tests/cpp/dist_probe.hip and compared, draw by draw, with tests/dist_ref.py.

Compared exactly: the stream position and stream id every draw ends at, *bad against the
reference's status, and the calling conventions (SeqRng = WinRng, four wavefronts = one, one lane
with its own arguments = the whole wave with them) byte for byte.  d_exp_rand, d_random_int and
d_runif(a, a) are compared bit for bit.  Every other value lies within imputer_ref.bounded(): 4 x
the spread of the reference over its 8 replays + 8 ulp of the value; no other constant.  A draw
whose replays disagree is set aside (finite, in its support, the reference's status): none but in
tn2-tail-1e-9, where dist_ref.cases() says why (tests/test_dist_ref_cpu.py holds the cap).

What the reference reaches nowhere, and so no case here: a gamma-tail hull of 64 points (the
largest has 7), a two-sided hull near its cap or a candidate outside [x0, x_last] (the largest
has 4), the slice sampler's shrinking loop.  d_rtrun_exp, d_runif and d_random_int read one number:
no slot limit sends them to the spill stream.  WinRng has no slots, so the spill cases run through
SeqRng alone.

Measured on the MI355X, largest error / bound per sampler (each test prints its own): d_rgamma_scale
0.157 (shape 0.05), d_draw_variance 0.177 (shape 1.0000001, the cut 1e-6 above the mode),
ar_rtrun_norm_2 0.25 (a window 1e-6 sigma wide), d_rtrun_exp 0.083, d_runif 0.083, d_norm_rand 0.476 over
2^18 draws; d_exp_rand, d_random_int and d_runif(a, a) bit for bit; every position, stream id, status and
convention identity exact.  No draw follows another path than the reference's: the gamma tail's hull,
whose exponent y - d z + d knot the compiler contracts, and both forms of the two-sided hull agree with
the oracle as they stand."""
import numpy as np
import pytest

import dist_probe_lib as dpl
import dist_ref as dr

pytestmark = pytest.mark.gpu

CASES = list(dr.cases())
BY_FN = {fn: [n for n in CASES if dr.cases()[n]["fn"] == fn] for fn in dpl.FN}


@pytest.fixture(scope="module")
def lib():
    return dpl.load()


_runs = {}


def run(lib, name, view=dpl.SEQ, mode=dpl.UNIFORM, threads=64):
    key = (name, view, mode, threads)
    if key not in _runs:
        case = dr.cases()[name]
        _runs[key] = dpl.draws(lib, case["fn"], dpl.pack_args(case["args"]), case["seed"], case["chain"], dr.STREAM,
                               case["index0"], dr.STRIDE, dr.serve_of(case), view, mode, threads)
    return _runs[key]


def in_support(fn, a, x):
    """a set-aside draw: finite and where the distribution lives"""
    if not np.isfinite(x):
        return False
    if fn == "draw_variance":
        # sigma^2 = fl(1 / g) with g >= cut = fl(1 / sigma_max^2): rounding is monotone
        return 0.0 < x <= 1.0 / (1.0 / (a[2] * a[2]))
    if fn == "rtrun_norm_2":
        # y in [(lo - mu) / sigma, (hi - mu) / sigma] comes back as y sigma + mu: two roundings each
        # way, each at most an ulp of the largest of |mu|, |lo|, |hi|
        slack = 4.0 * np.spacing(max(abs(a[0]), abs(a[2]), abs(a[3])))
        return a[2] - slack <= x <= a[3] + slack
    if fn == "rtrun_exp":
        return a[1] <= x <= a[2]
    return x > 0.0 if fn == "rgamma_scale" else True


def check_case(lib, name):
    """the case through SeqRng, one wavefront, against its reference; returns the largest error / bound"""
    case, ref = dr.cases()[name], dr.ref_of(name)
    x, bits, pos, stream, bad = dpl.one_wave(run(lib, name))
    assert np.array_equal(bad, ref["status"]), "*bad differs from the reference's status at %s" % np.flatnonzero(bad != ref["status"])[:8]
    failed = ref["status"] != 0
    compared = ref["same"] & ~failed
    aside = ~ref["same"] & ~failed
    assert case["loose"] or aside.sum() <= dr.SET_ASIDE_CAP * case["n"]
    exact = compared | failed
    assert np.array_equal(pos[exact], ref["pos"][exact]), "positions differ at %s" % np.flatnonzero(exact & (pos != ref["pos"]))[:8]
    assert np.array_equal(stream[exact], ref["stream"][exact])
    same_bits = bits == ref["want"].view(np.uint64)
    with np.errstate(invalid="ignore"):
        err = np.where(same_bits, 0.0, np.abs(x - ref["want"]))
        ratio = np.where(same_bits, 0.0, err / ref["bound"])
    worst = float(np.max(ratio[compared])) if compared.any() else 0.0
    over = compared & ~(ratio <= 1.0)
    print("%s: %d draws, %d compared, %d set aside, %d with a status; largest error / bound %.3g"
          % (name, case["n"], compared.sum(), aside.sum(), failed.sum(), worst))
    assert not over.any(), [(int(i), case["args"][i], float(x[i]), float(ref["want"][i]), float(ratio[i])) for i in np.flatnonzero(over)[:5]]
    for i in np.flatnonzero(aside):
        assert in_support(case["fn"], case["args"][i], float(x[i])), (name, int(i), case["args"][i], float(x[i]))
    return worst


@pytest.mark.parametrize("name", BY_FN["rgamma_scale"])
def test_rgamma_scale(lib, name):
    check_case(lib, name)


@pytest.mark.parametrize("name", BY_FN["draw_variance"])
def test_draw_variance(lib, name):
    check_case(lib, name)
    if name == "variance-zero":        # no number read, the value exact
        x, _, pos, _, _ = dpl.one_wave(run(lib, name))
        assert np.all(x == 0.0) and np.array_equal(pos, dr.ref_of(name)["pos"])


@pytest.mark.parametrize("name", BY_FN["rtrun_norm_2"])
def test_rtrun_norm_2(lib, name):
    check_case(lib, name)


@pytest.mark.parametrize("name", BY_FN["rtrun_exp"])
def test_rtrun_exp(lib, name):
    check_case(lib, name)


def test_runif(lib):
    check_case(lib, "runif")
    case, ref = dr.cases()["runif"], dr.ref_of("runif")
    _, bits, pos, _, _ = dpl.one_wave(run(lib, "runif"))
    point = np.array([a[0] == a[1] for a in case["args"]])
    assert point.sum() >= dr.MIN_COMPARED
    assert np.array_equal(bits[point], ref["want"].view(np.uint64)[point])            # bit for bit, -0.0 included
    assert np.array_equal(pos[point], np.uint64(dr.STRIDE) * (np.uint64(case["index0"]) + np.flatnonzero(point).astype(np.uint64)))


@pytest.mark.parametrize("name", ["norm_rand-spill", "exp_rand-spill"])
def test_slots_spill(lib, name):
    check_case(lib, name)
    if name.startswith("exp_rand"):
        _, bits, _, _, _ = dpl.one_wave(run(lib, name))
        assert np.array_equal(bits, dr.ref_of(name)["want"].view(np.uint64))


def test_random_int(lib):
    rows = [dr.INT_ROWS[i % len(dr.INT_ROWS)] for i in range(32 * len(dr.INT_ROWS))]
    seed, chain, index0 = dr.SEEDS[0], dr.CHAINS[1], 100
    for view in (dpl.SEQ, dpl.WIN):
        body = dpl.draws(lib, "random_int", dpl.pack_args(rows), seed, chain, dr.STREAM, index0, dr.STRIDE, dr.STRIDE, view)
        _, bits, pos, stream, bad = dpl.one_wave(body)
        for i, (lo, hi) in enumerate(rows):
            want, where, _ = dr.oracle_draw("random_int", (lo, hi), seed, chain, index0 + i)
            assert int(bits[i].astype(np.int64)) == want and (int(stream[i]), int(pos[i])) == where and bad[i] == 0


@pytest.mark.parametrize("fn", ["norm_rand", "exp_rand"])
def test_chained_draws(lib, fn):
    """2^18 consecutive draws of one stream, through both views"""
    seed, chain, pos0 = dr.CHAINED[fn]
    want, want_pos = dr.chained_ref(fn)
    args = np.zeros((dr.CHAINED_N, 4))
    bodies = [dpl.draws(lib, fn, args, seed, chain, dr.STREAM, pos0, 1, 1, view, chained=True) for view in (dpl.SEQ, dpl.WIN)]
    assert bodies[0].tobytes() == bodies[1].tobytes(), "SeqRng and WinRng differ"
    x, bits, pos, stream, bad = dpl.one_wave(bodies[0])
    assert np.array_equal(pos, want_pos) and np.all(stream == dr.STREAM) and not bad.any()
    if fn == "exp_rand":
        assert np.array_equal(bits, want.view(np.uint64))
        return
    ratio = np.abs(x - want) / dr.norm_rand_bound()
    print("norm_rand: %d draws, largest error / bound %.3g" % (x.size, ratio.max()))
    assert np.all(ratio <= 1.0)


# ---- the calling conventions ------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if not dr.cases()[n]["slot_limit"] and dr.cases()[n]["fn"] != "rtrun_norm_2"])
def test_window_view_gives_the_same_bytes(lib, name):
    """the templates over the stream view, and the hand-over to the out-of-line routines through
    seq_view / seq_resume: values, positions, stream ids and flags"""
    assert run(lib, name, view=dpl.WIN).tobytes() == run(lib, name).tobytes()


@pytest.mark.parametrize("name", BY_FN["draw_variance"])
def test_four_wavefronts_give_the_same_bytes(lib, name):
    """d_draw_variance from a workgroup of 256, as student_sigma_nu_kernel calls it"""
    four, one = run(lib, name, threads=256), run(lib, name)
    for wave in range(4):
        assert four[wave].tobytes() == one[0].tobytes(), "wavefront %d" % wave


@pytest.mark.parametrize("name", [n for n in BY_FN["rgamma_scale"] if min(a[0] for a in dr.cases()[n]["args"]) >= .3])
def test_per_lane_arguments_give_the_same_bytes(lib, name):
    """d_rgamma_scale with each lane's own (shape, scale) and slot, as student_impute_kernel and
    slt_weights_kernel call it"""
    assert run(lib, name, mode=dpl.PER_LANE).tobytes() == run(lib, name).tobytes()


REFUSED = [("rgamma_scale", (float("nan"), 1.0)), ("rgamma_scale", (0.0, 1.0)), ("rgamma_scale", (-1.0, 1.0)),
           ("rgamma_scale", (float("inf"), 1.0)), ("rgamma_scale", (2.0, 0.0)), ("rgamma_scale", (2.0, float("nan"))),
           ("rgamma_scale", (2.0, float("inf"))),
           ("draw_variance", (-1.0, 1.0, 1.0)), ("draw_variance", (float("nan"), 1.0, 1.0)), ("draw_variance", (1.0, -1.0, 1.0)),
           ("draw_variance", (1.0, float("nan"), 1.0)), ("draw_variance", (1.0, 1.0, -1.0)), ("draw_variance", (1.0, 1.0, float("nan"))),
           ("draw_variance", (0.0, 1.0, 1.0)), ("draw_variance", (1.0, 0.0, 1.0)), ("draw_variance", (1.0, float("inf"), 1.0)),
           ("draw_variance", (1.0, 1.0, 1e-200)),
           ("rtrun_norm_2", (0.0, 1.0, 1.0, 1.0)), ("rtrun_norm_2", (0.0, 1.0, 2.0, 1.0)), ("rtrun_norm_2", (0.0, 0.0, 1.0, 2.0)),
           ("rtrun_norm_2", (0.0, -1.0, 1.0, 2.0)), ("rtrun_norm_2", (0.0, 1.0, float("-inf"), 2.0)),
           ("rtrun_norm_2", (0.0, 1.0, 1.0, float("inf"))), ("rtrun_norm_2", (float("nan"), 1.0, 1.0, 2.0)),
           ("random_int", (3.0, 2.0)), ("random_int", (0.0, 2.0 ** 31 - 1)), ("random_int", (0.5, 2.0)),
           ("rtrun_exp", (1.0, 2.0, 2.0)), ("rtrun_exp", (0.0, 1.0, 2.0)), ("rtrun_exp", (1.0, 1.0, float("inf"))),
           ("runif", (0.0, float("inf")))]


def test_requests_without_an_exit_are_refused(lib):
    """the host wrapper returns -1 instead of launching, and writes nothing"""
    for fn, a in REFUSED:
        good = dict(rgamma_scale=(2.0, 1.0), draw_variance=(4.0, 2.0, 1.0), rtrun_norm_2=(0.0, 1.0, 1.0, 2.0), random_int=(0.0, 5.0),
                    rtrun_exp=(1.0, 0.0, 1.0), runif=(0.0, 1.0))[fn]
        rc, out = dpl.raw(lib, fn, dpl.pack_args([good, a, good]), 1, 2, dr.STREAM, 0, dr.STRIDE, dr.STRIDE)
        assert rc == dpl.BAD_REQUEST and np.all(out == dpl.SENT_BITS), (fn, a)
    ok = dpl.pack_args([(2.0, 1.0)] * 4)
    small = dpl.pack_args([(0.1, 1.0)] * 4)
    W = lib.dp_words()
    for kw in (dict(nout=4 * W - 1), dict(threads=256, nout=4 * 4 * W - 1), dict(threads=128), dict(view=dpl.WIN, mode=dpl.PER_LANE),
               dict(mode=dpl.PER_LANE, threads=256), dict(mode=dpl.PER_LANE, chained=True)):
        rc, out = dpl.raw(lib, "rgamma_scale", ok, 1, 2, dr.STREAM, 0, dr.STRIDE, dr.STRIDE, **kw)
        assert rc == dpl.BAD_REQUEST and np.all(out == dpl.SENT_BITS), kw
    # the shape below .3 broadcasts lane 0's draw: not for lanes with their own arguments
    assert dpl.raw(lib, "rgamma_scale", small, 1, 2, dr.STREAM, 0, dr.STRIDE, dr.STRIDE, mode=dpl.PER_LANE)[0] == dpl.BAD_REQUEST
    # WinRng has no slots; ar_rtrun_norm_2 reads a SeqRng; the functions of a whole wave have no per-lane mode
    assert dpl.raw(lib, "rgamma_scale", ok, 1, 2, dr.STREAM, 0, dr.STRIDE, 3, view=dpl.WIN)[0] == dpl.BAD_REQUEST
    assert dpl.raw(lib, "rtrun_norm_2", dpl.pack_args([(0.0, 1.0, 1.0, 2.0)]), 1, 2, dr.STREAM, 0, dr.STRIDE, dr.STRIDE, view=dpl.WIN)[0] == dpl.BAD_REQUEST
    assert dpl.raw(lib, "draw_variance", dpl.pack_args([(4.0, 2.0, 1.0)]), 1, 2, dr.STREAM, 0, dr.STRIDE, dr.STRIDE, mode=dpl.PER_LANE)[0] == dpl.BAD_REQUEST
    assert dpl.raw(lib, "rgamma_scale", ok, 1, 2, dr.STREAM, 0, dr.STRIDE, dr.STRIDE + 1)[0] == dpl.BAD_REQUEST
    assert dpl.raw(lib, "rgamma_scale", ok, 1, 2, dr.STREAM | 0x80000000, 0, dr.STRIDE, dr.STRIDE)[0] == dpl.BAD_REQUEST
