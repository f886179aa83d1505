"""The state stream's normals (boom_amd/csrc/stream_normals.h: Box-Muller pairs, two draws per
Philox block) made on the device through the probe tests/cpp/rng_probe.hip -- stream_normals
with the NormalsInOrder and LmSlots layouts, as a workgroup and as one wavefront, and the two
wavefronts' shared sub-chunks (normals_share_ctx / normals_share_chunk) -- against
tests/philox_ref.py in numpy.longdouble.

Which draw lands in which slot is checked exactly: a wrong pair, half or block is off by order
1.  The values themselves: |z_dev - z_ref| <= K 2^-53 R with the pair's own R (relative where
|cos| is near 1, absolute near its zeros).  The formula is one log, one sqrt, one sincos and two
products.  MEASURED on the MI355X over all cases of this file against the long-double
reference: max |z_dev - z_ref| / (2^-53 R) = 2.774 (MEASURED_RATIO below; in the 2^18-draw run of
seed 99, chain 3; 2.58 over the layout cases); K = 8 is the next power of two at or above twice
that (the factor 2: the device math library differing by a last-place unit on inputs not
sampled here), and must not exceed 16 -- more would be another formula.

Every output goes in filled with a NaN-payload sentinel with 64 guard doubles on either side;
every kernel is run twice and has to give identical bytes (rng_probe_lib)."""
import itertools

import numpy as np
import pytest

import philox_ref as R
import rng_probe_lib as P
from philox_ref import DISTRIBUTION_INPUTS, DISTRIBUTION_N, distribution_failures

pytestmark = pytest.mark.gpu

MEASURED_RATIO = 2.774
K = 8
assert K <= 16 and K >= 2 * MEASURED_RATIO > K / 2

SEED, CHAIN = 2024, 7
LM_TP, LM_THREADS, LM_BS, SN_SUB = 2048, 128, 16, 128
NREF = 4100                        # draws of reference per starting draw number (the cases need <= 4096)
IN_ORDER_N = [1, 2, 3, 127, 128, 129, 255, 256, 257, 4001]
IN_ORDER_FIRST = [0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 25 - 3, 2 ** 25 - 2, 2 ** 25 + 1]
TEAMS = [(64, False), (128, False), (256, False), (128, True)]       # (threads, ONE_WAVE)
LM_T = [1, 2, 15, 16, 17, 127, 128, 129, 2047, 2048]
LM_FIRST = [2 ** 20, 2 ** 20 + 1]                                    # an even and an odd first draw
LM_FIRST_CARRY = [2 ** 24 - 1, 2 ** 25 - 3]                          # T = 2048 runs across both carries
LM_TEAMS = [(128, False), (128, True)]
FLAGS = list(itertools.product((0, 1), repeat=3))                    # (dI, dL, dH)
SHARE_FIRST = [1, 2 ** 24 - 1, 2 ** 24, 2 ** 25 + 1]
worst = {"ratio": 0.0}


@pytest.fixture(scope="module")
def lib():
    lib = P.load()
    assert (lib.rp_lm_tp(), lib.rp_sn_sub(), lib.rp_state_slot_stride()) == (LM_TP, SN_SUB, R.STATE_SLOT_STRIDE)
    return lib


_refs = {}


def reference(first, n=NREF, seed=SEED, chain=CHAIN):
    """(z, R) of draws first .. first + n - 1, computed once per starting draw and left alone"""
    key = (seed, chain, first, n)
    if key not in _refs:
        z, Rr = R.state_normals(seed, chain, first + np.arange(n, dtype=np.uint64))
        z.setflags(write=False)
        Rr.setflags(write=False)
        _refs[key] = (z, Rr)
    return _refs[key]


def check_values(got_bits, z, Rr, tag):
    got = got_bits.view(np.float64)
    assert np.all(np.isfinite(got)), (tag, "a slot that should hold a draw does not")
    ratio = np.abs(got.astype(R.LD) - z) / (R.LD(2.0) ** -53 * np.maximum(Rr, R.LD(1e-300)))
    top = float(ratio.max()) if ratio.size else 0.0
    worst["ratio"] = max(worst["ratio"], top)
    print("%s: max |z_dev - z_ref| / (2^-53 R) = %.3f (this file so far: %.3f)" % (tag, top, worst["ratio"]))
    assert top <= K, (tag, top, int(np.argmax(ratio)))


# ------------------------------------------------------------------ NormalsInOrder
@pytest.mark.parametrize("first", IN_ORDER_FIRST)
def test_in_order(lib, first):
    z, Rr = reference(first)
    for N in IN_ORDER_N:
        runs = []
        for threads, one_wave in TEAMS:
            szz, pos = P.normals_in_order(lib, SEED, CHAIN, 256 * first, N, threads, one_wave)
            assert pos == 256 * (first + N), (first, N, threads, one_wave, pos)
            runs.append(szz)
        for other in runs[1:]:
            assert np.array_equal(runs[0], other), (first, N, "the team shapes differ")
        check_values(runs[0], z[:N], Rr[:N], ("in order", first, N))


# ------------------------------------------------------------------ LmSlots
def lm_layout(T, dI, dL, dH):
    """For every slot s of the lane-major normals array the index of the sweep's draw that
    belongs there, or -1, from the layout's definition (row s >> 7 = 2 j + kind, thread s & 127,
    step t = 16 (s & 127) + (row >> 1)) and the draw numbering of kalman_lm_body: step 0 draws
    the initial state's normal (if P0 != 0) and the observation's (if H != 0), every later step
    the level's (if its variance != 0) and then the observation's."""
    nfirst, nper = dI + dH, dL + dH
    s = np.arange(2 * LM_TP)
    row, th = s >> 7, s & (LM_THREADS - 1)
    kind, t = row & 1, LM_BS * th + (row >> 1)
    before = np.where(t == 0, 0, nfirst + (t - 1) * nper)           # draws of the steps before t
    exists = np.where(t == 0, np.where(kind == 0, dI, dH), np.where(kind == 0, dL, dH)) == 1
    offset = np.where(kind == 0, 0, np.where(t == 0, dI, dL))
    draw = np.where(exists & (t < T), before + offset, -1)
    return draw, t, kind


def lm_cases():
    for T in LM_T:
        for dI, dL, dH in FLAGS:
            N = dI + dH + (T - 1) * (dL + dH)
            if N == 0:
                continue
            for first in LM_FIRST + (LM_FIRST_CARRY if T == 2048 else []):
                yield T, dI, dL, dH, first, N


def steps_starting_odd(T, dI, dL, dH, first):
    """per step with TWO draws: does its first draw have an odd global number (then the second
    slot is half of another pair: the rare branch of normals_pairs)?  per step with one draw:
    the parity of that draw"""
    draw, t, kind = lm_layout(T, dI, dL, dH)
    two, one = [], []
    for step in range(T):
        d = np.sort(draw[(t == step) & (draw >= 0)])
        if d.size == 2:
            assert d[1] == d[0] + 1
            two.append(int(first + d[0]) & 1)
        elif d.size == 1:
            one.append(int(first + d[0]) & 1)
    return two, one


def test_lm_cases_reach_the_odd_starts():
    """so that the coverage cannot silently vanish: a case all of whose steps start on an odd
    global draw, one whose steps all do but the first, one whose steps alternate"""
    all_odd = all_but_first = alternating = False
    for T, dI, dL, dH, first, N in lm_cases():
        if T < 16:
            continue
        two, one = steps_starting_odd(T, dI, dL, dH, first)
        draw, _, _ = lm_layout(T, dI, dL, dH)
        assert np.array_equal(np.sort(draw[draw >= 0]), np.arange(N)), "every draw of the sweep has one slot"
        all_odd |= len(two) == T and all(two)
        all_but_first |= len(two) == T - 1 and all(two)
        alternating |= len(one) == T and all(a != b for a, b in zip(one[:-1], one[1:]))
    assert all_odd and all_but_first and alternating


@pytest.mark.parametrize("T", LM_T)
def test_lane_major(lib, T):
    for T_, dI, dL, dH, first, N in lm_cases():
        if T_ != T:
            continue
        z, Rr = reference(first)
        draw, _, _ = lm_layout(T, dI, dL, dH)
        held = draw >= 0
        runs = []
        for threads, one_wave in LM_TEAMS:
            szz, pos = P.normals_lm(lib, SEED, CHAIN, 256 * first, T, dI, dL, dH, threads, one_wave)
            assert pos == 256 * (first + N), (T, dI, dL, dH, first, pos)
            runs.append(szz)
        assert np.array_equal(runs[0], runs[1]), (T, dI, dL, dH, first, "workgroup and one wavefront differ")
        assert np.all(runs[0][~held] == P.SENT_BITS), (T, dI, dL, dH, first, "a slot without a draw was written")
        check_values(runs[0][held], z[draw[held]], Rr[draw[held]], ("lane major", T, (dI, dL, dH), first))


# ------------------------------------------------------------------ shared sub-chunks
@pytest.mark.parametrize("T", [2048, 129])
def test_shared_sub_chunks(lib, T):
    nsub = LM_TP // SN_SUB
    k = 6
    lists = {
        "ascending": list(range(nsub)),
        "descending": list(range(nsub))[::-1],
        "split, the meeting one twice": list(range(k + 1)) + list(range(nsub - 1, k - 1, -1)),
    }
    assert sorted(set(lists["split, the meeting one twice"])) == list(range(nsub))
    assert lists["split, the meeting one twice"].count(k) == 2
    for n, (first, (dI, dL, dH)) in enumerate(itertools.product(SHARE_FIRST, [(1, 1, 1), (0, 1, 1), (1, 0, 1)])):
        whole, _ = P.normals_lm(lib, SEED, CHAIN, 256 * first, T, dI, dL, dH, 128, True)
        for name, chunks in lists.items():
            got = P.share(lib, SEED, CHAIN, 256 * first, T, dI, dL, dH, n & 1, chunks)
            assert np.array_equal(got, whole), (T, first, (dI, dL, dH), name)
        # one sub-chunk left out: the slot pairs [128 c, 128 c + 128) = rows 2 c and 2 c + 1
        c = 5
        got = P.share(lib, SEED, CHAIN, 256 * first, T, dI, dL, dH, n & 1, [x for x in range(nsub) if x != c])
        want = whole.copy()
        assert np.any(want[256 * c:256 * (c + 1)] != P.SENT_BITS)
        want[256 * c:256 * (c + 1)] = P.SENT_BITS
        assert np.array_equal(got, want), (T, first, (dI, dL, dH), "one sub-chunk omitted")
        if n == 0:
            z, Rr = reference(first)
            draw, _, _ = lm_layout(T, dI, dL, dH)
            check_values(whole[draw >= 0], z[draw[draw >= 0]], Rr[draw[draw >= 0]], ("shared", T, first))


# ------------------------------------------------------------------ distribution
@pytest.mark.parametrize("seed,chain,first", DISTRIBUTION_INPUTS)
def test_distribution_of_what_the_device_produced(lib, seed, chain, first):
    """2^18 in-order draws by one workgroup: mean, variance, skewness, excess kurtosis, the
    correlation of a pair's halves, of their squares, of a pair's second half with the next
    pair's first, lag 2, each as a z-score (|z| < 3), and Kolmogorov-Smirnov against N(0, 1)
    (p > 0.01) -- the same function as test_philox_ref.py runs on the reference's numbers, and
    the device's statistics equal the reference's to 1e-9."""
    z, Rr = reference(first, DISTRIBUTION_N, seed, chain)
    szz, pos = P.normals_in_order(lib, seed, chain, 256 * first, DISTRIBUTION_N, 128, False)
    assert pos == 256 * (first + DISTRIBUTION_N)
    check_values(szz, z, Rr, ("distribution", seed, chain, first))
    bad, st, p = distribution_failures(szz.view(np.float64), first)
    assert not bad, (st, p)
    _, st_ref, p_ref = distribution_failures(z.astype(np.float64), first)
    for name in st:
        assert abs(st[name] - st_ref[name]) <= 1e-9, (name, st[name], st_ref[name])
    assert abs(p - p_ref) <= 1e-9, (p, p_ref)
