"""The three views of one Philox stream (boom_amd/csrc/device_rng.h) -- SeqRng, PairRng and
the wavefront's 128-number window WinRng -- run side by side on the device through the probe
tests/cpp/rng_probe.hip and compared BIT FOR BIT with tests/philox_ref.py (itself pinned on the
oracle by test_philox_ref.py).  Kernels mix the views freely on one stream, so all three have
to return the same 53-bit number at every position: an exact integer property, no tolerance.

Covered: the window's refill exactly at off == 128, a window filled from an odd position,
set_pos to the window's base + 128 (kept) and + 129 (dropped), backwards inside and out of
the window, stream_seek's 64-bit recombination across 2^32, the block counter's carry into
its second word (position 2^33), the seq_view / seq_resume hand-over, and a slot's transition
into its spill stream (also in the middle of a block that PairRng holds)."""
import numpy as np
import pytest

import philox_ref as R
import rng_probe_lib as P

pytestmark = pytest.mark.gpu

# (seed, chain, stream id): an ordinary one, the last chain id, a stream id with the spill bit set
KEYS = [(123, 5, 0), ((0xfeedface << 32) | 0x1234, 0xffffffff, 3), (2024, 1023, 2 | R.SPILL_STREAM_BIT)]
STARTS = [0, 1, 127, 128, 129, 2 ** 32 - 1, 2 ** 33 - 2, 2 ** 40 + 1]


@pytest.fixture(scope="module")
def lib():
    return P.load()


def draw(k):
    return ("draw", k)


def rel(d):
    return ("rel", d)


def to(q):
    return ("abs", q)


def trip(k):
    return ("trip", k)


def window_base(p):
    return p & ~1


# relative programmes, made absolute per starting position p0
PROGRAMMES = {
    # two refills of the 128-number window
    "300 in a row": lambda p0: [draw(300)],
    # the cursor ends exactly on off == 128 (no refill yet), then one more (refill), then on
    "up to the window's end and one more": lambda p0: [draw(128 - (p0 & 1)), draw(1), draw(3)],
    "forward by 1, 127, 128, 129": lambda p0: [draw(3), rel(1), draw(2), rel(127), draw(2), rel(128), draw(2),
                                               rel(129), draw(2)],
    # window loaded at base b: to b + 128 (kept: the next draw refills from there), then from
    # the new window at b + 128 to its base + 129 (dropped; refilled from an odd position)
    "to the window's end and one past it": lambda p0: [draw(2), to(window_base(p0) + 128), draw(3),
                                                        to(window_base(p0) + 128 + 129), draw(3)],
    "backward inside the window and out of it": lambda p0: [draw(50), rel(-30), draw(10), to(window_base(p0)),
                                                             draw(2), to(max(window_base(p0) - 1, 0)), draw(4)],
    "to an odd position far away": lambda p0: [draw(5), to(((p0 + 2 ** 36) | 1)), draw(5)],
    "across 2^32 and the counter's carry": lambda p0: [draw(5), to(2 ** 32 - 2), draw(5), to(2 ** 32 + 1), draw(3),
                                                        to(2 ** 33 - 3), draw(6), to(5), draw(2)],
    "seq_view / seq_resume after 5 draws": lambda p0: [draw(5), trip(7), draw(5), trip(1), draw(2)],
}


def expand(p0, programme):
    """(ops for the probe, the stream positions drawn in order, the final position)"""
    ops, positions, p = [], [], p0
    for what, a in programme:
        if what == "draw" or what == "trip":
            ops.append((P.OP_DRAW if what == "draw" else P.OP_SEQ_ROUND_TRIP, a))
            positions.extend(range(p, p + a))
            p += a
        else:
            p = p + a if what == "rel" else a
            assert p >= 0
            ops.append((P.OP_SEEK, p))
    return ops, np.array(positions, np.uint64), p


@pytest.mark.parametrize("name", list(PROGRAMMES))
def test_views_agree_with_the_reference(lib, name):
    for seed, chain, stream in KEYS:
        for p0 in STARTS:
            ops, positions, last = expand(p0, PROGRAMMES[name](p0))
            got, pos = P.views(lib, seed, chain, stream, p0, ops)
            want = R.uniform_bits(seed, chain, stream, positions)
            tag = (name, hex(seed), hex(chain), hex(stream), p0)
            for v, view in enumerate(("SeqRng", "PairRng", "WinRng")):
                assert np.array_equal(got[v, 0], got[v, 1]), (tag, view, "lane 0 and lane 63 differ")
                bad = np.flatnonzero(got[v, 0] != want)
                assert bad.size == 0, (tag, view, "first wrong number", int(bad[0]), int(positions[bad[0]]))
            assert np.all(pos == np.uint64(last)), (tag, pos, last)


def test_the_programmes_reach_the_edges():
    """from the definitions above: a draw with off == 128 pending, a window filled from an odd
    position, a seek to base + 128 and one to base + 129, a seek that changes the high word"""
    ops, positions, _ = expand(1, PROGRAMMES["up to the window's end and one more"](1))
    assert ops[0] == (P.OP_DRAW, 127) and positions[126] == 127 and positions[127] == 128
    ops, _, _ = expand(128, PROGRAMMES["to the window's end and one past it"](128))
    assert ops[1] == (P.OP_SEEK, 256) and ops[3] == (P.OP_SEEK, 256 + 129)
    ops, _, _ = expand(2 ** 32 - 1, PROGRAMMES["across 2^32 and the counter's carry"](0))
    assert any(c == P.OP_SEEK and a >> 32 for c, a in ops)


@pytest.mark.parametrize("index,stride,serve", [(0, 256, 256), (5, 256, 2), (3, 64, 3), (2 ** 30 + 1, 256, 4)])
def test_slot_goes_on_in_its_spill_stream(lib, index, stride, serve):
    n = serve + 5
    for seed, chain, stream in KEYS:
        got, info = P.slot(lib, seed, chain, stream, index, stride, serve, n)
        spilled, pos = R.slot_positions(index, stride, serve, n)
        assert np.array_equal(pos[:serve], index * stride + np.arange(serve, dtype=np.uint64))
        assert np.array_equal(pos[serve:], (index << R.SPILL_SHIFT) + np.arange(5, dtype=np.uint64))
        want = np.where(spilled, R.uniform_bits(seed, chain, stream | R.SPILL_STREAM_BIT, pos),
                        R.uniform_bits(seed, chain, stream, pos))
        tag = (hex(seed), hex(chain), hex(stream), index, stride, serve)
        for v, view in enumerate(("SeqRng", "PairRng")):
            for w in (0, 1):
                assert np.array_equal(got[v, w], want), (tag, view, w, np.flatnonzero(got[v, w] != want))
                assert int(info[v, w, 0]) == (index << R.SPILL_SHIFT) + 5, (tag, view, "final position")
                assert int(info[v, w, 1]) == stream | R.SPILL_STREAM_BIT, (tag, view, "final stream id")
                assert int(info[v, w, 2]) == 0, (tag, view, "overran()")
