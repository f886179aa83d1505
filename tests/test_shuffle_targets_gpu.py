"""The shuffle's targets (boom_amd/csrc/ssvs_device.h) launched directly on one workgroup
(tests/cpp/shuffle_targets_probe.hip): fork_shuffle_targets<W>, called as the sweep kernel calls it
behind a fork's command barrier -- with two wavefronts wave 1 draws all p - 1 targets and the
master none, with four every wavefront its share --, and the all-threads shuffle_targets of the
unforked path.  Both must leave

    oth[i] = floor((i + 1) u(pos + p - 1 - i)),   i = 1 .. p-1

with u the stream's uniforms (tests/philox_ref.py), compared exactly; entry 0 and the spare entry
p keep the sentinel they were filled with.

p: 2 and 3 (one block, one lane); 64, 65, 129, 130 (both parities around one and two lanes' worth
of blocks); 257, 258 (128 blocks and one more: a second pass of the 64-lane loop for one lane at
an odd position); 512, 513 (the headline's size: 256 blocks, 257 at an odd position -- a fifth
pass for one lane); 1024, 1025 and 1500 (the last size at which two wavefronts leave the draw to
wave 1, FORK_SOLO_MAX_P, and the first two at which they share it as four do).  pos: both parities at the stream's start, in the middle, and where the
position passes 2^32 inside the shuffle (the block index's low word passes 2^31)."""
import functools

import numpy as np
import pytest

import philox_ref as R
import shuffle_targets_probe_lib as P

SIZES = (2, 3, 64, 65, 129, 130, 257, 258, 512, 513, 1024, 1025, 1500)
WAVES = (2, 4)
POSITIONS = (0, 1, 510, 511, 2 ** 32 - 3, 2 ** 32 - 2)
SEED, CHAIN, STREAM = 0x9E3779B97F4A7C15, 517, 1


@functools.lru_cache(maxsize=None)
def expected(p, pos):
    """oth[0 .. p] as the routines must leave it, uint16[p + 1]"""
    i = np.arange(1, p, dtype=np.uint64)
    u = R.uniforms(SEED, CHAIN, STREAM, np.uint64(pos) + np.uint64(p - 1) - i)
    out = np.full(p + 1, P.SENTINEL, np.uint16)
    out[1:p] = np.floor((i.astype(np.float64) + 1.0) * u).astype(np.uint16)
    out.setflags(write=False)
    return out


def check_expected():
    """the expected arrays, on the CPU: in range, and the two parities of a position agree on which
    uniform serves which step -- step i from pos + 1 and step i - 1 from pos share theirs, so the
    targets differ by at most the one more candidate the longer range has"""
    for p in SIZES:
        for pos in POSITIONS:
            e = expected(p, pos)
            assert e.shape == (p + 1,) and e[0] == P.SENTINEL and e[p] == P.SENTINEL
            assert np.all(e[1:p].astype(np.int64) <= np.arange(1, p)), (p, pos)
        for pos in (0, 510, 2 ** 32 - 3):
            lo = expected(p, pos)[1:p - 1].astype(np.int64)        # floor((i + 1) u), i = 1 .. p-2
            hi = expected(p, pos + 1)[2:p].astype(np.int64)        # floor((i + 2) u), the same u
            assert np.all((hi == lo) | (hi == lo + 1)), (p, pos)
    # the uniforms themselves are not all alike: the largest size draws targets all over its range
    e = expected(513, 1)[1:513]
    assert np.unique(e).size > 100


def test_expected_targets_are_consistent():
    check_expected()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    check_expected()   # (before anything goes to the GPU)
    return P.load(tmp_path_factory.mktemp("shuffle_targets_probe"))


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("p", SIZES)
def test_targets_match_the_stream(lib, p, waves):
    for pos in POSITIONS:
        want = expected(p, pos)
        for forked, name in ((1, "fork_shuffle_targets"), (0, "shuffle_targets")):
            got = P.targets(lib, waves, forked, p, SEED, CHAIN, STREAM, pos)
            assert got[0] == P.SENTINEL and got[p] == P.SENTINEL, (name, p, waves, pos, int(got[0]), int(got[p]))
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s, p %d, %d wavefronts, pos %d: %d entries differ, first %d" % (
                name, p, waves, pos, bad.size, bad[0])
            assert np.array_equal(got, want)


@pytest.mark.gpu
def test_bad_requests_are_refused(lib):
    out = np.zeros(8, np.uint16)
    vp = out.ctypes.data
    assert lib.st_targets(3, 1, 4, 1, 0, 0, 0, 0, 0xFFFF, vp, 8) == P.BAD_REQUEST
    assert lib.st_targets(2, 1, 1, 1, 0, 0, 0, 0, 0xFFFF, vp, 8) == P.BAD_REQUEST
    assert lib.st_targets(2, 1, 4097, 1, 0, 0, 0, 0, 0xFFFF, vp, 8) == P.BAD_REQUEST
    assert lib.st_targets(2, 1, 8, 1, 0, 0, 0, 0, 0xFFFF, vp, 8) == P.BAD_REQUEST   # (p + 1 entries are needed)
