"""parallel_shuffle (boom_amd/csrc/ssvs_device.h) launched directly on one wavefront
(tests/cpp/shuffle_probe.hip) and compared, exactly, with the serial loop it replaces:
for i = p-1..1: swap(a[i], a[oth[i]])  (cpputil/shuffle.hpp:36-46).  Whole chains see the routine
only through the visiting order of a sweep; here one wrong position fails.

Both template instances (the block mask of the large-model kernel and the plain one).  Sizes at
the edges of a 64-lane round and of the 512-element block a lane's eight steps make, and one
size of several blocks for the mask: 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4096.
Targets, each applied to a starting order that is not the identity: three random draws of
oth[i] in [0, i]; all zero (one chain of links through every step); all self; i - 1; i // 2.
The probe calls the routine a second time on the result of the first (the buffers have swapped,
the work arrays and the spare entry hold what the first call left) and that is compared too."""
import numpy as np
import pytest

import shuffle_probe_lib as P

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4096)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return P.load(tmp_path_factory.mktemp("shuffle_probe"))


def serial(a, oth):
    a = a.copy()
    for i in range(a.size - 1, 0, -1):
        j = int(oth[i])
        a[i], a[j] = a[j], a[i]
    return a


def targets(p):
    i = np.arange(p)
    out = [("random seed %d" % s, np.random.default_rng(1000 * p + s).integers(0, i + 1)) for s in (1, 2, 3)]
    out += [("all zero", np.zeros(p, np.int64)), ("all self", i.copy()), ("i - 1", np.maximum(i - 1, 0)),
            ("i // 2", i // 2)]
    return [(name, t.astype(np.uint16)) for name, t in out]


def start_order(p):
    a = np.random.default_rng(77 + p).permutation(p).astype(np.uint16)
    return a[::-1].copy() if np.array_equal(a, np.arange(p)) else a


@pytest.mark.parametrize("masked", (False, True), ids=("plain", "masked"))
@pytest.mark.parametrize("p", SIZES)
def test_matches_the_serial_swaps(lib, p, masked):
    a0 = start_order(p)
    assert not np.array_equal(a0, np.arange(p))
    for name, oth in targets(p):
        assert np.all(oth <= np.arange(p))
        want1 = serial(a0, oth)
        want2 = serial(want1, oth)
        got1, got2 = P.shuffle(lib, masked, a0, oth)
        bad = np.flatnonzero(got1 != want1)
        assert bad.size == 0, "p %d, %s: %d positions differ, first %d" % (p, name, bad.size, bad[0])
        bad = np.flatnonzero(got2 != want2)
        assert bad.size == 0, "p %d, %s, second call: %d positions differ, first %d" % (p, name, bad.size, bad[0])


def test_bad_requests_are_refused(lib):
    a = np.arange(4, dtype=np.uint16)
    oth = np.array([0, 2, 0, 0], np.uint16)   # oth[1] > 1
    zero = np.zeros(4, np.uint16)
    out = np.zeros(8, np.uint16)
    vp = lambda x: x.ctypes.data
    assert lib.sp_shuffle(0, 4, vp(a), vp(oth), vp(out), 8) == P.BAD_REQUEST
    assert lib.sp_shuffle(0, 4, vp(a), vp(zero), vp(out), 7) == P.BAD_REQUEST
    assert lib.sp_shuffle(0, 1, vp(a), vp(zero), vp(out), 8) == P.BAD_REQUEST
    assert lib.sp_lds_bytes(4097) == P.BAD_REQUEST
    for p in SIZES:   # the five arrays with a spare entry each (last: 32-bit)
        assert lib.sp_lds_bytes(p) >= 12 * (p + 1)
