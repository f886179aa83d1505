"""Pins tests/philox_ref.py -- the reference that the direct device tests of the stream readers
(test_stream_views_gpu.py) and of the state stream's normals (test_stream_normals_gpu.py)
compare with -- on the published Philox vectors and on the oracle.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import philox_ref as R
from philox_ref import DISTRIBUTION_INPUTS, DISTRIBUTION_N, distribution_failures


def test_philox_known_answers():
    """the Random123 kat_vectors of test_oracle_golden.py"""
    vec = [
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
         (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for ctr, key, want in vec:
        assert tuple(int(x[0]) for x in R.philox4x32_10(*ctr, *key)) == want
    # ... and all three at once: the arrays are element-wise
    got = R.philox4x32_10(*[np.array([v[0][i] for v in vec[::2]], np.uint64) for i in range(4)], 0, 0)
    assert int(got[0][0]) == 0x6627e8d5 and int(got[0][1]) != 0xd16cfe09   # (the third has another key)


def test_blocks_match_the_oracle(oracle):
    rng = np.random.Generator(np.random.PCG64(5))
    ctr = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64)
    ctr[0] = 0xffffffff
    k0, k1 = 0x9abcdef0, 0x12345678
    got = np.stack(R.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], k0, k1), axis=1)
    for i in range(ctr.shape[0]):
        c = (C.c_uint32 * 4)(*[int(x) for x in ctr[i]])
        k = (C.c_uint32 * 2)(k0, k1)
        o = (C.c_uint32 * 4)()
        oracle.lib.bo_philox4x32_10(c, k, o)
        assert tuple(o) == tuple(int(x) for x in got[i])


@pytest.mark.parametrize("seed,chain,stream", [(123, 5, 0), ((0xfeedface << 32) | 0x1234, 0xffffffff, 2 | 0x80000000),
                                               (2024, 1023, 7)])
@pytest.mark.parametrize("pos", [0, 1, 127, 2 ** 32 - 1, 2 ** 33 - 2, 2 ** 33 + 5, 2 ** 40 + 1])
def test_stream_layout_matches_the_oracle(oracle, seed, chain, stream, pos):
    """positions below and above 2^33 (the block counter's second word)"""
    want = oracle.uniforms(oracle.rng_philox(seed, chain=chain, stream=stream, pos=pos), 9)
    got = R.uniforms(seed, chain, stream, pos + np.arange(9))
    assert np.array_equal(want.view(np.uint64), got.view(np.uint64))
    assert np.array_equal(got.view(np.uint64), R.uniform_bits(seed, chain, stream, pos + np.arange(9)))


@pytest.mark.parametrize("first", [0, 1, 2 ** 25 - 2, 2 ** 25 - 1])
def test_state_normals_match_the_oracle(oracle, first):
    """bo_rnorm on stream 2, 200 draws from an even and an odd starting slot, below and across
    the draw number at which the pair's block enters the counter's second word.  The oracle
    evaluates the formula in double: one log, one sqrt, one sin or cos and two products, each
    within a unit in the last place of glibc -- 8 units of 2^-53 R leave room to spare, and a
    wrong pair, half or block is off by order 1."""
    L = oracle.lib
    L.bo_rnorm.restype = C.c_double
    L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    r = oracle.rng_philox(99, chain=3, stream=2, pos=256 * first)
    want = np.array([L.bo_rnorm(C.byref(r), 0.0, 1.0) for _ in range(200)])
    z, Rr = R.state_normals(99, 3, first + np.arange(200))
    assert r.pos == 256 * (first + 200)
    assert np.all(np.abs(want.astype(R.LD) - z) <= 8 * R.LD(2.0) ** -53 * Rr)


@pytest.fixture(scope="module")
def reference_statistics():
    out = {}
    for seed, chain, first in DISTRIBUTION_INPUTS:
        z, _ = R.state_normals(seed, chain, first + np.arange(DISTRIBUTION_N, dtype=np.uint64))
        out[seed, chain, first] = distribution_failures(z.astype(np.float64), first)
    return out


@pytest.mark.parametrize("key", DISTRIBUTION_INPUTS)
def test_reference_normals_are_standard_normal(reference_statistics, key):
    """mean, variance, skewness, excess kurtosis, the correlations inside and across pairs and a
    Kolmogorov-Smirnov test of 2^18 draws: every |z| < 3, p > 0.01 (the largest |z| of the three
    inputs: 2.37 -- variance, third input -- and 2.29 -- squares of a pair, first input; KS
    p-values 0.73, 0.51, 0.23)"""
    bad, st, p = reference_statistics[key]
    assert not bad, (key, st, p)
