"""A vectorised reference of the device's random-number streams (boom_amd/csrc/device_rng.h)
and of the state stream's normals (stream_normals.h), for the tests that call those headers
directly.  Pinned on the oracle and on the published Philox vectors by tests/test_philox_ref.py.

Stream layout: uniform number i of stream (seed, chain, stream id) is 64-bit half (i & 1) of
Philox4x32-10 block (i >> 1) -- counter (block low word, block high word, chain, stream id),
key (seed low word, seed high word) --, mapped to [0, 1) as (x >> 11) * 2^-53.

State stream: draw number g owns the positions [256 g, 256 (g + 1)); draws 2 j and 2 j + 1 are
the Box-Muller pair of the two uniforms at position 512 j, i.e. of block 128 (g & ~1):
    R = sqrt(-2 log(1 - u1)),  theta = fl64(6.283185307179586 u2),
    z_{2j} = R cos(theta),  z_{2j+1} = R sin(theta)
1 - u1 is exact in double; theta is rounded to double because that product is part of the
operation; everything else is evaluated in numpy.longdouble."""
import numpy as np

LD = np.longdouble
M32 = np.uint64(0xFFFFFFFF)
STATE_SLOT_STRIDE = 256
SPILL_STREAM_BIT = 0x80000000
SPILL_SHIFT = 20


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """the four output words (uint64 arrays holding 32-bit values) of counters c0..c3, key k0, k1"""
    c0, c1, c2, c3 = np.broadcast_arrays(_u64(c0), _u64(c1), _u64(c2), _u64(c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> s32) ^ c1 ^ k0
        n2 = (p0 >> s32) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & M32, n2, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def block_halves(seed, chain, stream, block):
    """the two 53-bit integers (x >> 11) of every block of the stream"""
    block = _u64(block)
    seed = int(seed)
    o0, o1, o2, o3 = philox4x32_10(block & M32, block >> np.uint64(32), np.uint64(chain), np.uint64(stream),
                                   seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    s11 = np.uint64(11)
    return (o0 | (o1 << np.uint64(32))) >> s11, (o2 | (o3 << np.uint64(32))) >> s11


def uniform_ints(seed, chain, stream, pos):
    """the 53-bit integer of every stream position in pos"""
    pos = _u64(pos)
    h0, h1 = block_halves(seed, chain, stream, pos >> np.uint64(1))
    return np.where((pos & np.uint64(1)) != 0, h1, h0)


def uniforms(seed, chain, stream, pos):
    """the uniform at every stream position in pos, as float64 (exact)"""
    return uniform_ints(seed, chain, stream, pos).astype(np.float64) * 2.0 ** -53


def uniform_bits(seed, chain, stream, pos):
    """the same as the bit patterns of the doubles"""
    return uniforms(seed, chain, stream, pos).view(np.uint64)


def slot_positions(index, stride, serve, n):
    """(spilled, position) of the n numbers a slot's reader hands out: the first `serve` at
    index * stride ..., the rest in the spill stream (stream id | SPILL_STREAM_BIT) from
    index << SPILL_SHIFT"""
    i = np.arange(n, dtype=np.uint64)
    spilled = i >= np.uint64(serve)
    pos = np.where(spilled, np.uint64(int(index) << SPILL_SHIFT) + i - np.uint64(serve),
                   np.uint64(int(index) * int(stride)) + i)
    return spilled, pos


def state_normals(seed, chain, draws, stream=2):
    """(z, R) of the state stream's draws with the global numbers in `draws`, in longdouble"""
    g = _u64(draws)
    leader = g & ~np.uint64(1)
    h0, h1 = block_halves(seed, chain, stream, leader * np.uint64(STATE_SLOT_STRIDE // 2))
    u1 = h0.astype(np.float64) * 2.0 ** -53
    u2 = h1.astype(np.float64) * 2.0 ** -53
    R = np.sqrt(LD(-2.0) * np.log((1.0 - u1).astype(LD)))
    theta = (6.283185307179586 * u2).astype(LD)
    z = np.where((g & np.uint64(1)) != 0, R * np.sin(theta), R * np.cos(theta))
    return z, R


def normal_statistics(z, first):
    """What the advisor asked of the state stream's normals, for consecutive draws of which the
    first has the global number `first` (its parity says where the pairs lie): a dict of
    z-scores under the large-sample standard errors, and the Kolmogorov-Smirnov p-value
    against N(0, 1)."""
    from scipy import stats
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    m = z.mean()
    d = z - m
    v = np.mean(d * d)
    zp = z[int(first) & 1:]
    zp = zp[:zp.size & ~1]
    a, b = zp[0::2], zp[1::2]

    def corr(x, y):
        return np.corrcoef(x, y)[0, 1] * np.sqrt(x.size)
    out = {
        "mean": m * np.sqrt(n),
        "variance": (v - 1.0) / np.sqrt(2.0 / n),
        "skewness": np.mean(d ** 3) / v ** 1.5 / np.sqrt(6.0 / n),
        "excess kurtosis": (np.mean(d ** 4) / v ** 2 - 3.0) / np.sqrt(24.0 / n),
        "pair halves": corr(a, b),
        "pair halves squared": corr(a * a, b * b),
        "second half, next first half": corr(b[:-1], a[1:]),
        "lag 2": corr(z[:-2], z[2:]),
    }
    return {k: float(x) for k, x in out.items()}, float(stats.kstest(z, "norm").pvalue)


# (seed, chain, first draw) of the distribution checks: fixed, so nothing there is random
DISTRIBUTION_INPUTS = [(2024, 7, 0), (99, 3, 1), (8675309, 1023, 2 ** 25 - 5)]
DISTRIBUTION_N = 2 ** 18


def distribution_failures(z, first):
    """(what misses |z| < 3.0 or KS p > 0.01, the z-scores, the p-value)"""
    st, p = normal_statistics(z, first)
    bad = {k: v for k, v in st.items() if not abs(v) < 3.0}
    if not p > 0.01:
        bad["KS p"] = p
    return bad, st, p
