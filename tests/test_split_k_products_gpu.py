"""The split-K matrix-core products (boom_amd/csrc/xtwx_cols_kernel.hip) and predict_kernel,
called directly through the host-only probe tests/cpp/kernel_probe.cpp and compared with the
same product written plainly in numpy.longdouble -- at the 64-request tile, the 128-variable
tile, the 16-row staging step and the plane length (2048 rows, 128 for the bsts X'e).

Tolerance, derived and not tuned: a device result is a sum of n products whose partial sums
meet in nplanes planes, plus at most one more rounding per term (the gather form rounds
w_i x_ig before the product) -- every term passes through at most m = n + nplanes + 1
rounded operations, so |got - ref| <= gamma_m sum|terms| with gamma_m = m u / (1 - m u),
u = 2^-53, and sum|terms| formed per element in longdouble; where a base is added, its share
of the last rounding, |base| u, comes on top.  The reference's own error is gamma_m at
u = 2^-64, 2^-11 of the bound: the bound is widened by 2^-10 for it.  A dropped, doubled or
misplaced row or tile is off by O(1) terms, twelve orders above the bound.

Every output and workspace goes in filled with a sentinel and with a guard band behind its
logical end, and comes back whole: nothing may be written outside."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
U53 = 2.0 ** -53
GUARD = 96
SENT_BITS = np.uint64(0xC0DEC0DEC0DEC0DE)            # a finite double no product gives
SENT = np.array([SENT_BITS], np.uint64).view(np.float64)[0]
SENT_I32 = np.int32(-77777777)
SENT_U32 = np.uint32(0xDEADBEEF)
_vp = C.c_void_p
_sz = C.c_size_t


@pytest.fixture(scope="module")
def probe():
    assert np.finfo(LD).eps <= 2.0 ** -63, "the reference needs an extended-precision long double"
    path = os.path.join(HERE, "cpp", "build", "libkernel_probe.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "build/libkernel_probe.so"])
    lib = C.CDLL(path)
    sig = {
        "kp_planes": [C.c_int64],
        "kp_xte_planes": [C.c_int64],
        "kp_rows_times_columns": [_vp, _sz, C.c_int, _vp, _sz, C.c_int64, C.c_int, _vp, _sz, _vp, _sz, _vp, _sz],
        "kp_xte_tiled": [_vp, _sz, C.c_int64, C.c_int, _vp, _sz, C.c_int64, C.c_int, _vp, _sz, _vp, _sz],
        "kp_xtwx_cols": [_vp, _sz, C.c_int64, C.c_int, _vp, _sz, _vp, C.c_int, _vp, _sz, _vp, _sz, _vp, _sz,
                         C.c_int, _vp, _sz],
        "kp_xtwx_cols_start": [_vp, _sz, C.c_int, C.c_int, _vp, _sz, _vp, _vp, _sz, C.c_int],
        "kp_square": [_vp, _sz, _vp, _sz],
        "kp_predict": [_vp, _sz, _vp, _sz, _vp, _sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                       _vp, _sz, C.c_int, _vp, _sz],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = args
    return lib


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_vp)


def _n(a):
    return 0 if a is None else a.size


def sentinel(count):
    return np.full(count + GUARD, SENT)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def untouched(a):
    return bool(np.all(bits(a) == SENT_BITS))


def gamma_m(m):
    return m * U53 / (1.0 - m * U53)


def assert_within(got, ref, mag, m, extra=None, tag=None):
    """|got - ref| <= gamma_m mag (1 + 2^-10) (+ extra), element by element"""
    bound = LD(gamma_m(m) * (1.0 + 2.0 ** -10)) * mag
    if extra is not None:
        bound = bound + extra
    err = np.abs(got.astype(LD) - ref)
    assert np.all(np.isfinite(got)), tag
    share = float(np.max(err / np.maximum(bound, LD(1e-300))))
    print("%s: largest share of the bound %.3g" % (tag, share))
    assert np.all(err <= bound), (tag, share)


def normals(seed, *shape):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)


# ---------------------------------------------------------------- rows_times_columns
def rows_times_columns(probe, U, B, diag_base=None):
    """out and planes as they come back (guard bands included)"""
    R, n = U.shape
    p = B.shape[0]
    nplanes = probe.kp_planes(n)
    out, planes = sentinel(R * p), sentinel(nplanes * R * p)
    rc = probe.kp_rows_times_columns(_p(U), U.size, R, _p(B), B.size, n, p, _p(diag_base), _n(diag_base),
                                     _p(out), out.size, _p(planes), planes.size)
    assert rc == 0, rc
    return out, planes, nplanes


ROWS_SHAPES = [(1, 1, 1), (3, 5, 15), (64, 128, 16), (65, 129, 17), (63, 127, 2047), (2, 130, 2048), (70, 3, 2049),
               (5, 260, 4100)]


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("shape", ROWS_SHAPES)
def test_rows_times_columns(probe, shape, with_base):
    R, p, n = shape
    U, B = normals(1000 + n + R, R, n), normals(2000 + n + p, p, n)
    base = None
    if with_base:
        # only the diagonal may be read
        base = np.full((p, p), np.nan)
        base[np.arange(p), np.arange(p)] = normals(3000 + p, p)
    out, planes, nplanes = rows_times_columns(probe, U, B, base)
    assert nplanes == (n + 2047) // 2048
    Ul, Bl = U.astype(LD), B.astype(LD)
    ref, mag = Ul @ Bl.T, np.abs(Ul) @ np.abs(Bl).T
    extra = None
    if with_base:
        d = np.diag(base).astype(LD)
        ref = ref + d[None, :]
        extra = np.abs(d)[None, :] * LD(U53) * np.ones((R, 1), LD)
    assert_within(out[:R * p].reshape(R, p), ref, mag, n + nplanes + 1, extra, ("rows", shape, with_base))
    assert untouched(out[R * p:]) and untouched(planes[nplanes * R * p:])
    assert not np.any(bits(planes[:nplanes * R * p]) == SENT_BITS)
    # the same call again: the same bits
    out2, planes2, _ = rows_times_columns(probe, U, B, base)
    assert same_bits(out, out2) and same_bits(planes, planes2)


def test_rows_times_columns_batch_invariance(probe):
    """a row's products do not depend on how many rows share the launch"""
    R, p, n = 65, 129, 2049
    U, B = normals(11, R, n), normals(12, p, n)
    out, _, _ = rows_times_columns(probe, U, B)
    out = out[:R * p].reshape(R, p)
    for r in (0, 63, 64):
        alone, _, _ = rows_times_columns(probe, np.ascontiguousarray(U[r:r + 1]), B)
        assert same_bits(alone[:p], out[r]), r


# ---------------------------------------------------------------- xte_tiled
def xte_tiled(probe, Upad, n, B, want_out=True):
    R, ldu = Upad.shape
    p = B.shape[0]
    nplanes = probe.kp_xte_planes(n)
    out = sentinel(R * p) if want_out else None
    planes = sentinel(nplanes * R * p)
    rc = probe.kp_xte_tiled(_p(Upad), Upad.size, ldu, R, _p(B), B.size, n, p, _p(out), _n(out), _p(planes),
                            planes.size)
    assert rc == 0, rc
    return out, planes, nplanes


def padded_rows(U, pad=7):
    """rows of U `pad` doubles further apart, NaN in the gaps"""
    R, n = U.shape
    Upad = np.full((R, n + pad), np.nan)
    Upad[:, :n] = U
    return Upad


def host_plane_sum(planes, nplanes, count):
    z = planes[:nplanes * count].reshape(nplanes, count)
    a = z[0].copy()
    for k in range(1, nplanes):
        a = a + z[k]
    return a


@pytest.mark.parametrize("p", [3, 129])
@pytest.mark.parametrize("R", [1, 65])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 300])
def test_xte_tiled(probe, n, R, p):
    U, B = normals(4000 + n + R, R, n), normals(5000 + n + p, p, n)
    Upad = padded_rows(U)
    out, planes, nplanes = xte_tiled(probe, Upad, n, B)
    assert nplanes == (n + 127) // 128
    Ul, Bl = U.astype(LD), B.astype(LD)
    assert_within(out[:R * p].reshape(R, p), Ul @ Bl.T, np.abs(Ul) @ np.abs(Bl).T, n + nplanes + 1,
                  tag=("xte", n, R, p))
    assert untouched(out[R * p:]) and untouched(planes[nplanes * R * p:])
    # planes only: the same planes, and their sum in plane order is `out` bit for bit
    none, planes_only, _ = xte_tiled(probe, Upad, n, B, want_out=False)
    assert none is None
    assert same_bits(planes, planes_only)
    assert same_bits(host_plane_sum(planes_only, nplanes, R * p), out[:R * p])
    # the same call again: the same bits
    out2, planes2, _ = xte_tiled(probe, Upad, n, B)
    assert same_bits(out, out2) and same_bits(planes, planes2)


# ---------------------------------------------------------------- xtwx_cols (+ its request list)
def cols_start(probe, gam, stale=True):
    chains, p = gam.shape
    words = (p + 31) // 32
    total = int(gam.astype(bool).sum())
    req = np.full(2 * total + GUARD, SENT_I32, np.int32)
    count = np.full(1, SENT_I32, np.int32)
    valid = np.full(chains * words + GUARD, SENT_U32 if stale else 0, np.uint32)   # (stale bits planted)
    rc = probe.kp_xtwx_cols_start(_p(gam), gam.size, chains, p, _p(req), req.size, _p(count), _p(valid),
                                  valid.size, words)
    assert rc == 0, rc
    return req, int(count[0]), valid, words


def check_request_list(gam, req, count, valid, words):
    chains, p = gam.shape
    assert count == int(gam.astype(bool).sum())
    assert np.all(req[2 * count:] == SENT_I32)
    pairs = req[:2 * count].reshape(count, 2)
    want = {(c, j) for c, j in zip(*np.nonzero(gam))}
    assert {(int(c), int(j)) for c, j in pairs} == want and len(want) == count
    # each chain's entries contiguous and ascending
    seen, at = set(), 0
    while at < count:
        c = int(pairs[at, 0])
        assert c not in seen, c
        seen.add(c)
        end = at
        while end < count and pairs[end, 0] == c:
            end += 1
        assert np.all(np.diff(pairs[at:end, 1]) > 0), c
        assert end - at == int(gam[c].astype(bool).sum()), c
        at = end
    # every valid word cleared, stale bits included; nothing behind them
    assert np.all(valid[:chains * words] == 0)
    assert np.all(valid[chains * words:] == SENT_U32)


def cols(probe, Xt, w, pairs, base, valid=None):
    """V (chains x p x p + guard), valid and planes after launch_xtwx_cols on the requests `pairs`"""
    p, n = Xt.shape
    chains = w.shape[0]
    words = (p + 31) // 32
    R = len(pairs)
    nplanes = probe.kp_planes(n)
    req = np.ascontiguousarray(pairs, dtype=np.int32)
    V, planes = sentinel(chains * p * p), sentinel(nplanes * R * p)
    if valid is None:
        valid = np.zeros(chains * words + GUARD, np.uint32)
        valid[chains * words:] = SENT_U32
    valid = valid.copy()
    rc = probe.kp_xtwx_cols(_p(Xt), Xt.size, n, p, _p(w), w.size, _p(req), R, _p(base), base.size, _p(V), V.size,
                            _p(valid), valid.size, words, _p(planes), planes.size)
    assert rc == 0, rc
    return V, valid, planes, nplanes


def make_gammas(seed, chains, p):
    """random models of about three variables; with three chains or more one that includes nothing
    and one that includes everything"""
    rng = np.random.Generator(np.random.PCG64(seed))
    gam = (rng.random((chains, p)) < min(0.5, 3.0 / p)).astype(np.uint8)
    gam[0, rng.integers(p)] = 1
    if chains >= 3:
        gam[1] = 0
        gam[chains - 1] = 1
    return gam


@pytest.mark.parametrize("n", [17, 2049])
@pytest.mark.parametrize("p", [5, 129, 260])
@pytest.mark.parametrize("chains", [1, 3, 70])
def test_xtwx_cols_and_request_list(probe, chains, p, n):
    seed = 6000 + 1000 * chains + 10 * p + n
    Xt, w, base = normals(seed, p, n), np.abs(normals(seed + 1, chains, n)), normals(seed + 2, p, p)
    gam = make_gammas(seed + 3, chains, p)
    req, count, valid0, words = cols_start(probe, gam)
    check_request_list(gam, req, count, valid0, words)
    pairs = req[:2 * count].reshape(count, 2)
    V, valid, planes, nplanes = cols(probe, Xt, w, pairs, base, valid0)
    # values: V_c[g, .] = base[g, .] + X'(w_c o x_g)
    Xl, m = Xt.astype(LD), n + nplanes + 1
    Vv = V[:chains * p * p].reshape(chains, p, p)
    for c in range(chains):
        inc = np.flatnonzero(gam[c])
        if inc.size:
            wx = w[c].astype(LD)[None, :] * Xl[inc]
            ref = wx @ Xl.T + base[inc].astype(LD)
            assert_within(Vv[c, inc], ref, np.abs(wx) @ np.abs(Xl).T, m, np.abs(base[inc]).astype(LD) * LD(U53),
                          ("cols", chains, p, n, c))
        # the vectors nobody asked for are untouched
        assert untouched(Vv[c, np.flatnonzero(gam[c] == 0)]), c
    assert untouched(V[chains * p * p:]) and untouched(planes[nplanes * count * p:])
    # the valid words hold exactly the requested bits
    want = np.zeros((chains, words), np.uint32)
    for c, j in pairs:
        want[int(c), int(j) >> 5] |= np.uint32(1 << (int(j) & 31))
    assert np.array_equal(valid[:chains * words].reshape(chains, words), want)
    assert np.all(valid[chains * words:] == SENT_U32)
    # the same calls again: the same list for each chain, the same bits
    V2, valid2, planes2, _ = cols(probe, Xt, w, pairs, base, valid0)
    assert same_bits(V, V2) and np.array_equal(valid, valid2) and same_bits(planes, planes2)


def test_xtwx_cols_batch_invariance(probe):
    """header of xtwx_cols_kernel.hip: "an element's value depends on n alone -- not on how many
    requests share the launch": one request's vector alone and at positions 0, 63, 64 and 129 of a
    130-request list, bit for bit"""
    chains, p, n = 2, 129, 2049
    Xt, w, base = normals(21, p, n), np.abs(normals(22, chains, n)), normals(23, p, p)
    target = (1, 77)
    alone, _, _, _ = cols(probe, Xt, w, [target], base)
    alone = alone[:chains * p * p].reshape(chains, p, p)[target]
    assert not np.any(bits(alone) == SENT_BITS)
    others = [(c, j) for j in range(p) for c in range(chains) if (c, j) != target]
    for pos in (0, 63, 64, 129):
        pairs = others[:129]
        pairs.insert(pos, target)
        assert len(pairs) == 130 and pairs[pos] == target
        V, _, _, _ = cols(probe, Xt, w, pairs, base)
        assert same_bits(V[:chains * p * p].reshape(chains, p, p)[target], alone), pos


# ---------------------------------------------------------------- padding lanes read but discard
@pytest.mark.parametrize("n", [17, 2049])
def test_padding_lanes_are_discarded_plain(probe, n):
    """The kernel loads row 0 / column 0 for the tile lanes out of range and the plane's last row
    for the steps out of range, then masks: a NaN there reaches only the outputs it belongs to
    (partial tiles in every dimension), and every other output keeps its bits."""
    R, p = 65, 129
    U, B = normals(31 + n, R, n), normals(32 + n, p, n)
    for runner in ("rows", "xte"):
        def run(Um, Bm):
            if runner == "rows":
                o, _, _ = rows_times_columns(probe, Um, Bm)
            else:
                o, _, _ = xte_tiled(probe, padded_rows(Um), n, Bm)
            assert untouched(o[R * p:])
            return o[:R * p].reshape(R, p)
        clean = run(U, B)
        assert np.all(np.isfinite(clean))

        def only(out, nan_mask):
            assert np.array_equal(np.isnan(out), nan_mask), runner
            assert same_bits(out[~nan_mask], clean[~nan_mask]), runner
        mask = np.zeros((R, p), bool)
        # column 0 of X
        Bm = B.copy()
        Bm[0, :] = np.nan
        mask[:] = False
        mask[:, 0] = True
        only(run(U, Bm), mask)
        # row 0 of U
        Um = U.copy()
        Um[0, :] = np.nan
        mask[:] = False
        mask[0, :] = True
        only(run(Um, B), mask)
        # the last row of one column
        Bm = B.copy()
        Bm[100, n - 1] = np.nan
        mask[:] = False
        mask[:, 100] = True
        only(run(U, Bm), mask)


@pytest.mark.parametrize("n", [17, 2049])
def test_padding_lanes_are_discarded_gather(probe, n):
    """the same for the gather form: 65 requests, of which request 0 names variable 0"""
    chains, p = 5, 129
    Xt, w, base = normals(41 + n, p, n), np.abs(normals(42 + n, chains, n)), normals(43 + n, p, p)
    pairs = [(c, j) for c in range(chains) for j in (0, 3, 64, 100, 127, 128)]
    pairs += [(c, off + c) for off in (10, 20, 30, 40, 50, 70, 80) for c in range(chains)]
    assert len(pairs) == 65 and len(set(pairs)) == 65 and pairs[0] == (0, 0)
    rows = tuple(np.array(pairs).T)

    def run(Xm, wm):
        V, _, _, _ = cols(probe, Xm, wm, pairs, base)
        assert untouched(V[chains * p * p:])
        return V[:chains * p * p].reshape(chains, p, p)[rows]      # 65 x p, in request order
    clean = run(Xt, w)
    assert np.all(np.isfinite(clean))
    req_c, req_g = np.array(pairs).T

    def only(out, nan_mask):
        assert np.array_equal(np.isnan(out), nan_mask)
        assert same_bits(out[~nan_mask], clean[~nan_mask])
    # column 0 of X: element j = 0 of every vector, and the whole vector of the requests for g = 0
    Xm = Xt.copy()
    Xm[0, :] = np.nan
    mask = np.zeros((65, p), bool)
    mask[:, 0] = True
    mask[req_g == 0, :] = True
    only(run(Xm, w), mask)
    # the weights of request 0's chain: that chain's requests
    wm = w.copy()
    wm[0, :] = np.nan
    mask[:] = False
    mask[req_c == 0, :] = True
    only(run(Xt, wm), mask)
    # the last row of one column
    Xm = Xt.copy()
    Xm[100, n - 1] = np.nan
    mask[:] = False
    mask[:, 100] = True
    mask[req_g == 100, :] = True
    only(run(Xm, w), mask)


# ---------------------------------------------------------------- launch_square
def test_square(probe):
    for count in (1, 255, 256, 257):
        x = normals(50 + count, count)
        out = sentinel(count)
        assert probe.kp_square(_p(x), count, _p(out), out.size) == 0
        assert same_bits(out[:count], x * x) and untouched(out[count:]), count


# ---------------------------------------------------------------- predict_kernel
@pytest.mark.parametrize("nnew", [1, 255, 256, 257])
@pytest.mark.parametrize("p", [5, 40000])
@pytest.mark.parametrize("cap", [64, 128])
def test_predict_kernel_on_a_synthetic_record(probe, cap, p, nnew):
    """out[c, d, i] = sum_{m < min(k, cap)} beta_m newX[i, var_m] over the rows [first_draw,
    first_draw + ndraws) of the record; everything else in the record is NaN / index 65535 and
    must not reach the output.  Bound: gamma_k sum|beta x|."""
    chains, stride, first, ndraws = 3, 7, 2, 4
    rng = np.random.Generator(np.random.PCG64(7000 + cap + p + nnew))
    newXt = rng.standard_normal((p, nnew))                       # column-major nnew x p
    ks = np.full((chains, stride), float(cap))
    idx = np.full((chains, stride, cap), 65535, np.uint16)
    beta = np.full((chains, stride, cap), np.nan)
    k_of = [0, 1, cap, cap + 5]
    for c in range(chains):
        for d in range(ndraws):
            k = k_of[(c + d) % 4]
            ks[c, first + d] = k
            kk = min(k, cap)                                     # (the kernel clamps)
            idx[c, first + d, :kk] = rng.integers(0, p, kk)
            beta[c, first + d, :kk] = rng.standard_normal(kk)
    out = sentinel(chains * ndraws * nnew)
    rc = probe.kp_predict(_p(ks), ks.size, _p(idx), idx.size, _p(beta), beta.size, stride, cap, first, ndraws,
                          chains, p, _p(newXt), newXt.size, nnew, _p(out), out.size)
    assert rc == 0, rc
    got = out[:chains * ndraws * nnew].reshape(chains, ndraws, nnew)
    assert untouched(out[chains * ndraws * nnew:])
    assert sorted({k_of[(c + d) % 4] for c in range(chains) for d in range(ndraws)}) == k_of
    for c in range(chains):
        for d in range(ndraws):
            kk = min(int(ks[c, first + d]), cap)
            if kk == 0:
                assert np.all(bits(got[c, d]) == 0), (c, d)
                continue
            terms = beta[c, first + d, :kk].astype(LD)[:, None] * newXt[idx[c, first + d, :kk]].astype(LD)
            assert_within(got[c, d], terms.sum(axis=0), np.abs(terms).sum(axis=0), kk, tag=("predict", cap, p, nnew, c, d))
