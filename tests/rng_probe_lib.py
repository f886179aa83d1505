"""ctypes loader of tests/cpp/rng_probe.hip (build/librng_probe.so, built by `make -C tests/cpp`):
the product's stream readers and state-stream normals, launched directly.  Every call runs the
kernel TWICE from the same inputs and requires identical bytes back (repeatability), then
returns the arrays of the second run."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64
SENT_BITS = np.uint64(0x7FF8C0DEC0DEC0DE)            # a NaN with a payload: no draw gives it
SENT_I32 = np.int32(-77777777)
_vp, _sz, _u32, _u64, _i64, _int = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int64, C.c_int
OP_DRAW, OP_SEEK, OP_SEQ_ROUND_TRIP = 0, 1, 2


def load():
    path = os.path.join(HERE, "cpp", "build", "librng_probe.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "build/librng_probe.so"])
    lib = C.CDLL(path)
    key = [_u32, _u32, _u32, _u32]
    sig = {
        "rp_state_slot_stride": [], "rp_lm_tp": [], "rp_sn_sub": [], "rp_chain_ok": [],
        "rp_views": key + [_u64, _vp, _int, _vp, _sz, _vp, _sz],
        "rp_slot": key + [_u64, _u32, _u32, _i64, _vp, _sz, _vp, _sz],
        "rp_normals_in_order": key + [_u64, _int, _int, _int, _vp, _sz, _sz, _vp, _vp, _sz],
        "rp_normals_lm": key + [_u64, _int, _int, _int, _int, _int, _int, _vp, _sz, _sz, _vp, _vp, _sz],
        "rp_share": [_u32, _u32, _u32, _u32, _u32, _int, _int, _int, _int, _int, _int, _vp, _int, _vp, _sz],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = args
    return lib


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_vp)


def seed_words(seed):
    return int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF


def sentinel_u64(count):
    return np.full(count, SENT_BITS, np.uint64)


def _twice(call, make):
    """run `call` on two fresh sets of arrays from `make`; identical bytes; the second set"""
    first = make()
    assert call(*first) == 0
    second = make()
    assert call(*second) == 0
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes(), "two runs of one kernel differ"
    return second


def views(lib, seed, chain, stream, pos0, ops):
    """ops: [(code, argument)]; returns (numbers[view, lane 0 / lane 63, i] as uint64 bit
    patterns, final positions[view, lane 0 / lane 63]); guards checked here"""
    ops_a = np.array(ops, np.int64).reshape(-1, 2)
    total = int(sum(a for c, a in ops if c != OP_SEEK))
    k0, k1 = seed_words(seed)

    def make():
        return sentinel_u64(6 * total + GUARD), sentinel_u64(6 + GUARD)

    def call(out, pos):
        return lib.rp_views(k0, k1, chain, stream, pos0, _p(ops_a), len(ops), _p(out), out.size, _p(pos), pos.size)
    out, pos = _twice(call, make)
    assert np.all(out[6 * total:] == SENT_BITS) and np.all(pos[6:] == SENT_BITS), "written past the end"
    return out[:6 * total].reshape(3, 2, total), pos[:6].reshape(3, 2)


def slot(lib, seed, chain, stream, index, stride, serve, n):
    """returns (numbers[Seq / Pair, lane 0 / lane 63, i], info[Seq / Pair, lane, (pos, stream, overran)])"""
    k0, k1 = seed_words(seed)

    def make():
        return sentinel_u64(4 * n + GUARD), sentinel_u64(12 + GUARD)

    def call(out, info):
        return lib.rp_slot(k0, k1, chain, stream, index, stride, serve, n, _p(out), out.size, _p(info), info.size)
    out, info = _twice(call, make)
    assert np.all(out[4 * n:] == SENT_BITS) and np.all(info[12:] == SENT_BITS), "written past the end"
    return out[:4 * n].reshape(2, 2, n), info[:12].reshape(2, 2, 3)


def _normals(call, count, threads, one_wave, chain_ok):
    def make():
        return sentinel_u64(GUARD + count + GUARD), sentinel_u64(1), np.full(threads + GUARD, SENT_I32, np.int32)
    szz, pos, status = _twice(call, make)
    assert np.all(szz[:GUARD] == SENT_BITS) and np.all(szz[GUARD + count:] == SENT_BITS), "a guard band was written"
    live = 64 if one_wave else threads
    assert np.all(status[:live] == chain_ok) and np.all(status[live:] == SENT_I32)
    return szz[GUARD:GUARD + count], int(pos[0])


def normals_in_order(lib, seed, chain, bpos0, N, threads, one_wave, stream=2):
    """returns (szz as uint64 bit patterns, *pos_out); guards and status checked here"""
    k0, k1 = seed_words(seed)

    def call(szz, pos, status):
        return lib.rp_normals_in_order(k0, k1, chain, stream, bpos0, N, threads, int(one_wave), _p(szz), szz.size,
                                       GUARD, _p(pos), _p(status), status.size)
    return _normals(call, N, threads, one_wave, lib.rp_chain_ok())


def normals_lm(lib, seed, chain, bpos0, T, dI, dL, dH, threads, one_wave, stream=2):
    k0, k1 = seed_words(seed)

    def call(szz, pos, status):
        return lib.rp_normals_lm(k0, k1, chain, stream, bpos0, T, dI, dL, dH, threads, int(one_wave), _p(szz),
                                 szz.size, GUARD, _p(pos), _p(status), status.size)
    return _normals(call, 2 * lib.rp_lm_tp(), threads, one_wave, lib.rp_chain_ok())


def share(lib, seed, chain, bpos0, T, dI, dL, dH, zbuf, chunks):
    """the sub-chunks `chunks` of a shared job whose words say position bpos0; the scratch
    array is that of one chain, pitch LM_TP; returns the normals' 2 LM_TP slots"""
    k0, k1 = seed_words(seed)
    TP = lib.rp_lm_tp()
    first = (5 + 2 * zbuf) * TP
    lst = np.array(chunks, np.int32)

    def make():
        return (sentinel_u64(first + 2 * TP + GUARD),)

    def call(scratch):
        return lib.rp_share(k0, k1, chain, bpos0 & 0xFFFFFFFF, bpos0 >> 32, T, dI, dL, dH, zbuf, TP, _p(lst), lst.size,
                            _p(scratch), scratch.size)
    (scratch,) = _twice(call, make)
    assert np.all(scratch[:first] == SENT_BITS) and np.all(scratch[first + 2 * TP:] == SENT_BITS), \
        "written outside the normals buffer"
    return scratch[first:first + 2 * TP]
