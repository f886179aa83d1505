"""ctypes loader of tests/cpp/fill_probe.hip (build/libfill_probe.so, built by `make -C tests/cpp`):
the product's diag_inverses, mf_proposal_sums and solve_blocks, launched directly on one
wavefront.  Every call runs the kernel TWICE from the same inputs and requires identical bytes
back (repeatability), checks the guard bands behind every writable buffer, and returns the
arrays of the second run."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64
SENT_BITS = np.uint64(0x7FF8C0DEC0DEC0DE)            # a NaN with a payload no arithmetic gives
BAD_REQUEST = -1
_vp, _sz, _int, _dbl = C.c_void_p, C.c_size_t, C.c_int, C.c_double


def load():
    path = os.path.join(HERE, "cpp", "build", "libfill_probe.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "build/libfill_probe.so"])
    lib = C.CDLL(path)
    sig = {
        "fp_block_total": [_int], "fp_block_rows": [_int],
        "fp_inverses": [_int, _int, _vp, _sz],
        "fp_sums": [_int, _vp, _vp, _int, _dbl, _dbl, _vp, _sz, _int, _vp, _int, _int, _vp, _vp, _sz],
        "fp_lane_solve": [_int, _vp, _sz, _int, _int, _int, _vp, _sz],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = args
    lib.fp_layout.restype = None
    lib.fp_layout.argtypes = [_int, _vp]
    return lib


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_vp)


def layout(lib, kcap):
    o = np.zeros(8, np.int32)
    lib.fp_layout(kcap, _p(o))
    S = dict(zip(("Lv", "La", "rdv", "rda", "w", "bg", "iv", "ia"), (int(x) for x in o)))
    S["total"] = lib.fp_block_total(kcap)
    return S


def _guarded(a):
    """a copy of the f64 array `a` followed by a guard band of sentinels"""
    out = np.empty(a.size + GUARD, np.float64)
    out[:a.size] = a
    out[a.size:].view(np.uint64)[:] = SENT_BITS
    return out


def _sentinels(count):
    return np.full(count + GUARD, SENT_BITS, np.uint64).view(np.float64)


def _intact(a, count):
    return np.all(a[count:].view(np.uint64) == SENT_BITS)


def _twice(call, make):
    first = make()
    assert call(*first) == 0
    second = make()
    assert call(*second) == 0
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes(), "two runs of one kernel differ"
    return second


def inverses(lib, kcap, k, block):
    """the block with S.iv / S.ia filled"""
    (b,) = _twice(lambda b: lib.fp_inverses(kcap, k, _p(b), b.size), lambda: (_guarded(block),))
    assert _intact(b, block.size), "written past the block"
    return b[:block.size]


def sums(lib, maxni, V, A, sv, sa, block, kcap, g, jbase, flags):
    """(sums[4, 64] = nv, dv, na, ab per lane, the block as the kernel left it)"""
    p, k = V.shape[0], len(g)
    g = np.ascontiguousarray(g, np.int32)
    flags = np.ascontiguousarray(flags, np.int32)
    assert V.shape == A.shape == (p, p) and flags.size == 64

    def call(b, out):
        return lib.fp_sums(maxni, _p(V), _p(A), p, sv, sa, _p(b), b.size, kcap, _p(g), k, jbase, _p(flags),
                           _p(out), out.size)
    b, out = _twice(call, lambda: (_guarded(block), _sentinels(256)))
    assert _intact(b, block.size) and _intact(out, 256), "written past the end"
    return out[:256].reshape(4, 64), b[:block.size]


def lane_solve(lib, nb, block, kcap, k, which, rhs):
    """rhs[64, nb * 8] -> the 64 solutions"""
    rhs = np.ascontiguousarray(rhs, np.float64)
    assert rhs.shape == (64, nb * 8)
    block = np.ascontiguousarray(block)
    (x,) = _twice(lambda x: lib.fp_lane_solve(nb, _p(block), block.size, kcap, k, which, _p(x), x.size),
                  lambda: (_guarded(rhs.ravel()),))
    assert _intact(x, rhs.size), "written past the right-hand sides"
    return x[:rhs.size].reshape(64, nb * 8)
