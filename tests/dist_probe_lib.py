"""ctypes loader of tests/cpp/dist_probe.hip (build/libdist_probe.so, built by `make -C tests/cpp`):
the product's scalar samplers, launched directly.  Every call runs the kernel TWICE from the same
inputs and requires identical bytes back (repeatability), checks the guard band and that every
word was written, and returns the second run."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64
SENT_BITS = np.uint64(0x7FF8C0DEC0DEC0DE)            # a NaN with a payload: no draw gives it
FN = dict(exp_rand=0, norm_rand=1, runif=2, random_int=3, rtrun_exp=4, rgamma_scale=5, draw_variance=6,
          rtrun_norm_2=7)
SEQ, WIN = 0, 1
UNIFORM, PER_LANE = 0, 1
BAD_REQUEST = -1
_hip_error = []
_vp, _sz, _u32, _u64, _i64, _int = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int64, C.c_int


def load():
    path = os.path.join(HERE, "cpp", "build", "libdist_probe.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "build/libdist_probe.so"])
    lib = C.CDLL(path)
    sig = {
        "dp_words": [], "dp_nargs": [], "dp_spill_shift": [],
        "dp_draws": [_int] * 5 + [_u32] * 4 + [_u64, _u32, _u32, _i64, _vp, _sz, _vp, _sz],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = args
    return lib


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_vp)


def pack_args(rows):
    """[(a0, ...)] -> float64 array n x 4 (unused arguments 0)"""
    out = np.zeros((len(rows), 4))
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def raw(lib, fn, args, seed, chain, stream, index0, stride, serve, view=SEQ, mode=UNIFORM, threads=64,
        chained=False, nout=None):
    """one call, no checks: (return code, the output array with its guard band).  After a HIP error
    nothing more is launched in this process."""
    if _hip_error:
        raise RuntimeError("an earlier call returned HIP error %d: nothing more is launched" % _hip_error[0])
    args = np.ascontiguousarray(args, np.float64).reshape(-1, 4)
    n = args.shape[0]
    words = lib.dp_words() * n * (threads // 64 if threads >= 64 else 1)
    out = np.full((words if nout is None else nout) + GUARD, SENT_BITS, np.uint64)
    rc = lib.dp_draws(FN[fn], view, mode, threads, int(chained), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF,
                      chain, stream, index0, stride, serve, n, _p(args), args.size, _p(out), out.size - GUARD)
    if rc > 0:
        _hip_error.append(rc)
    return rc, out


def draws(lib, fn, args, seed, chain, stream, index0, stride, serve, view=SEQ, mode=UNIFORM, threads=64,
          chained=False):
    """uint64 array [wave, draw, word]: words 0 1 the value's bits (lane 0, lane 63), 2 3 the final
    position, 4 5 the final stream id, 6 7 *bad"""
    args = np.ascontiguousarray(args, np.float64).reshape(-1, 4)
    n, W = args.shape[0], lib.dp_words()
    runs = []
    for _ in range(2):
        rc, out = raw(lib, fn, args, seed, chain, stream, index0, stride, serve, view, mode, threads, chained)
        assert rc == 0, "dp_draws returned %d" % rc
        runs.append(out)
    assert runs[0].tobytes() == runs[1].tobytes(), "two runs of one kernel differ"
    out = runs[1]
    words = W * n * (threads // 64)
    assert np.all(out[words:] == SENT_BITS), "written past the end"
    body = out[:words].reshape(threads // 64, n, W)
    # (a value may be any NaN but this one; positions, ids and flags never are)
    assert not np.any(body[:, :, 2:] == SENT_BITS), "a word was not written"
    return body


def one_wave(body):
    """(values as float64, value bits, positions, stream ids, bad) of wave 0, after checking that
    lane 0 and lane 63 saw the same"""
    b = body[0]
    for w in (0, 2, 4, 6):
        assert np.array_equal(b[:, w], b[:, w + 1]), "lane 0 and lane 63 differ in word %d" % w
    bits = b[:, 0].copy()
    return bits.view(np.float64), bits, b[:, 2].copy(), b[:, 4].copy(), b[:, 6].astype(np.int64)
