"""ctypes loader of tests/cpp/big_probe.hip (build/libbig_probe.so, built by `make -C tests/cpp`):
the large-model kernel's chol_tile, chol_tile_regs, big_solve, big_build_body and big_eval,
launched directly.  Every call runs the kernel TWICE from the same inputs and requires identical
bytes back (repeatability), checks the guard bands behind every writable buffer -- the solve
parking space included --, and returns the arrays of the second run.  The guard bands travel: every
writable array is handed over with its full length (nominal + GUARD), so the device buffer holds
the band behind what the kernel may write and the copy back brings it home.

A HIP error raises ProbeHipError and latches FAULTED: every later call raises at once without a
launch (a device that has reported an error is not used again by this process)."""
import ctypes as C
import os
import subprocess

import numpy as np

import big_ref as R
from fill_probe_lib import GUARD, SENT_BITS, BAD_REQUEST, _guarded, _intact, _p, _sentinels  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
_vp, _sz, _int, _dbl, _i64, _u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int64, C.c_uint64
LAYOUT_NAMES = ("Lv", "La", "rdv", "rda", "w", "bg", "g", "scal", "iv", "ia")
LDS_NAMES = ("tile", "rdt", "w", "y", "rd", "bst", "ctrl", "g", "gst", "perm0", "perm1", "oth", "last", "pred", "gam",
             "gam0", "nbr", "total")
SCALARS = ("logp", "lp", "ldv", "lda", "Q", "c", "SS", "pd", "bad", "k")


def load():
    path = os.path.join(HERE, "cpp", "build", "libbig_probe.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "build/libbig_probe.so"])
    lib = C.CDLL(path)
    chain = [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _i64, _int, _int, _int, _dbl, _dbl, _dbl, _dbl, _dbl]
    sig = {
        "bp_block_total": [_int],
        "bp_chol_tiles": [_int, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz],
        "bp_solve": [_int, _int, _int, _vp, _sz, _vp, _sz, _vp, _sz],
        "bp_build": [_int, _int] + chain + [_vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _u64],
        "bp_eval": chain + [_vp, _int, _vp, _sz, _int, _vp, _sz, _vp, _sz, _vp, _sz],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = args
    for name, args in (("bp_layout", [_int, _vp]), ("bp_lds_layout", [_int, _int, _vp])):
        fn = getattr(lib, name)
        fn.restype = None
        fn.argtypes = args
    return lib


class ProbeHipError(RuntimeError):
    """a probe call came back with a hipError_t"""


FAULTED = False


def _twice(call, make):
    """two runs from the same inputs, identical bytes back.  A refused request is an AssertionError; a
    HIP error is a ProbeHipError, now and for every later call (which then launches nothing)"""
    global FAULTED
    runs = []
    for _ in range(2):
        if FAULTED:
            raise ProbeHipError("an earlier probe call returned a HIP error: nothing more is launched")
        arrays = make()
        rc = call(*arrays)
        if rc > 0:
            FAULTED = True
            raise ProbeHipError("the probe's launch returned HIP error %d" % rc)
        assert rc == 0, "the probe refused the request"
        runs.append(arrays)
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes(), "two runs of one kernel differ"
    return runs[1]


def layout(lib, kcap):
    o = np.zeros(10, np.int32)
    lib.bp_layout(kcap, _p(o))
    S = dict(zip(LAYOUT_NAMES, (int(x) for x in o)))
    S["total"] = lib.bp_block_total(kcap)
    return S


def lds_layout(lib, p, kcap):
    o = np.zeros(18, np.int32)
    lib.bp_lds_layout(p, kcap, _p(o))
    return dict(zip(LDS_NAMES, (int(x) for x in o)))


def chol_tiles(lib, kk, tile):
    """dict(t1, t2: 64 x 64 (chol_tile's LDS tile where it has rows, chol_tile_regs' register rows),
    rd1, rd2, ok1, ok2, ld1, ld2); what the kernel does not write is the sentinel NaN"""
    tile = np.ascontiguousarray(tile, np.float64)
    assert tile.shape == (64, 64)

    def call(t1, t2, r1, r2, s):
        assert t1.size == t2.size and r1.size == r2.size
        return lib.bp_chol_tiles(kk, _p(tile), tile.size, _p(t1), _p(t2), t1.size, _p(r1), _p(r2), r1.size, _p(s), s.size)
    t1, t2, r1, r2, s = _twice(call, lambda: (_sentinels(4096), _sentinels(4096), _sentinels(64), _sentinels(64),
                                              _sentinels(4)))
    for a, n in ((t1, 4096), (t2, 4096), (r1, 64), (r2, 64), (s, 4)):
        assert _intact(a, n), "written past the end"
    return dict(t1=t1[:4096].reshape(64, 64), t2=t2[:4096].reshape(64, 64), rd1=r1[:64], rd2=r2[:64],
                ok1=s[0] != 0.0, ok2=s[1] != 0.0, ld1=s[2], ld2=s[3])


def solve(lib, kcap, k, which, block, rhs):
    """rhs[64 lanes, npan * 64] -> the parked solutions [kcap rows, 64 lanes] (sentinel where big_solve
    parks nothing)"""
    npan = (k + 63) // 64
    rhs = np.ascontiguousarray(rhs, np.float64)
    block = np.ascontiguousarray(block)
    assert rhs.shape == (64, npan * 64)
    (xs,) = _twice(lambda xs: lib.bp_solve(kcap, k, which, _p(block), block.size, _p(rhs), rhs.size, _p(xs), xs.size),
                   lambda: (_sentinels(kcap * 64),))
    assert _intact(xs, kcap * 64), "written past the parking space"
    return xs[:kcap * 64].reshape(kcap, 64)


def _chain_args(c):
    p = c["p"]
    for name in ("V", "A", "b", "l1", "l0", "xty", "gamma"):
        assert c[name].flags["C_CONTIGUOUS"] and c[name].shape[0] == p
    return (_p(c["V"]), _p(c["A"]), p * p, _p(c["b"]), _p(c["l1"]), _p(c["l0"]), _p(c["xty"]), _p(c["gamma"]), p)


def build(lib, waves, reuse, c, kcap, block=None, **over):
    """big_build_body on the case c (fields of big_ref.build_case; `over` replaces some: V, A, xty,
    ss0q, max_model_size, l1, gamma, ...).  block: the block to start from (default: all sentinel).
    Returns dict(block, xs, w, rdv (the LDS copies), and the scalars by name)."""
    c = dict(c, **over)
    S = layout(lib, kcap)
    nxs = waves * kcap * 64

    def make():
        b = _sentinels(S["total"]) if block is None else _guarded(block)
        return b, _sentinels(nxs), _sentinels(10), _sentinels(kcap), _sentinels(kcap)

    def call(b, xs, s, w, rdv):
        return lib.bp_build(waves, int(reuse), *_chain_args(c), int(c["max_model_size"]), c["p"], kcap, c["mode"],
                            c["DF"], c["ss0q"], c["sv"], c["sa"], c["sx"], _p(b), b.size, _p(xs), xs.size, _p(s), s.size,
                            _p(w), _p(rdv), min(w.size, rdv.size), int(SENT_BITS))
    b, xs, s, w, rdv = _twice(call, make)
    assert _intact(b, S["total"]), "written past the block"
    assert _intact(xs, nxs), "written past the parking space"
    assert _intact(s, 10) and _intact(w, kcap) and _intact(rdv, kcap)
    out = dict(zip(SCALARS, (float(x) for x in s[:10])))
    out.update(block=b[:S["total"]], xs=xs[:nxs], w_lds=w[:kcap], rdv_lds=rdv[:kcap], S=S)
    return out


def build_fields(out, k):
    """what big_ref.check_build reads, from a build's outputs"""
    S, b = out["S"], out["block"]
    f = dict(Lv=R.unpack(b[S["Lv"]:], k), La=R.unpack(b[S["La"]:], k), rdv=b[S["rdv"]:S["rdv"] + k],
             rda=b[S["rda"]:S["rda"] + k], w=b[S["w"]:S["w"] + k])
    f.update({n: out[n] for n in ("logp", "lp", "ldv", "lda", "Q", "c", "SS")})
    return f


def evaluate(lib, c, kcap, block, jbase, **over):
    """big_eval<true> on both wavefronts: out[wave, (logp, slow, bad_ss), lane]; the block has to come
    back unchanged"""
    c = dict(c, **over)
    g = np.ascontiguousarray(c["g"], np.int32)
    model = np.ascontiguousarray(c["model"], np.float64)
    block = np.ascontiguousarray(block)
    nxs = 2 * kcap * 64

    def call(b, xs, out):
        return lib.bp_eval(*_chain_args(c), int(c["max_model_size"]), c["p"], kcap, c["mode"], c["DF"], c["ss0q"],
                           c["sv"], c["sa"], c["sx"], _p(g), len(g), _p(model), model.size, jbase, _p(b), b.size,
                           _p(xs), xs.size, _p(out), out.size)
    b, xs, out = _twice(call, lambda: (_guarded(block), _sentinels(nxs), _sentinels(384)))
    assert _intact(b, block.size) and _intact(xs, nxs) and _intact(out, 384), "written past the end"
    assert b[:block.size].tobytes() == block.tobytes(), "the proposals' evaluation changed the model block"
    return out[:384].reshape(2, 3, 64)
