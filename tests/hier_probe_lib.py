"""ctypes loader of tests/cpp/hier_probe.hip (build/libhier_probe.so, built by
`make -C tests/cpp -f hier_regholiday.mk`): the product's rhh_draw_kernel, launched directly.  draw() runs
the kernel TWICE from the same inputs and requires identical bytes back, checks that nothing outside the
model's own coefficients, mu and Omega was written, and returns the second run."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SENT = 0x7FF8C0DEC0DEC0DE   # a NaN with a payload: no draw gives it
BAD_REQUEST = -1
_hip_error = []
_vp, _sz, _u32, _u64, _i64, _int, _dbl = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int64, C.c_int, C.c_double


def load():
    path = os.path.join(HERE, "cpp", "build", "libhier_probe.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-f", "hier_regholiday.mk", "build/libhier_probe.so"])
    lib = C.CDLL(path)
    for name in ("hp_max_coef", "hp_max_models", "hp_max_width", "hp_hyper_stride", "hp_stream", "hp_bad_draw"):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = []
    lib.hp_draw.restype = C.c_int
    lib.hp_draw.argtypes = [_int] * 5 + [_dbl, _u32, _u32, _i64] + [_vp, _sz] * 9
    return lib


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_vp)


def pack_hyper(lib, slot, hy, d):
    """ss_hier_regholiday_oracle.hyper()'s matrices as the device block of model `slot`"""
    W, stride = lib.hp_max_width(), lib.hp_hyper_stride()
    out = np.zeros((lib.hp_max_models(), stride))
    for r in range(d):
        out[slot, 2 * W * W + r] = hy["sinv0mu0"][r]
        for c in range(d):
            out[slot, r * W + c] = hy["sinv0"][r, c]
            out[slot, W * W + r * W + c] = hy["s0"][r, c]
    return out


def draw(lib, d, H, nu0, hy, sigsq, counts, totals, coef, mu, omega, pos, seed, slot=0, base=0, chain_offset=0):
    """`chains` = len(sigsq) chains on one model: counts (H d, shared), totals / coef (chains x H d), mu
    (chains x d), omega (chains x d x d), pos (chains).  Returns dict(coef, mu, omega, pos, status) after the
    call; everything the kernel must not touch is filled with a sentinel and checked."""
    if _hip_error:
        raise RuntimeError("an earlier call returned HIP error %d: nothing more is launched" % _hip_error[0])
    NC, NM, W = lib.hp_max_coef(), lib.hp_max_models(), lib.hp_max_width()
    chains, n = len(sigsq), H * d
    sent = np.array([SENT], np.uint64).view(np.float64)[0]
    hyper = pack_hyper(lib, slot, hy, d)
    cnt = np.zeros(NC)
    cnt[base:base + n] = counts
    tot = np.zeros((chains, NC))
    tot[:, base:base + n] = totals
    runs = []
    for _ in range(2):
        cf = np.full((chains, NC), sent)
        cf[:, base:base + n] = coef
        m = np.full((chains, NM, W), sent)
        m[:, slot, :d] = mu
        om = np.full((chains, NM, W, W), sent)
        om[:, slot, :d, :d] = omega
        ps = np.ascontiguousarray(pos, np.uint64).copy()
        st = np.zeros(chains, np.int32)
        sg = np.ascontiguousarray(sigsq, np.float64)
        rc = lib.hp_draw(chains, slot, base, d, H, float(nu0), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, chain_offset,
                         _p(hyper), hyper.size, _p(sg), sg.size, _p(cnt), cnt.size, _p(tot), tot.size, _p(cf), cf.size,
                         _p(m), m.size, _p(om), om.size, _p(ps), ps.size, _p(st), st.size)
        if rc > 0:
            _hip_error.append(rc)
        assert rc == 0, "hp_draw returned %d" % rc
        runs.append((cf, m, om, ps, st))
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes(), "two runs of one kernel differ"
    cf, m, om, ps, st = runs[1]
    # nothing but the model's own entries was written
    keep = np.ones(NC, bool)
    keep[base:base + n] = False
    assert np.all(cf[:, keep].view(np.uint64) == SENT), "coefficients of another model were written"
    mk = np.ones((NM, W), bool)
    mk[slot, :d] = False
    assert np.all(m[:, mk].view(np.uint64) == SENT), "mu was written outside the model's d entries"
    ok = np.ones((NM, W, W), bool)
    ok[slot, :d, :d] = False
    assert np.all(om[:, ok].view(np.uint64) == SENT), "Omega was written outside the model's d x d entries"
    return dict(coef=cf[:, base:base + n].copy(), mu=m[:, slot, :d].copy(), omega=om[:, slot, :d, :d].copy(), pos=ps, status=st)
