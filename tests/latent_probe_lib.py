"""ctypes loader of tests/cpp/latent_probe.hip (build/liblatent_probe.so, built by
`make -C tests/cpp`): the product's Student, quantile and multinomial logit latent-data kernels,
launched directly with the product's geometry.  The discipline is imputer_probe_lib's: every call
runs the kernel TWICE from the same inputs and requires identical bytes back (repeatability),
checks the guard bands, and returns the arrays of the second run as uint64 bit patterns.  A call
that does not return 0 (a HIP error, or a request the probe refused) fails its assertion, and the
loader then refuses every further launch of the process."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle_lib import fcol
from rng_probe_lib import GUARD, SENT_BITS, SENT_I32, _p, _twice, seed_words, sentinel_u64

HERE = os.path.dirname(os.path.abspath(__file__))
_vp, _sz, _u32, _u64, _i64, _int, _dbl = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int64, C.c_int, C.c_double
_HEAD = [_int, _int, _int, _int, _i64, _vp, _sz, _vp, _vp, _sz, _u32, _u32, _u64, _vp, _sz]
STUDENT_ENTRY = dict(student="lp_student_impute", student_ss="lp_student_impute_ss", ss_h="lp_student_ss_h",
                     ss_suf="lp_student_ss_suf", sn="lp_student_sigma_nu", sn_ss="lp_student_sigma_nu_ss")
ROW_ARRAYS = ("z", "w", "u", "h")
_failed = []


def load():
    path = os.path.join(HERE, "cpp", "build", "liblatent_probe.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "build/liblatent_probe.so"])
    lib = C.CDLL(path)
    student = _HEAD + [_vp, _sz, _vp, _vp, _vp, _vp, _sz, _dbl, _dbl, _dbl, _int, _dbl, _dbl, _vp, _sz, _vp, _sz, _i64,
                       _vp, _vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _sz, _int, _vp, _sz]
    for name in STUDENT_ENTRY.values():
        getattr(lib, name).argtypes = student
    lib.lp_quantile_impute.argtypes = _HEAD + [_vp, _sz, _dbl, _vp, _vp, _sz, _sz]
    lib.lp_mlogit_expand.argtypes = [_i64, _int, _int, _int, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _sz]
    for name in ("lp_mlogit_impute", "lp_mlogit_wss"):
        getattr(lib, name).argtypes = _HEAD + [_int, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _sz]
    for name in ("lp_kmax", "lp_stream", "lp_stride"):
        getattr(lib, name).argtypes = [_int]
    return lib


def _guarded(call):
    """after a call that did not return 0 nothing more is launched in this process"""
    def run(*arrays):
        assert not _failed, "an earlier launch failed (%r): nothing more is launched" % (_failed[0],)
        rc = call(*arrays)
        if rc != 0:
            _failed.append(rc)
        return rc
    return run


def _head(case):
    n, p, chains, rows = int(case["n"]), int(case["p"]), int(case["chains"]), int(case.get("M", 1))
    X = fcol(case["X"])
    gamma = np.ascontiguousarray(case["gamma"], np.uint8).ravel()
    beta = np.ascontiguousarray(case["beta"], np.float64).ravel()
    assert X.size == n * rows * p and gamma.size == chains * p == beta.size
    k0, k1 = seed_words(case["seed"])
    keep = (X, gamma, beta)

    def args(status):
        return (n, p, chains, int(case["slot_limit"]), int(case["chain_offset"]), _p(X), X.size, _p(gamma), _p(beta),
                gamma.size, k0, k1, int(case["sweep"]), _p(status), status.size)
    return args, keep


def _status(case):
    status = np.full(case["chains"] + GUARD, SENT_I32, np.int32)
    status[:case["chains"]] = case["status0"]
    return status


def _rows(cn, given=None):
    a = sentinel_u64(GUARD + cn + GUARD)
    if given is not None:
        a[GUARD:GUARD + cn] = np.ascontiguousarray(given, np.float64).ravel().view(np.uint64)
    return a


def _tail(count, given=None):
    """a per-chain array: `count` values (sentinels unless given), then the guard band"""
    a = sentinel_u64(count + GUARD)
    if given is not None:
        a[:count] = np.ascontiguousarray(given, np.float64).ravel().view(np.uint64)
    return a


def _check_rows(name, a, cn):
    assert np.all(a[:GUARD] == SENT_BITS) and np.all(a[GUARD + cn:] == SENT_BITS), "a guard band of %s was written" % name
    return a[GUARD:GUARD + cn]


def _check_tail(name, a, count):
    assert np.all(a[count:] == SENT_BITS), "written past the end of %s" % name
    return a[:count]


def _check_status(status, chains):
    assert np.all(status[chains:] == SENT_I32), "written past the status words"
    return status[:chains].copy()


def run_student(lib, case, kind=None, inputs=None):
    """a kernel of student_kernel.hip on the case; inputs: name -> chains x n doubles that the kernel
    READS from a row array (w).  Returns the row arrays z, w, u, h (chains x n), the per-chain
    sigsq, nu, dx, margin, the trace rows, acc (or None) as uint64 bit patterns, and status"""
    kind = kind or case["kind"]
    n, chains = int(case["n"]), int(case["chains"])
    cn = chains * n
    head, keep = _head(case)
    y = np.ascontiguousarray(case["y"], np.float64)
    assert y.size == n
    observed = offset = None
    stride = 0
    if "observed" in case:
        observed = np.ascontiguousarray(case["observed"], np.uint8)
        offset = np.ascontiguousarray(case["offset"], np.float64).ravel()
        stride = int(case["offset_stride"])
        assert offset.size == chains * stride and observed.size == n
    ts = int(case.get("trace_stride", 0))
    tidx = np.ascontiguousarray(case.get("trace_idx", np.zeros(chains)), np.int32)
    assert tidx.size == chains
    acc_in = case.get("acc")
    nacc = chains * lib.lp_acc_count()
    prior = case.get("nu_prior", (0, 0.1, 100.0))

    def make():
        rows = [_rows(cn, (inputs or {}).get(name)) for name in ROW_ARRAYS]
        per = [_tail(chains, case.get(name)) for name in ("sigsq", "nu", "dx", "margin")]
        trace = [_tail(chains * ts), _tail(chains * ts)]
        acc = [_tail(nacc, acc_in)] if acc_in is not None else []
        return rows + per + trace + acc + [_status(case)]

    fn = getattr(lib, STUDENT_ENTRY[kind])

    def call(z, w, u, h, sigsq, nu, dx, margin, tsig, tnu, *rest):
        acc, status = (rest[0], rest[1]) if acc_in is not None else (None, rest[0])
        return fn(*head(status), _p(y), y.size, _p(sigsq), _p(nu), _p(dx), _p(margin), sigsq.size,
                  float(case.get("prior_df", 1.0)), float(case.get("prior_ss", 1.0)), float(case.get("sigma_max", np.inf)),
                  int(prior[0]), float(prior[1]), float(prior[2]),
                  _p(observed) if observed is not None else None, observed.size if observed is not None else 0,
                  _p(offset) if offset is not None else None,
                  offset.size if offset is not None else 0, stride, _p(z), _p(w), _p(u), _p(h), z.size, GUARD,
                  _p(tidx), tidx.size, _p(tsig), _p(tnu), tsig.size, ts, _p(acc) if acc is not None else None,
                  acc.size if acc is not None else 0)
    got = _twice(_guarded(call), make)
    del keep
    out = {name: _check_rows(name, a, cn).reshape(chains, n) for name, a in zip(ROW_ARRAYS, got[:4])}
    for name, a in zip(("sigsq", "nu", "dx", "margin"), got[4:8]):
        out[name] = _check_tail(name, a, chains)
    out["trace_sigsq"] = _check_tail("trace_sigsq", got[8], chains * ts).reshape(chains, ts)
    out["trace_nu"] = _check_tail("trace_nu", got[9], chains * ts).reshape(chains, ts)
    out["acc"] = _check_tail("acc", got[10], nacc).reshape(chains, -1) if acc_in is not None else None
    out["status"] = _check_status(got[-1], chains)
    return out


def run_quantile(lib, case):
    """quantile_impute_kernel: z, w (chains x n) and status"""
    n, chains = int(case["n"]), int(case["chains"])
    cn = chains * n
    head, keep = _head(case)
    y = np.ascontiguousarray(case["y"], np.float64)
    assert y.size == n

    def make():
        return [_rows(cn), _rows(cn), _status(case)]

    def call(z, w, status):
        return lib.lp_quantile_impute(*head(status), _p(y), y.size, float(case["shift"]), _p(z), _p(w), z.size, GUARD)
    z, w, status = _twice(_guarded(call), make)
    del keep
    return dict(z=_check_rows("z", z, cn).reshape(chains, n), w=_check_rows("w", w, cn).reshape(chains, n),
                status=_check_status(status, chains))


def mix_table():
    """the mixture table as the engine passes it (MlogitParams's order), from mlogit_oracle"""
    import mlogit_oracle as mo
    return np.ascontiguousarray(np.concatenate([mo.MIX_MU, mo.MIX_SD, mo.MIX_PREC, mo.MIX_LOGW, mo.MIX_LOGSD]))


def run_mlogit(lib, case, mix=None):
    """mlogit_impute_kernel, then mlogit_wss_kernel on what it left (the shares and the status
    words): u, w, z (chains x n M), wss_part (chains x blocks), wss (chains), status"""
    n, chains, nch = int(case["n"]), int(case["chains"]), int(case["M"])
    cN, nblocks = chains * n * nch, (n + 255) // 256
    head, keep = _head(case)
    y = np.ascontiguousarray(case["y"], np.int32)
    mix = mix_table() if mix is None else np.ascontiguousarray(mix, np.float64)
    assert y.size == n

    def entry(fn):
        def call(u, w, z, part, wss, status):
            return fn(*head(status), nch, _p(y), y.size, _p(mix), mix.size, _p(u), _p(w), _p(z), u.size, GUARD,
                      _p(part), part.size, _p(wss), wss.size)
        return _guarded(call)

    def make():
        return [_rows(cN), _rows(cN), _rows(cN), _tail(chains * nblocks), _tail(chains), _status(case)]
    first = _twice(entry(lib.lp_mlogit_impute), make)
    assert np.all(first[4] == SENT_BITS), "mlogit_impute_kernel wrote wss"

    def make2():
        return [a.copy() for a in first]
    got = _twice(entry(lib.lp_mlogit_wss), make2)
    del keep
    for a, b in zip(first[:4] + [first[5]], got[:4] + [got[5]]):
        assert a.tobytes() == b.tobytes(), "mlogit_wss_kernel wrote more than wss"
    out = {name: _check_rows(name, a, cN).reshape(chains, n * nch) for name, a in zip("uwz", got[:3])}
    out["wss_part"] = _check_tail("wss_part", got[3], chains * nblocks).reshape(chains, nblocks)
    out["wss"] = _check_tail("wss", got[4], chains)
    out["status"] = _check_status(got[5], chains)
    return out


def run_expand(lib, n, nch, psub, pch, Xs, Xc):
    """mlogit_expand_kernel: (X, Xsq) as N x D column-major bit patterns"""
    N, D = n * nch, (nch - 1) * psub + pch
    xs = fcol(Xs) if psub else None
    xc = fcol(Xc) if pch else None

    def make():
        return [_rows(N * D), _rows(N * D)]

    def call(X, Xsq):
        return lib.lp_mlogit_expand(n, nch, psub, pch, _p(xs) if psub else None, xs.size if psub else 0,
                                    _p(xc) if pch else None, xc.size if pch else 0, _p(X), _p(Xsq), X.size, GUARD)
    X, Xsq = _twice(_guarded(call), make)
    return (_check_rows("X", X, N * D).reshape(D, N).T, _check_rows("Xsq", Xsq, N * D).reshape(D, N).T)
