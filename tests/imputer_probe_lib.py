"""ctypes loader of tests/cpp/imputer_probe.hip (build/libimputer_probe.so, built by
`make -C tests/cpp`): the product's imputation kernels of probit_kernel.hip, launched directly
with the product's geometry.  Every call runs the kernel TWICE from the same inputs and requires
identical bytes back (repeatability), checks the guard bands, and returns the arrays of the
second run as uint64 bit patterns."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle_lib import fcol
from rng_probe_lib import GUARD, SENT_BITS, SENT_I32, _p, _twice, seed_words, sentinel_u64

HERE = os.path.dirname(os.path.abspath(__file__))
_vp, _sz, _u32, _u64, _i64, _int = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int64, C.c_int
ENTRY = dict(probit="ip_probit", logit="ip_logit", logit_ss="ip_logit_ss", pg="ip_logit_pg", poisson="ip_poisson",
             poisson_ss="ip_poisson_ss", ss_h="ip_latent_ss_h", ss_suf="ip_latent_ss_suf")
ARRAYS = ("z", "w", "value", "h")


def load():
    path = os.path.join(HERE, "cpp", "build", "libimputer_probe.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "build/libimputer_probe.so"])
    lib = C.CDLL(path)
    args = [_int, _int, _int, _int, _i64, _vp, _sz, _vp, _vp, _sz, _u32, _u32, _u64, _vp, _sz, _int, _vp, _vp, _sz,
            _vp, _sz, _vp, _vp, _vp, _sz, _vp, _int, _vp, _vp, _sz, _i64, _vp, _vp, _vp, _vp, _sz, _sz]
    for name in ENTRY.values():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, args
    for name in ("ip_chain_ok", "ip_chain_rng_branch", "ip_chain_model_too_large", "ip_chain_forecast_variance",
                 "ip_kmax"):
        getattr(lib, name).restype = C.c_int
    for name in ("ip_logit_missing_variance", "ip_poisson_missing_variance"):
        getattr(lib, name).restype = C.c_double
    return lib


def run(lib, case, kind=None, inputs=None):
    """launch the kernel of case["kind"] (or `kind`) on the case; inputs: name -> chains x n
    doubles that the kernel READS from an output array (w, value).  Returns name -> chains x n
    uint64 bit patterns for z, w, value and h, and "status" (chains)"""
    kind = kind or case["kind"]
    n, p, chains = int(case["n"]), int(case["p"]), int(case["chains"])
    cn = chains * n
    X = fcol(case["X"])
    gamma = np.ascontiguousarray(case["gamma"], np.uint8).ravel()
    beta = np.ascontiguousarray(case["beta"], np.float64).ravel()
    y = np.ascontiguousarray(case["y"], np.float64)
    nt = np.ascontiguousarray(case["nt"], np.float64)
    assert X.size == n * p and gamma.size == chains * p == beta.size and y.size == n == nt.size
    k0, k1 = seed_words(case["seed"])
    mix = None
    if kind.startswith("poisson"):
        from imputer_ref import poisson_table
        from ss_poisson_oracle import Mixtures
        M = Mixtures(poisson_table()[0])
        mix = (np.ascontiguousarray(M.off, np.int32), np.ascontiguousarray(M.mu), np.ascontiguousarray(M.sigma),
               np.ascontiguousarray(M.logw), np.ascontiguousarray(case["obs_mix"], np.int32),
               int(np.searchsorted(M.counts, 1)))
    observed = offset = None
    stride = 0
    if "observed" in case:
        observed = np.ascontiguousarray(case["observed"], np.uint8)
        offset = np.ascontiguousarray(case["offset"], np.float64).ravel()
        stride = int(case["offset_stride"])
        assert offset.size == chains * stride

    def make():
        out = []
        for name in ARRAYS:
            a = sentinel_u64(GUARD + cn + GUARD)
            if inputs and name in inputs:
                a[GUARD:GUARD + cn] = np.ascontiguousarray(inputs[name], np.float64).ravel().view(np.uint64)
            out.append(a)
        status = np.full(chains + GUARD, SENT_I32, np.int32)
        status[:chains] = case["status0"]
        return out + [status]

    fn = getattr(lib, ENTRY[kind])

    def call(z, w, value, h, status):
        return fn(n, p, chains, int(case["slot_limit"]), int(case["chain_offset"]), _p(X), X.size, _p(gamma), _p(beta),
                  gamma.size, k0, k1, int(case["sweep"]), _p(status), status.size, int(case["clt"]), _p(y), _p(nt), n,
                  _p(mix[0]) if mix else None, mix[0].size - 1 if mix else 0, _p(mix[1]) if mix else None,
                  _p(mix[2]) if mix else None, _p(mix[3]) if mix else None, mix[1].size if mix else 0,
                  _p(mix[4]) if mix else None, mix[5] if mix else 0,
                  _p(observed) if observed is not None else None, _p(offset) if offset is not None else None,
                  offset.size if offset is not None else 0, stride, _p(z), _p(w), _p(value), _p(h), z.size, GUARD)
    got = _twice(call, make)
    out = {}
    for name, a in zip(ARRAYS, got):
        assert np.all(a[:GUARD] == SENT_BITS) and np.all(a[GUARD + cn:] == SENT_BITS), "a guard band of %s was written" % name
        out[name] = a[GUARD:GUARD + cn].reshape(chains, n)
    status = got[4]
    assert np.all(status[chains:] == SENT_I32), "written past the status words"
    out["status"] = status[:chains].copy()
    return out
