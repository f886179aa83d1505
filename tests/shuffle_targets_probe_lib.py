"""Builder and ctypes loader of tests/cpp/shuffle_targets_probe.hip: the product's
fork_shuffle_targets<W> and shuffle_targets launched directly on one workgroup of W wavefronts.
Compiled as shuffle_probe_lib compiles its probe (the product's own flags, nothing of the
product library linked) into a directory the caller names."""
import ctypes as C
import os
import subprocess

import numpy as np

import shuffle_probe_lib as SP

SRC = os.path.join(SP.HERE, "cpp", "shuffle_targets_probe.hip")
BAD_REQUEST = -1
SENTINEL = 0xFFFF


def load(build_dir):
    out = os.path.join(str(build_dir), "libshuffle_targets_probe.so")
    subprocess.run([SP.HIPCC] + SP.product_flags() + ["-I" + SP.CSRC, "-shared", SRC, "-o", out], check=True,
                      stderr=subprocess.DEVNULL, cwd=os.path.dirname(SRC))
    lib = C.CDLL(out)
    lib.st_targets.restype = C.c_int
    lib.st_targets.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                               C.c_uint64, C.c_uint16, C.c_void_p, C.c_size_t]
    return lib


def targets(lib, waves, forked, p, seed, chain, stream, pos):
    """oth[0 .. p] after the call, uint16[p + 1] (every entry held SENTINEL before it)"""
    out = np.zeros(p + 1, np.uint16)
    rc = lib.st_targets(waves, int(forked), p, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, chain, stream, pos,
                        SENTINEL, out.ctypes.data_as(C.c_void_p), out.size)
    assert rc == 0, "st_targets returned %d" % rc
    return out
