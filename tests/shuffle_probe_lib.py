"""Builder and ctypes loader of tests/cpp/shuffle_probe.hip: the product's parallel_shuffle<MASKED>
launched directly on one wavefront.  The probe is compiled with the product's own flags (FLAGS
and FLAGS_ssvs_kernel of boom_amd/csrc/Makefile, read from there) into a directory the caller
names; nothing of the product library is linked."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "boom_amd", "csrc")
SRC = os.path.join(HERE, "cpp", "shuffle_probe.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
BAD_REQUEST = -1


def product_flags(arch="gfx950"):
    """the flags ssvs_kernel.hip is compiled with"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    flags += re.search(r"^FLAGS_ssvs_kernel\s*:=\s*(.*)$", text, re.M).group(1).split()
    return flags


def compile_probe(out, extra):
    subprocess.run([HIPCC] + product_flags() + ["-I" + CSRC] + extra + [SRC, "-o", out], check=True,
                   stderr=subprocess.DEVNULL, cwd=os.path.dirname(SRC))
    return out


def load(build_dir):
    lib = C.CDLL(compile_probe(os.path.join(str(build_dir), "libshuffle_probe.so"), ["-shared"]))
    lib.sp_lds_bytes.restype = C.c_int
    lib.sp_lds_bytes.argtypes = [C.c_int]
    lib.sp_shuffle.restype = C.c_int
    lib.sp_shuffle.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    return lib


def shuffle(lib, masked, perm, oth):
    """(the order after one call, after a second call on it), both uint16[p]"""
    perm = np.ascontiguousarray(perm, np.uint16)
    oth = np.ascontiguousarray(oth, np.uint16)
    p = perm.size
    assert oth.size == p
    out = np.full(2 * p, 0xFFFF, np.uint16)
    rc = lib.sp_shuffle(int(masked), p, perm.ctypes.data_as(C.c_void_p), oth.ctypes.data_as(C.c_void_p),
                        out.ctypes.data_as(C.c_void_p), out.size)
    assert rc == 0, "sp_shuffle returned %d" % rc
    return out[:p].copy(), out[p:].copy()
