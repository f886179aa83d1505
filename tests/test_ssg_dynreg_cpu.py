"""The dynamic regression's part of the arithmetic of a list of state models (boom_amd/csrc/ssg_spec.h: the
block's row and sampler ids, the limits and refusal texts, the predictor table, bl with and without such a
block): runs the host-only check tests/cpp/ssg_dynreg_check.cpp, built with the address and
undefined-behaviour sanitizers by `make -C tests/cpp -f dynreg.mk`.  No GPU, and the library is not loaded."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_dynamic_regression_list_arithmetic():
    exe = os.path.join(HERE, "cpp", "build", "ssg_dynreg_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-f", "dynreg.mk", "build/ssg_dynreg_check"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failures" in out.stdout, out.stdout
