"""The arithmetic of a list of state models (boom_amd/csrc/ssg_spec.h: the table of kinds, the append
and its limits, sampler ids, ld / bl, the template shape, the rule book of refusals, the packed
calendars): runs the host-only check tests/cpp/ssg_spec_check.cpp, built with the address and
undefined-behaviour sanitizers by `make -C tests/cpp`.  No GPU, and the library is not loaded."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_state_model_list_arithmetic():
    exe = os.path.join(HERE, "cpp", "build", "ssg_spec_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "build/ssg_spec_check"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failures" in out.stdout, out.stdout
