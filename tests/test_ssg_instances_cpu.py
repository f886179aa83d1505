"""Which kernel serves a state draw of the structural model (boom_amd/csrc/ssg_instances.h: the template
kernel, or one variant of the general kernel, or a refusal -- from the tables the launch carries): runs the
host-only check tests/cpp/ssg_instances_check.cpp, built with the address and undefined-behaviour sanitizers
by `make -C tests/cpp`.  No GPU, and the library is not loaded."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_kernel_choice_of_a_state_draw():
    exe = os.path.join(HERE, "cpp", "build", "ssg_instances_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "build/ssg_instances_check"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failures" in out.stdout, out.stdout
