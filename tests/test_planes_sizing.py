"""The planes workspace of the column service covers both of its users
(boom_amd/csrc/planes_sizing.h): runs the host-only check tests/cpp/planes_sizing_check.cpp,
built with the address and undefined-behaviour sanitizers by `make -C tests/cpp`.  No GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_planes_capacity_covers_rows_and_column_launches():
    exe = os.path.join(HERE, "cpp", "build", "planes_sizing_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "build/planes_sizing_check"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failures" in out.stdout, out.stdout
