"""The regression holiday's host arithmetic (boom_amd/csrc/ssg_regholiday.h: the arguments' checks, the
calendars against a launch and a forecast, the shared table, the active steps and the counts), its row of
the rule book and the kernel choice of a launch with a series per chain: runs the host-only check
tests/cpp/ssg_regholiday_check.cpp, built with the address and undefined-behaviour sanitizers by
`make -C tests/cpp -f regholiday.mk`.  No GPU, and the library is not loaded."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_regression_holiday_host_arithmetic():
    exe = os.path.join(HERE, "cpp", "build", "ssg_regholiday_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-f", "regholiday.mk", "build/ssg_regholiday_check"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failures" in out.stdout, out.stdout
