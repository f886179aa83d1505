"""Generates tests/golden/ss_state_oracle_pins.npz: what tests/ss_holiday_oracle.py, tests/ss_dynreg_oracle.py
and tests/ss_calendar_seasonal_oracle.py computed for the lists of tests/test_ss_state_oracle_pins_cpu.py.
The committed file was written while each of the three modules held its own copy of the recursion, before
they were moved onto tests/ss_state_models_oracle.py; a run of today's modules writes what that test
compares with it, so regenerate it only where a convention of the restatement changes on purpose."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from oracle_lib import Oracle  # noqa: E402
from test_ss_state_oracle_pins_cpu import GOLDEN, entries, record  # noqa: E402


def main():
    oracle = Oracle()
    out = {}
    for module, name in entries():
        for key, value in record(oracle, module, name).items():
            out["%s/%s/%s" % (module, name, key)] = value
    np.savez_compressed(GOLDEN, **out)
    print("wrote %s: %d arrays, %d bytes" % (GOLDEN, len(out), os.path.getsize(GOLDEN)))


if __name__ == "__main__":
    main()
