"""The lists, calendars and data of the calendar seasonal tests (tests/test_ss_calendar_seasonal_cpu.py,
tests/test_ss_calendar_seasonal_gpu.py).  T = 70 crosses one edge of the kernel's 64-step time blocks,
T = 130 two (63 | 64 and 127 | 128)."""
import numpy as np

import ss_calendar_seasonal_oracle as sco
import ss_holiday_cases as shc
import ss_holiday_oracle as sho
from cases import general_spec

P = shc.P
HORIZON = 40
FIRST_DATE = (2023, 1, 30)
# consecutive starts at the first step, at both time-block edges and at T - 1 (129 at T = 130): more
# starts than a block of nseasons = 4 has components, so the rotating layout's cursor wraps
EDGE_STARTS = (1, 2, 3, 63, 64, 65, 66, 127, 128, 129)
MISSING = (2, 30, 64, 128)   # season starts among them; the first step of the second and third time block


def calendar(name, T, extra=0):
    """(nseasons, flags): T + extra entries"""
    n = T + extra
    if name == "edges":
        return 4, sco.starts_calendar(n, EDGE_STARTS)
    if name == "months":
        return 12, sco.month_starts(FIRST_DATE, n)
    if name == "never":
        return 4, np.zeros(n, np.uint8)
    assert name == "two seasons"
    return 2, sco.starts_calendar(n, EDGE_STARTS)


CALENDARS = ("edges", "months", "never", "two seasons")


def data(T, seed=5, trig=None, missing=MISSING):
    return shc.data(T, seasonal=((7, 1),), seed=seed, missing=missing, trig=trig)


def shaped(y, T, block, shape):
    """the block in a list that runs on the named instance of the general kernel:
      small   level + block                                       (m <= 16)
      ldc33   level + 7 seasons + block + 12 seasons              (16 < m <= 32; small for nseasons = 2 is m 19)
      glob    trig (2 frequencies) + block                        (a GLOB instance)
      holiday level + block + a random-walk holiday of width 3    (both tables live)"""
    sdy = float(np.std(y, ddof=1))
    if shape == "small":
        return general_spec(y, [("level",)]) + [block]
    if shape == "ldc33":
        return general_spec(y, [("level",), ("seasonal", 7, 1)]) + [block] + general_spec(y, [("seasonal", 12, 1)])
    if shape == "glob":
        return general_spec(y, [("trig", 12.0, [1.0, 2.0])]) + [block]
    assert shape == "holiday"
    cal = shc.calendar(3, T, [(0, 1, 2), (20, 0, 3), (63, 0, 3), (T - 2, 0, 2)])
    return general_spec(y, [("level",)]) + [block, sho.holiday_block(3, cal, sdy, 0.6)]


SHAPES = ("small", "ldc33", "glob")


def calendar_list(y, T, name, shape, extra=0):
    sdy = float(np.std(y, ddof=1))
    ns, cal = calendar(name, T, extra)
    return shaped(y, T, sco.calendar_block(ns, cal, sdy), shape)


def regular_pair(y, T, nseasons, duration, phase, shape):
    """the same list twice: a calendar seasonal on the regular calendar t % duration == phase (one entry
    past T: the last transition's flag), and the seasonal of that duration and phase"""
    sdy = float(np.std(y, ddof=1))
    blk = sco.calendar_block(nseasons, sco.regular_calendar(T + 1, duration, phase), sdy)
    seas = general_spec(y, [("seasonal", nseasons, duration, phase)])[0]
    return shaped(y, T, blk, shape), shaped(y, T, seas, shape)


chain_parameters = shc.chain_parameters

# ---- the whole-rounds loop of the GPU test: level + 7 seasons + months, T = 70
LOOP = dict(T=70, chains=4, seed=1213, rounds=12, sig0=0.7, check=(0, 3))


def loop_case():
    c = dict(LOOP)
    c["X"], c["y"], c["obs"] = data(c["T"])
    sdy = float(np.std(c["y"], ddof=1))
    ns, cal = calendar("months", c["T"])
    c["blocks"] = general_spec(c["y"], [("level",), ("seasonal", 7, 1)]) + [sco.calendar_block(ns, cal, sdy)]
    c["g0"] = np.zeros(P, np.uint8)
    c["g0"][0] = 1
    c["b0"] = np.zeros(P)
    return c


# ---- the dense-posterior case: the edges pattern cut to T = 30, variances fixed
DENSE = dict(T=30, chains=4096, seed=20311, sigsq=0.6)


def dense_case():
    c = dict(DENSE)
    c["X"], c["y"], c["obs"] = data(c["T"], missing=(2, 17))
    c["blocks"] = calendar_list(c["y"], c["T"], "edges", "small")
    return c
