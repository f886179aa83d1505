"""The calendars, lists and data of the regression holiday tests (tests/test_ss_regholiday_cpu.py,
tests/test_ss_regholiday_gpu.py).  T = 70 crosses one edge of the structural kernel's 64-step time blocks,
T = 130 two (63 | 64 and 127 | 128); the observe kernel takes the active steps 64 at a time.

Two models on a list:
  model 0  widths (3, 2, 1), coefficients 0 .. 5
           holiday 0 (0, 1, 2): a recurring holiday at t = 0, 1, 2, at 62, 63, 64 and -- T = 130 -- at 126,
                       127, 128: t = 0 and both time-block edges; t = 62 is a missing day
           holiday 1 (3, 4): t = 30 and T - 1 and, for the forecast, T + 3, T + 4
           holiday 2 (5): never active -- count 0
  model 1  widths (2, 2), coefficients 0 .. 3
           holiday 0 (0, 1): t = 63, 64, the days model 0 is active on too
           holiday 1 (2, 3): coefficient 2 on t = 12 alone, a missing day -- count 0; coefficient 3 at t = 20,
                       40 and T + 1
"""
import numpy as np

import ss_regholiday_oracle as sro
from cases import general_data, general_spec

P = 3
HORIZON = 10
MISSING = (12, 62)
PRIORS = ((0.25, 0.8), (-0.5, 1.5))
COEFS = (np.array([0.75, -1.25, 0.5, 2.0, -0.375, 9.0]), np.array([-0.625, 1.5, 3.0, -2.25]))


def calendars(T):
    n = T + HORIZON
    c0, c1 = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for start in (0, 62, 126):
        for d in range(3):
            if start + d < T:
                c0[start + d] = d
    c0[30], c0[T - 1], c0[T + 3], c0[T + 4] = 3, 4, 3, 4
    c1[63], c1[64] = 0, 1
    c1[12] = 2
    c1[20] = c1[40] = c1[T + 1] = 3
    return c0, c1


def models(T, coefficients=COEFS):
    c0, c1 = calendars(T)
    return [sro.reg_holiday_model((3, 2, 1), PRIORS[0], c0, coefficients[0]),
            sro.reg_holiday_model((2, 2), PRIORS[1], c1, coefficients[1])]


def expected_counts(T):
    """by hand: t = 62 and t = 12 are missing"""
    rec = 3.0 if T > 128 else 2.0
    return [np.array([rec - 1.0, rec, rec, 1.0, 1.0, 0.0]), np.array([1.0, 1.0, 0.0, 2.0])]


def data(T, seasonal=((4, 1),), seed=11, missing=MISSING, p=P):
    X, y, _, _ = general_data(T, p, 2, list(seasonal), seed=seed + T)
    obs = np.ones(T, np.uint8)
    obs[[t for t in missing if t < T]] = 0
    return X, y, obs


def chain_coefficients(chains, seed=17):
    """every chain its own coefficients (multiples of 1/64)"""
    rs = np.random.Generator(np.random.PCG64(seed))
    return [[np.round(rs.standard_normal(6) * 64) / 64, np.round(rs.standard_normal(4) * 64) / 64] for _ in range(chains)]


def chain_parameters(chains, seed, p=P):
    rs = np.random.Generator(np.random.PCG64(seed))
    gam = (rs.uniform(size=(chains, p)) < 0.6).astype(np.uint8)
    gam[:, 0] = 1
    return gam, rs.standard_normal((chains, p)) * gam


def list_small(y):
    """SMALL: level + 4 seasons, m = 4 (the template kernel's shape: the twin is forced onto the general kernel)"""
    return general_spec(y, [("level",), ("seasonal", 4, 1)])


def list_ldc33(y):
    """LDC 33: level + 20 seasons, m = 20"""
    return general_spec(y, [("level",), ("seasonal", 20, 1)])
