"""The lists, calendars and data of the random-walk holiday tests (tests/test_ss_holiday_cpu.py,
tests/test_ss_holiday_gpu.py).  T = 70 crosses one edge of the kernel's 64-step time blocks, T = 130
two (63 | 64 and 127 | 128)."""
import numpy as np

import ss_holiday_oracle as sho
from cases import general_data, general_spec, kernel_instance

P = 3            # regression coefficients
HORIZON = 10


def calendar(width, T, windows, extra=()):
    """windows: (first time, first position, days); extra: the entries past T"""
    cal = np.full(T, -1, np.int32)
    for t0, k0, n in windows:
        for i in range(n):
            if t0 + i < T:
                assert 0 <= k0 + i < width
                cal[t0 + i] = k0 + i
    return np.concatenate([cal, np.asarray(extra, np.int32)])


def calendars_a(T):
    """two holidays, widths 3 and 2, HORIZON entries past T each.
      holiday 1: a window that began before the series (t = 0, 1 at positions 1, 2); days 20-22; days
                 63-65, across the first time-block edge; at T = 130 days 127-129, across the second
                 edge and active at T - 1; at T = 70 days 68, 69 (active at T - 1) -- the window goes on
                 into the forecast horizon (position 2 at T), and another opens inside it (T + 4 .. T + 6)
      holiday 2: days 21, 22 (both holidays active), 62, 63 and 65, 66: with holiday 1, steps 62-66 are
                 all active and both are on days 63 and 65; at T = 130 days 126, 127; a window at
                 T + 5, T + 6 of the horizon
    every position recurs in a later window: the random walk continues from its last incidence"""
    last = [(127, 0, 3)] if T == 130 else [(T - 2, 0, 2)]
    ext1 = [2 if T != 130 else -1, -1, -1, -1, 0, 1, 2, -1, -1, -1]
    ext2 = [-1, -1, -1, -1, -1, 0, 1, -1, -1, -1]
    w1 = [(0, 1, 2), (20, 0, 3), (63, 0, 3)] + last
    w2 = [(21, 0, 2), (62, 0, 2), (65, 0, 2)] + ([(126, 0, 2)] if T == 130 else [])
    return calendar(3, T, w1, ext1), calendar(2, T, w2, ext2)


MISSING_A = (21, 64)   # an active day; the first step of the second time block (active too)


def data(T, seasonal=((7, 1),), seed=5, missing=MISSING_A, trig=None, p=P):
    X, y, _, _ = general_data(T, p, 2, list(seasonal), seed=seed + T, trig=trig)
    obs = np.ones(T, np.uint8)
    obs[[t for t in missing if t < T]] = 0
    return X, y, obs


def list_a(y, T, pad=False):
    """level + 7 seasons + holiday (3) + holiday (2) [+ 12 seasons: state dimension 23, the LDC 33 instances]"""
    sdy = float(np.std(y, ddof=1))
    c1, c2 = calendars_a(T)
    blocks = general_spec(y, [("level",), ("seasonal", 7, 1)])
    blocks += [sho.holiday_block(3, c1, sdy, 0.6), sho.holiday_block(2, c2, sdy, 0.4)]
    if pad:
        blocks += general_spec(y, [("seasonal", 12, 1)])
    return blocks


def list_c(y, T):
    """a trig block + a holiday of width 4: a GLOB instance"""
    sdy = float(np.std(y, ddof=1))
    cal = calendar(4, T, [(0, 2, 2), (30, 0, 4), (62, 0, 4), (T - 1, 0, 1)])
    return general_spec(y, [("trig", 12.0, [1.0, 2.0])]) + [sho.holiday_block(4, cal, sdy, 0.5)]


def list_d(y, T):
    """a never-active block beside a level"""
    sdy = float(np.std(y, ddof=1))
    return general_spec(y, [("level",)]) + [sho.holiday_block(2, np.full(T, -1), sdy, 0.5)]


def list_instance(y, T, seasons, glob):
    """a holiday of width 2 [+ a one-frequency trig block: GLOB] + a duration-1 seasonal that pads the state to
    the leading dimension wanted (18, 34, 61 seasons: 33, 61, 65): the kernel instances the lists above do
    not reach"""
    sdy = float(np.std(y, ddof=1))
    cal = calendar(2, T, [(0, 1, 1), (T // 2, 0, 2), (T - 1, 0, 1)])
    pad = ([("trig", 12.0, [1.0])] if glob else []) + [("seasonal", seasons, 1)]
    return [sho.holiday_block(2, cal, sdy, 0.5)] + general_spec(y, pad)


def instance_case(seasons, glob):
    """(T, make, data arguments) of test_impute_state_matches_restatement: two time blocks and three steps"""
    T = 2 * kernel_instance(list_instance(np.arange(8.0), 8, seasons, glob))[2] + 3
    return T, lambda y, T: list_instance(y, T, seasons, glob), dict(seasonal=(), missing=(5, T - 2), p=2)


def chain_parameters(chains, seed, p=P):
    """every chain its own regression parameters"""
    rs = np.random.Generator(np.random.PCG64(seed))
    gam = (rs.uniform(size=(chains, p)) < 0.6).astype(np.uint8)
    gam[:, 0] = 1
    return gam, rs.standard_normal((chains, p)) * gam


# ---- the whole-rounds loop of the GPU test: list (a), T = 70
LOOP = dict(T=70, chains=4, seed=911, rounds=12, sig0=0.7, check=(0, 3))


def loop_case():
    c = dict(LOOP)
    c["X"], c["y"], c["obs"] = data(c["T"])
    c["blocks"] = list_a(c["y"], c["T"])
    c["g0"] = np.zeros(P, np.uint8)
    c["g0"][0] = 1
    c["b0"] = np.zeros(P)
    return c
