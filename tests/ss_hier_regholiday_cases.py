"""The cases of the hierarchical regression holiday tests (tests/test_ss_hier_regholiday_cpu.py,
tests/test_hier_draw_probe_gpu.py, tests/test_ss_hier_regholiday_gpu.py).

PROBE CASES (probe_cases): one draw each, the smallest at which a path of rhh_draw_kernel can break --
  d = 1, 3, 16 (one lane, a few, a full group of 16); H = 1, 2, 5 (5: more holidays than the wave's four
  groups, a second batch with one group at work); 16 x 16 (the 256-coefficient limit); a holiday whose counts
  are all 0 (its draw is the prior's); a day that is never active (a zero column of counts); nu0 = 2.5, d = 3,
  H = 1 (the last chi-square has 1.5 degrees of freedom: a gamma shape of 0.75, the small-shape sampler); an
  Omega of condition number KAPPA = 1e6; totals with a NaN (the draw is refused).

ENGINE CASES: T = 70 crosses one edge of the structural kernel's 64-step time blocks, T = 130 two.
  the hierarchical model  H = 3 holidays of width 2, coefficients 0 .. 5
           holiday 0 (0, 1): t = 0, 1 and 63, 64 and -- T = 130 -- 127, 128; t = 63 .. are block edges
           holiday 1 (2, 3): t = 30, 31 (31 is a missing day), day 0 again at t = 50, day 1 at T - 1, and T + 2, T + 3
                       for the forecast
           holiday 2 (4, 5): day 0 at t = 45 only: coefficient 5 is never active
  the plain model beside it  ss_regholiday_cases' model 1 (active at 63, 64 too)
"""
import numpy as np

import ss_hier_regholiday_oracle as hro
import ss_regholiday_cases as src
import ss_regholiday_oracle as sro

KAPPA = 1e6
P = src.P
HORIZON = src.HORIZON
MISSING = (12, 31)


def spd(rs, d, ridge=0.5):
    a = rs.standard_normal((d, d))
    m = a @ a.T / d + ridge * np.eye(d)
    return (m + m.T) / 2


def with_condition(rs, d, kappa):
    """an SPD matrix with eigenvalues 1 .. kappa"""
    q, _ = np.linalg.qr(rs.standard_normal((d, d)))
    m = (q * np.logspace(0, np.log10(kappa), d)) @ q.T
    return (m + m.T) / 2


def probe_case(name, d, H, nu0=None, seed=1, zero_holiday=None, zero_day=None, omega=None, nan_total=False):
    rs = np.random.Generator(np.random.PCG64(seed))
    nu0 = float(d + 2) if nu0 is None else float(nu0)
    model = hro.hier_model(H, d, (rs.standard_normal(d), spd(rs, d, 1.0)), (spd(rs, d), nu0), None)
    counts = rs.integers(1, 6, size=(H, d)).astype(np.float64)
    if zero_holiday is not None:
        counts[zero_holiday] = 0.0
    if zero_day is not None:
        counts[:, zero_day] = 0.0
    totals = counts * rs.standard_normal((H, d)) + np.sqrt(counts) * rs.standard_normal((H, d))
    if nan_total:
        totals[0, 0] = np.nan
    return dict(name=name, d=d, H=H, nu0=nu0, model=model, sigsq=float(rs.uniform(0.5, 2.0)), counts=counts, totals=totals,
                mu=rs.standard_normal(d), omega=spd(rs, d) if omega is None else omega(rs), coef=rs.standard_normal((H, d)),
                pos=int(rs.integers(0, 1 << 20)), bad=nan_total)


def probe_cases():
    return [
        probe_case("d 1, H 1", 1, 1, seed=1),
        probe_case("d 1, H 5", 1, 5, seed=2),
        probe_case("d 3, H 1", 3, 1, seed=3),
        probe_case("d 3, H 2", 3, 2, seed=4),
        probe_case("d 3, H 5", 3, 5, seed=5),
        probe_case("d 16, H 2", 16, 2, seed=6),
        probe_case("d 16, H 16", 16, 16, seed=7),
        probe_case("a holiday never observed", 3, 5, seed=8, zero_holiday=4),
        probe_case("a day never active", 3, 2, seed=9, zero_day=1),
        probe_case("nu0 2.5: a gamma shape below 1", 3, 1, nu0=2.5, seed=10),
        probe_case("Omega of condition 1e6", 3, 2, seed=11, omega=lambda rs: with_condition(rs, 3, KAPPA)),
        probe_case("a NaN in the totals", 3, 2, seed=12, nan_total=True),
    ]


# ---- the engine's cases ---------------------------------------------------------------------------------------
H, D = 3, 2
MEAN_PRIOR = (np.array([0.25, -0.5]), np.array([[1.5, 0.25], [0.25, 0.75]]))
VARIANCE_PRIOR = (np.array([[0.5, 0.125], [0.125, 0.25]]), 4.0)
COEFS = np.array([0.75, -1.25, 0.5, 2.0, -0.375, 9.0])


def calendar(T):
    c = np.full(T + HORIZON, -1, np.int32)
    for start in (0, 63, 127):
        for day in range(2):
            if start + day < T:
                c[start + day] = day
    c[30], c[31], c[50], c[T - 1], c[T + 2], c[T + 3] = 2, 3, 2, 3, 2, 3
    c[45] = 4
    return c


def expected_counts(T):
    """by hand: t = 31 is missing"""
    rec = 3.0 if T > 128 else 2.0
    return np.array([rec, rec, 2.0, 1.0, 1.0, 0.0])


def hier(T, coefficients=COEFS):
    return hro.hier_model(H, D, MEAN_PRIOR, VARIANCE_PRIOR, calendar(T), coefficients)


def plain(T, coefficients=src.COEFS[1]):
    return sro.reg_holiday_model((2, 2), src.PRIORS[1], src.calendars(T)[1], coefficients)


def data(T, seasonal=((4, 1),), p=P):
    return src.data(T, seasonal=seasonal, missing=MISSING, p=p)
