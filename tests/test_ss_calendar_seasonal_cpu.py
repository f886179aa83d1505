"""The restatement of the calendar seasonal state model (tests/ss_calendar_seasonal_oracle.py) pinned
before anything is compared with it, the date helper, and the seeds of the GPU tests -- no GPU.

  (a) on a regular calendar (flag[t] = t % d == ph) the restatement is the seasonal restatement of
      ss_holiday_oracle.py with duration d and time_of_first_observation ph: impute_state, the
      statistics, the forecast and the prediction errors within 1e-12 of scale, the stream positions
      and the counts exactly
  (b) with zero normals impute_state is dense_posterior's mean within 1e-9 on an irregular calendar
  (c) ba_monthly_cycle_calendar against Python's datetime (host only)
  (d) the seeds of the GPU test's loop: no variance draw decides within 1e-9 of a threshold
  (e) the seed of the GPU test's distribution case: the restatement's own 4096 draws pass the bound
"""
import ctypes as C
import datetime

import numpy as np
import pytest

import ss_calendar_seasonal_cases as scc
import ss_calendar_seasonal_oracle as sco
import ss_holiday_oracle as sho
import ss_student_oracle as sso
from cases import general_spec


class Stream:
    """one Philox stream of the oracle with its position in view"""

    def __init__(self, oracle, seed, chain, sid):
        self.L = oracle.lib
        self.L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
        self.L.bo_rnorm.restype = C.c_double
        self.rng = oracle.rng_philox(seed, chain, sid, 0)
        self.count = 0

    def __call__(self, mu, sd):
        self.count += 1
        return self.L.bo_rnorm(C.byref(self.rng), float(mu), float(sd))

    def position(self):
        return bytes(self.rng)


REGULAR = [(1, 0), (3, 0), (3, 2), (7, 0), (7, 1), (7, 6)]


@pytest.mark.parametrize("duration,phase", REGULAR)
def test_regular_calendar_is_the_seasonal(oracle, duration, phase):
    T, ns, h = 40, 4, 9
    X, y, obs = scc.data(T, missing=(0, 17, 21))
    ob = obs.astype(bool)
    sdy = float(np.std(y, ddof=1))
    level = general_spec(y, [("level",)])
    cal = [sco.calendar_block(ns, sco.regular_calendar(T + h, duration, phase), sdy)]
    seas = general_spec(y, [("seasonal", ns, duration, phase)])
    Sc, Ss = sco.Structure(level + cal), sho.Structure(level + seas)
    var = [b["initial_sigma"] ** 2 for b in level + seas]
    H = np.full(T, 0.8)
    a, b = Stream(oracle, 7, 2, 2), Stream(oracle, 7, 2, 2)
    got = sco.impute_state(Sc, var, y, ob, H, a)
    want = sho.impute_state(Ss, var, y, ob, H, b)
    scale = np.abs(want).max()
    assert np.max(np.abs(got - want)) <= 1e-12 * scale
    assert a.count == b.count and a.position() == b.position()
    n0, s0 = sho.state_model_suf(Ss, want)
    n1, s1 = sco.state_model_suf(Sc, want)
    assert all(np.array_equal(u, v) for u, v in zip(n0, n1))
    assert all(np.all(np.abs(u - v) <= 1e-12 * np.abs(u)) for u, v in zip(s0, s1))
    # the forecast, on the forecast stream
    fa, fb = Stream(oracle, 7, 2, 5), Stream(oracle, 7, 2, 5)
    xb = np.linspace(-1.0, 1.0, h)
    f1 = sco.forecast(Sc, T, want[-1], var, 0.8, xb, fa)
    f0 = sho.forecast(Ss, T, want[-1], var, 0.8, xb, fb)
    assert np.max(np.abs(f1 - f0)) <= 1e-12 * np.abs(f0).max()
    assert fa.count == fb.count and fa.position() == fb.position()
    # the prediction errors: the filter asks the Structure alone
    F0, K0 = sho.gains(Ss, var, ob, H)
    F1, K1 = sho.gains(Sc, var, ob, H)
    v0, v1 = sho.innovations(Ss, K0, y, ob), sho.innovations(Sc, K1, y, ob)
    assert np.max(np.abs(F1 - F0) / F0) <= 1e-12 and np.max(np.abs(v1 - v0)) <= 1e-12 * np.abs(v0).max()
    assert abs(sho.log_likelihood(v1, F1, ob) - sho.log_likelihood(v0, F0, ob)) <= 1e-12 * abs(sho.log_likelihood(v0, F0, ob))


@pytest.mark.parametrize("name", ["edges", "months"])
def test_zero_normals_give_the_dense_posterior_mean(name):
    T = 36
    X, y, obs = scc.data(T, missing=(2, 17))
    ob = obs.astype(bool)
    blocks = scc.calendar_list(y, T, name, "small")
    if name == "months":   # (two starts inside T = 36: 2 and 30)
        assert list(np.flatnonzero(blocks[1]["calendar"][:T])) == [2, 30]
    S = sco.Structure(blocks)
    var = [b["initial_sigma"] ** 2 for b in blocks]
    H = np.full(T, 0.5)
    got = sco.impute_state(S, var, y, ob, H, lambda mu, sd: mu)
    mean, cov = sho.dense_posterior(S, var, y, ob, H)
    err = np.max(np.abs(got.reshape(-1) - mean)) / np.abs(mean).max()
    print("%s: zero normals against the dense posterior mean: relative error %.3e" % (name, err))
    assert err < 1e-9
    assert np.all(np.diag(cov) > 0)


def test_statistics_count_the_season_starts_after_the_first_step():
    T = 70
    ns, cal = scc.calendar("edges", T)
    cal[0] = 1   # (entry 0 is accepted and never read)
    S = sco.Structure([sco.calendar_block(ns, cal, 1.0)])
    st = np.random.Generator(np.random.PCG64(3)).standard_normal((T, 3))
    n, ss = sco.state_model_suf(S, st)
    starts = [1, 2, 3, 63, 64, 65, 66]
    assert n[0][0] == len(starts)
    want = sum((st[t, 0] + st[t - 1].sum()) ** 2 for t in starts)
    assert abs(ss[0][0] - want) <= 1e-13 * want
    nn, _ = sco.state_model_suf(sco.Structure([sco.calendar_block(4, np.zeros(T, np.uint8), 1.0)]), st)
    assert nn[0][0] == 0


DATES = [
    ((2023, 1, 30), 130, [2, 30, 61, 91, 122]),
    ((2024, 1, 30), 130, [2, 31, 62, 92, 123]),
    ((1900, 2, 27), 10, [2]),
    ((2000, 2, 27), 10, [3]),
]


@pytest.mark.parametrize("first,count,starts", DATES)
def test_date_helper_against_datetime(first, count, starts):
    from boom_amd.capi import monthly_cycle_calendar
    got = monthly_cycle_calendar(*first, count)
    assert got.dtype == np.uint8 and got.shape == (count,)
    assert list(np.flatnonzero(got)) == starts
    assert np.array_equal(got, sco.month_starts(first, count))


def test_date_helper_across_a_year_end_and_its_refusals():
    import boom_amd
    from boom_amd.capi import monthly_cycle_calendar
    for first in ((2023, 11, 17), (2023, 12, 1), (1999, 12, 31), (2100, 2, 28)):
        got = monthly_cycle_calendar(*first, 800)
        assert np.array_equal(got, sco.month_starts(first, 800)), first
        d0 = datetime.date(*first)
        assert (d0 + datetime.timedelta(days=799)).year > first[0]
    assert monthly_cycle_calendar(2023, 12, 1, 1)[0] == 1
    assert monthly_cycle_calendar(2023, 1, 30, 0).shape == (0,)
    for bad in ((2023, 2, 29), (1900, 2, 29), (2023, 13, 1), (2023, 0, 1), (2023, 4, 31), (2023, 1, 0)):
        with pytest.raises(boom_amd.BoomAmdError) as e:
            monthly_cycle_calendar(*bad, 3)
        assert "not a date of the Gregorian calendar" in str(e.value)
    assert monthly_cycle_calendar(2000, 2, 29, 2)[1] == 1


def test_library_exports_the_season_calendar_entry_points():
    import boom_amd
    from boom_amd.capi import SIGNATURES
    lib = boom_amd.load_library()
    for name in ("ba_ss_set_season_calendar", "ba_ss_get_season_calendar", "ba_monthly_cycle_calendar"):
        assert name in SIGNATURES
        assert getattr(lib, name) is not None


def test_gpu_loop_seeds_decide_with_margin(oracle):
    c = scc.loop_case()
    ystar = c["y"] - c["X"] @ c["b0"]
    assert sho.block_stream_ids(sco.Structure(c["blocks"]).blocks) == [[1], [7], [23]]
    for ch in c["check"]:
        o = sco.CalendarOracle(oracle, c["T"], c["obs"], c["blocks"], c["seed"], ch)
        o.impute_state(ystar, c["sig0"])
        for _ in range(c["rounds"]):
            o.draw_state_models()
            o.impute_state(ystar, c["sig0"])
        assert o.margin > 1e-9, (ch, o.margin)
        assert all(np.all(v > 0) for v in o.var)


def test_gpu_distribution_seed_passes_on_the_cpu(oracle):
    """the 4096 draws the device is asked for, made by the restatement: the same bound"""
    c = scc.dense_case()
    T, y, ob, blocks = c["T"], c["y"], c["obs"].astype(bool), c["blocks"]
    S = sco.Structure(blocks)
    var = [b["initial_sigma"] ** 2 for b in blocks]
    H = np.full(T, c["sigsq"])
    FK = sho.gains(S, var, ob, H)
    draws = np.stack([sco.impute_state(S, var, y, ob, H, Stream(oracle, c["seed"], ch, 2), FK).reshape(-1)
                      for ch in range(c["chains"])])
    mean, cov = sho.dense_posterior(S, var, y, ob, H)
    d = len(mean)
    bound = sso.bonferroni_bound(d + d * (d + 1) // 2)
    zm, zc = sso.moment_z(draws, mean, cov)
    print("largest |z|: mean %.3f covariance %.3f, bound %.3f" % (np.abs(zm).max(), np.abs(zc).max(), bound))
    assert np.abs(zm).max() < bound and np.abs(zc).max() < bound
