"""The restatement of the random-walk holiday state model (tests/ss_holiday_oracle.py) pinned before
anything is compared with it, and the library's new entry points -- no GPU.

  (a) a width-1 block active at every step is a local level: its impute_state draw equals
      ss_student_oracle.impute_state's of [level + 4 seasons] within 1e-12 (the gate
      test_student_trend_cpu.py uses for its twin identity)
  (b) with zero normals impute_state is dense_posterior's mean within 1e-9 (that file's gate): two
      holidays that overlap on two days, a level, windows active at t = 0 and at T - 1, a missing
      observation on an active day
  (c) state_model_suf counts the active t >= 1 only; a never-active block has n = 0 and its variance
      draw is the prior's
  (d) the seeds of the GPU test's loop: no variance draw of the restatement decides within 1e-9 of a
      threshold (the regression-free form of the loop; the GPU test asserts it on the rounds it runs)
  (e) the library exports ba_ss_set_holiday_calendar / ba_ss_get_holiday_calendar and SIGNATURES binds
      them
"""
import ctypes as C

import numpy as np

import ss_holiday_cases as shc
import ss_holiday_oracle as sho
import ss_student_oracle as sso
from cases import general_spec


def state_stream(oracle, seed, chain):
    L = oracle.lib
    L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_rnorm.restype = C.c_double
    rng = oracle.rng_philox(seed, chain, 2, 0)
    return lambda mu, sd: L.bo_rnorm(C.byref(rng), float(mu), float(sd))


def test_always_active_width_one_is_a_local_level(oracle):
    T = 40
    X, y, obs = shc.data(T, seasonal=((4, 1),), missing=(0, 17))
    sdy = float(np.std(y, ddof=1))
    plain = general_spec(y, [("level",), ("seasonal", 4, 1)])
    hol = [sho.holiday_block(1, np.zeros(T, np.int32), sdy, plain[0]["initial_sigma"][0], a0=plain[0]["a0"])] + plain[1:]
    var = [b["initial_sigma"] ** 2 for b in plain]
    H = np.full(T, 0.8)
    ob = obs.astype(bool)
    want = sso.impute_state(sso.Structure(plain), var, y, ob, H, state_stream(oracle, 7, 2))
    got = sho.impute_state(sho.Structure(hol), var, y, ob, H, state_stream(oracle, 7, 2))
    err = np.max(np.abs(got - want)) / np.abs(want).max()
    print("width-1 holiday against the local level: relative error %.3e" % err)
    assert err < 1e-12
    n0, s0 = sso.state_model_suf(sso.Structure(plain), want)
    n1, s1 = sho.state_model_suf(sho.Structure(hol), want)
    assert all(np.array_equal(a, b) for a, b in zip(n0, n1))
    assert all(np.allclose(a, b, rtol=1e-13, atol=0) for a, b in zip(s0, s1))


def overlap_case():
    T = 30
    X, y, obs = shc.data(T, seasonal=(), missing=(11,))
    sdy = float(np.std(y, ddof=1))
    c1 = shc.calendar(3, T, [(0, 1, 2), (10, 0, 3), (T - 2, 0, 2)])   # active at t = 0 and at T - 1
    c2 = shc.calendar(2, T, [(11, 0, 2), (20, 0, 2)])                  # days 11 and 12: both active; 11 is missing
    blocks = [sho.holiday_block(3, c1, sdy, 0.6), sho.holiday_block(2, c2, sdy, 0.4)] + general_spec(y, [("level",)])
    var = [b["initial_sigma"] ** 2 for b in blocks]
    return T, y, obs.astype(bool), blocks, var


def test_zero_normals_give_the_dense_posterior_mean():
    T, y, ob, blocks, var = overlap_case()
    S = sho.Structure(blocks)
    H = np.full(T, 0.5)
    got = sho.impute_state(S, var, y, ob, H, lambda mu, sd: mu)
    mean, cov = sho.dense_posterior(S, var, y, ob, H)
    err = np.max(np.abs(got.reshape(-1) - mean)) / np.abs(mean).max()
    print("zero normals against the dense posterior mean: relative error %.3e" % err)
    assert err < 1e-9
    assert np.all(np.diag(cov) > 0)


def test_statistics_count_active_steps_after_the_first():
    T, y, ob, blocks, var = overlap_case()
    S = sho.Structure(blocks)
    rs = np.random.Generator(np.random.PCG64(3))
    st = rs.standard_normal((T, S.m))
    n, ss = sho.state_model_suf(S, st)
    # holiday 1: t = 0 does not count; 1, 10, 11, 12, T - 2, T - 1 do
    assert n[0][0] == 6 and n[1][0] == 4 and n[2][0] == T - 1
    want = sum((st[t, k] - st[t - 1, k]) ** 2 for t, k in [(1, 2), (10, 0), (11, 1), (12, 2), (T - 2, 0), (T - 1, 1)])
    assert abs(ss[0][0] - want) < 1e-13 * want
    want2 = sum((st[t, 3 + k] - st[t - 1, 3 + k]) ** 2 for t, k in [(11, 0), (12, 1), (20, 0), (21, 1)])
    assert abs(ss[1][0] - want2) < 1e-13 * want2


def test_never_active_block_draws_from_the_prior(oracle):
    T = 20
    X, y, obs = shc.data(T, seasonal=(), missing=())
    blocks = shc.list_d(y, T)
    o = sho.HolidayOracle(oracle, T, obs, blocks, seed=5, chain=1)
    o.impute_state(y, 0.6)
    assert o.suf_n[1][0] == 0 and o.suf_ss[1][0] == 0.0
    # (the block's components never move: the draw of every step is the initial state's)
    assert np.all(o.state[:, 1:] == o.state[0, 1:])
    o.draw_state_models()
    b = blocks[1]
    df, guess, smax = b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0]
    rng = oracle.rng_philox(5, 1, 8, 0)
    prior_draw = 1.0 / oracle.trun_gammas(rng, df / 2, df * guess * guess / 2, 1.0 / (smax * smax), 1)[0]
    assert o.var[1][0] == prior_draw
    assert sho.block_stream_ids(shc.list_a(y, T)) == [[1], [7], [8], [24]]


def test_gpu_loop_seeds_decide_with_margin(oracle):
    c = shc.loop_case()
    ystar = c["y"] - c["X"] @ c["b0"]
    for ch in c["check"]:
        o = sho.HolidayOracle(oracle, c["T"], c["obs"], c["blocks"], c["seed"], ch)
        o.impute_state(ystar, c["sig0"])
        for _ in range(c["rounds"]):
            o.draw_state_models()
            o.impute_state(ystar, c["sig0"])
        assert o.margin > 1e-9, (ch, o.margin)
        assert all(np.all(v > 0) for v in o.var)


def test_library_exports_the_calendar_entry_points():
    import boom_amd
    from boom_amd.capi import SIGNATURES
    lib = boom_amd.load_library()
    for name in ("ba_ss_set_holiday_calendar", "ba_ss_get_holiday_calendar"):
        assert name in SIGNATURES
        assert getattr(lib, name) is not None
