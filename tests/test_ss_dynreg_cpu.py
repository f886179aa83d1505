"""The restatement of the dynamic regression state model (tests/ss_dynreg_oracle.py) pinned before anything
is compared with it, and the library's new entry points -- no GPU.

  (a) d = 1, x = 1 is a local level: its impute_state draw equals ss_student_oracle.impute_state's of
      [level + 4 seasons] within 1e-12 (that file's twin gate), statistics included
  (b) with zero normals impute_state is dense_posterior's mean within 1e-9: d = 3, a column that is 0 over
      a stretch holding t = 0 and one holding T - 1, an all-zero row, a missing observation, mixed signs
  (c) n = T - 1 for every coefficient
  (d) the doubling identity: x -> 2 x with a0, sigma -> 1/2 and P0 -> 1/4 gives states of exactly half,
      bit for bit (every scaling is a power of two)
  (e) the seeds of the GPU test's loop: no variance draw decides within 1e-9 of a threshold
  (f) the library exports the three calls and SIGNATURES binds them
"""
import ctypes as C

import numpy as np

import ss_dynreg_cases as sdc
import ss_dynreg_oracle as sdo
import ss_holiday_oracle as sho
import ss_student_oracle as sso
from cases import general_spec


def state_stream(oracle, seed, chain):
    L = oracle.lib
    L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_rnorm.restype = C.c_double
    rng = oracle.rng_philox(seed, chain, 2, 0)
    return lambda mu, sd: L.bo_rnorm(C.byref(rng), float(mu), float(sd))


def test_one_predictor_of_ones_is_a_local_level(oracle):
    T = 40
    X, y, obs = sdc.data(T, seasonal=((4, 1),), missing=(0, 17))
    sdy = float(np.std(y, ddof=1))
    plain = general_spec(y, [("level",), ("seasonal", 4, 1)])
    dyn = [sdo.dynreg_block(np.ones((T, 1)), sdy, plain[0]["initial_sigma"], a0=plain[0]["a0"])] + plain[1:]
    dyn[0]["P0"] = plain[0]["P0"]
    var = [b["initial_sigma"] ** 2 for b in plain]
    H = np.full(T, 0.8)
    ob = obs.astype(bool)
    want = sso.impute_state(sso.Structure(plain), var, y, ob, H, state_stream(oracle, 7, 2))
    got = sdo.impute_state(sdo.Structure(dyn), var, y, ob, H, state_stream(oracle, 7, 2))
    err = np.max(np.abs(got - want)) / np.abs(want).max()
    print("d = 1, x = 1 against the local level: relative error %.3e" % err)
    assert err < 1e-12
    n0, s0 = sso.state_model_suf(sso.Structure(plain), want)
    n1, s1 = sdo.state_model_suf(sdo.Structure(dyn), want)
    assert all(np.array_equal(a[:len(b)], b) for a, b in zip(n0, n1))
    assert all(np.allclose(a[:len(b)], b, rtol=1e-13, atol=0) for a, b in zip(s0, s1))


def hard_case():
    T = 30
    X, y, obs = sdc.data(T, seasonal=(), missing=(11,))
    sdy = float(np.std(y, ddof=1))
    x = sdc.predictors(T, 3, 41, hard=T)
    assert np.all(x[:5, 1] == 0) and np.all(x[T - 6:, 1] == 0) and np.all(x[9] == 0)
    assert (x < 0).any() and (x > 0).any()
    blocks = general_spec(y, [("level",)]) + [sdo.dynreg_block(x, sdy, [0.3, 0.6, 0.2])]
    var = [b["initial_sigma"] ** 2 for b in blocks]
    return T, y, obs.astype(bool), blocks, var


def test_zero_normals_give_the_dense_posterior_mean():
    T, y, ob, blocks, var = hard_case()
    assert not ob[11]
    S = sdo.Structure(blocks)
    H = np.full(T, 0.5)
    got = sdo.impute_state(S, var, y, ob, H, lambda mu, sd: mu)
    mean, cov = sho.dense_posterior(S, var, y, ob, H)
    err = np.max(np.abs(got.reshape(-1) - mean)) / np.abs(mean).max()
    print("zero normals against the dense posterior mean: relative error %.3e" % err)
    assert err < 1e-9
    assert np.all(np.diag(cov) > 0)


def test_every_coefficient_counts_all_steps_after_the_first():
    T, y, ob, blocks, var = hard_case()
    S = sdo.Structure(blocks)
    rs = np.random.Generator(np.random.PCG64(3))
    st = rs.standard_normal((T, S.m))
    n, ss = sdo.state_model_suf(S, st)
    assert n[0][0] == T - 1
    assert np.array_equal(n[1], np.full(3, T - 1.0))
    for i in range(3):
        want = float(np.sum(np.diff(st[:, 1 + i]) ** 2))
        assert abs(ss[1][i] - want) < 1e-13 * want
    assert sdo.block_stream_ids(sdc.list_two(y, T)) == [[10, 26, 42], [1], [58, 74]]


def doubled(blocks):
    """x -> 2 x, a0 and sigma -> 1/2, P0 -> 1/4 on every dynamic block"""
    out = []
    for b in blocks:
        if b["kind"] == sdo.DYNREG:
            b = dict(b, predictors=2.0 * b["predictors"], a0=0.5 * b["a0"], P0=0.25 * b["P0"],
                     initial_sigma=0.5 * b["initial_sigma"])
        out.append(b)
    return out


def test_doubling_the_predictors_halves_the_coefficients_bit_for_bit(oracle):
    T, y, ob, blocks, var = hard_case()
    blocks[1]["a0"] = np.array([0.25, -1.5, 0.75])
    twice = doubled(blocks)
    H = np.full(T, 0.5)
    one = sdo.impute_state(sdo.Structure(blocks), var, y, ob, H, state_stream(oracle, 9, 1))
    two = sdo.impute_state(sdo.Structure(twice), [b["initial_sigma"] ** 2 for b in twice], y, ob, H,
                           state_stream(oracle, 9, 1))
    assert np.array_equal(two[:, 0], one[:, 0])
    assert np.array_equal(two[:, 1:], 0.5 * one[:, 1:])
    assert np.abs(one[:, 1:]).max() > 0


def test_gpu_loop_seeds_decide_with_margin(oracle):
    c = sdc.loop_case()
    ystar = c["y"] - c["X"] @ c["b0"]
    for ch in c["check"]:
        o = sdo.DynRegOracle(oracle, c["T"], c["obs"], c["blocks"], c["seed"], ch)
        o.impute_state(ystar, c["sig0"])
        for _ in range(c["rounds"]):
            o.draw_state_models()
            o.impute_state(ystar, c["sig0"])
        assert o.margin > 1e-9, (ch, o.margin)
        assert all(np.all(v > 0) for v in o.var)


def test_library_exports_the_dynamic_regression_entry_points():
    import boom_amd
    from boom_amd.capi import SIGNATURES
    lib = boom_amd.load_library()
    for name in ("ba_ss_add_dynamic_regression", "ba_ss_set_dynamic_predictors", "ba_ss_get_dynamic_predictors"):
        assert name in SIGNATURES
        assert getattr(lib, name) is not None
