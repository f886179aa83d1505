"""Pins the yardstick of ba_ss_holdout_prediction_errors (tests/holdout_errors_ref.py) without a device:
(a) for kinds 1-7 the holdout filter from (alpha, T) is prediction_errors_ref.kalman on the same blocks moved to
    a time origin of T (a0 := T_{T-1} alpha, P0 := diag RQR_{T-1}, the seasonal t0 shifted by -T);
(b) its standardised errors are the Cholesky-whitened residuals of that model's joint normal distribution;
(c) horizon 1 in closed form, v_0 = y*_0 - Z_T'T_{T-1} alpha and F_0 = Z_T'RQR_{T-1} Z_T + sigma^2, for a seasonal
    block with T on a season boundary and off it and for a holiday whose window covers T, ends at T - 1 and
    starts at T + 1;
(d) the C-ABI: the symbol is declared, has a row in capi's table and a method of Engine."""
import os
import re

import numpy as np
import pytest

import holdout_errors_ref as her
import prediction_errors_ref as per
import ss_state_models_oracle as ssm
from cases import general_spec
from ss_holiday_oracle import holiday_block

L = np.longdouble
RTOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LISTS = {
    "level": [("level",)],
    "trend+seasonal(4,3,t0=1)": [("trend",), ("seasonal", 4, 3, 1)],
    "ar3": [("ar", 3, [0.5, -0.2, 0.1])],
    "level+ar1": [("level",), ("ar", 1, [0.6])],
    "intercept+trig": [("intercept",), ("trig", 7.0, [1.0, 2.0])],
    "semilocal+seasonal7": [("semilocal",), ("seasonal", 7, 1)],
    "trend+seasonal(5,1)+seasonal(3,4,t0=2)": [("trend",), ("seasonal", 5, 1), ("seasonal", 3, 4, 2)],
}


def drawn_case(desc, seed, h):
    """blocks, one chain's parameters, a final state, sigma^2 and h rows of y* -- all drawn, nothing fitted"""
    rs = np.random.Generator(np.random.PCG64(seed))
    blocks = general_spec(rs.standard_normal(40), desc)
    params = per.initial_params(blocks)
    for b, q in zip(blocks, params):
        q["var"] = rs.uniform(0.05, 1.5, len(q["var"]))
        if b["kind"] == per.SEMILOCAL:
            q["phi"] = np.array([0.7, 0.3])
    m = sum(per.block_dim(b) for b in blocks)
    alpha = rs.standard_normal(m)
    f = 0
    for b, q in zip(blocks, params):
        if b["kind"] == per.SEMILOCAL:
            alpha[f + 2] = q["phi"][1]   # (the component IS the slope's long-run mean)
        f += per.block_dim(b)
    return blocks, params, alpha, float(rs.uniform(0.3, 1.2)), rs.standard_normal(h) * 2.0


def rel(a, b):
    a, b = np.asarray(a, L), np.asarray(b, L)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), L(1e-300))))


# ---- (a), (b)
@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("T", [40, 41, 42, 43])
def test_holdout_filter_is_the_filter_of_the_shifted_model(name, T):
    h = 14
    blocks, params, alpha, sigsq, ys = drawn_case(LISTS[name], 100 + T, h)
    shifted = her.shifted_blocks(blocks, params, alpha, T)
    for form in ("update", "filtered"):
        got = her.holdout_filter(her.model_view(blocks, params), alpha, T, sigsq, ys, form=form)
        want = per.kalman(shifted, params, sigsq, ys, None, form=form)
        sF = np.sqrt(want["F"])
        assert float(np.max(np.abs(got["v"] - want["v"]) / sF)) <= RTOL, (name, form)
        assert rel(got["F"], want["F"]) <= RTOL, (name, form)
        assert float(np.max(np.abs(got["std"] - want["std"]))) <= RTOL, (name, form)
    # (b): one multivariate normal, no filter
    joint = per.joint_gaussian(shifted, params, sigsq, ys, None)
    got = her.holdout_filter(her.model_view(blocks, params), alpha, T, sigsq, ys)
    assert float(np.max(np.abs(got["std"] - joint["white"]))) <= RTOL * max(1.0, float(np.max(np.abs(joint["white"])))), name


def test_the_two_views_agree_where_both_serve():
    """level + trend + seasonal + trig through prediction_errors_ref.Model and through Structure"""
    desc = [("trend",), ("seasonal", 4, 3, 1), ("trig", 7.0, [1.0, 2.0])]
    blocks, params, alpha, sigsq, ys = drawn_case(desc, 7, 20)
    for T in (40, 41):
        a = her.holdout_filter(her.model_view(blocks, params), alpha, T, sigsq, ys)
        b = her.holdout_filter(her.structure_view(ssm.Structure(blocks), [q["var"] for q in params]), alpha, T, sigsq, ys)
        assert rel(a["F"], b["F"]) <= RTOL and float(np.max(np.abs(a["v"] - b["v"]))) <= 1e-11


# ---- (c)
@pytest.mark.parametrize("T,boundary", [(40, True), (41, False), (42, False), (43, True)])
def test_horizon_one_seasonal_closed_form(T, boundary):
    """[level, seasonal(4 seasons, duration 3, t0 = 1)]: time t starts a season where (t - 1) % 3 == 0"""
    blocks, params, alpha, sigsq, ys = drawn_case([("level",), ("seasonal", 4, 3, 1)], 11, 1)
    assert ((T - 1) % 3 == 0) == boundary
    lv, sv = L(params[0]["var"][0]), L(params[1]["var"][0])
    al = np.asarray(alpha, L)
    seas = -(al[1] + al[2] + al[3]) if boundary else al[1]
    v0 = L(ys[0]) - (al[0] + seas)
    F0 = lv + (sv if boundary else L(0)) + L(sigsq)
    got = her.holdout_filter(her.model_view(blocks, params), alpha, T, sigsq, ys)
    assert abs(got["v"][0] - v0) <= RTOL * np.sqrt(F0) and abs(got["F"][0] - F0) <= RTOL * F0
    got = her.holdout_filter(her.structure_view(ssm.Structure(blocks), [q["var"] for q in params]), alpha, T, sigsq, ys)
    assert abs(got["v"][0] - v0) <= RTOL * np.sqrt(F0) and abs(got["F"][0] - F0) <= RTOL * F0


def holiday_calendar(count, first, width):
    cal = np.full(count, -1, np.int32)
    cal[first:first + width] = np.arange(width)[:max(0, min(width, count - first))]
    return cal


@pytest.mark.parametrize("which,first", [("covers T", 39), ("ends at T - 1", 37), ("starts at T + 1", 41)])
def test_horizon_one_holiday_closed_form(which, first):
    """[level, random-walk holiday of width 3] at T = 40: the window is [first, first + 3)"""
    T, width = 40, 3
    rs = np.random.Generator(np.random.PCG64(13))
    y = rs.standard_normal(40)
    blocks = general_spec(y, [("level",)]) + [holiday_block(width, holiday_calendar(T + 1, first, width), 1.0)]
    var = [np.array([0.4]), np.array([0.9])]
    alpha, sigsq, ys = rs.standard_normal(1 + width), 0.6, rs.standard_normal(1)
    k = T - first if 0 <= T - first < width else -1
    assert (k >= 0) == (which == "covers T")
    al = np.asarray(alpha, L)
    v0 = L(ys[0]) - (al[0] + (al[1 + k] if k >= 0 else L(0)))
    F0 = L(var[0][0]) + (L(var[1][0]) if k >= 0 else L(0)) + L(sigsq)
    got = her.holdout_filter(her.structure_view(ssm.Structure(blocks), var), alpha, T, sigsq, ys)
    assert abs(got["v"][0] - v0) <= RTOL * np.sqrt(F0) and abs(got["F"][0] - F0) <= RTOL * F0


def test_nothing_of_time_T_plus_h_is_asked_for():
    """a holiday calendar of exactly T + h entries serves horizon h (entry T + h would be an index error)"""
    T, h, width = 40, 5, 3
    rs = np.random.Generator(np.random.PCG64(17))
    blocks = general_spec(rs.standard_normal(40), [("level",)]) + [holiday_block(width, holiday_calendar(T + h, 42, width), 1.0)]
    var = [np.array([0.4]), np.array([0.9])]
    out = her.holdout_filter(her.structure_view(ssm.Structure(blocks), var), rs.standard_normal(1 + width), T, 0.5,
                             rs.standard_normal(h))
    assert np.all(np.isfinite(np.asarray(out["v"], float))) and np.all(out["F"] > 0)


def test_gate_has_its_floor_and_is_the_reference_alone():
    blocks, params, alpha, sigsq, ys = drawn_case([("trend",), ("seasonal", 4, 3, 1)], 19, 30)
    X = np.random.Generator(np.random.PCG64(3)).standard_normal((30, 3))
    ref, gate = her.reference_and_gate(her.model_view(blocks, params), alpha, 40, sigsq, ys, X, [1, 0, 1], [0.5, 9.0, -0.25])
    assert gate["v"] >= 64 * her.U and gate["F"] >= 64 * her.U and gate["v"] < 1e-10 and gate["F"] < 1e-10
    want = her.holdout_filter(her.model_view(blocks, params), alpha, 40, sigsq,
                              np.asarray(ys, L) - L(0.5) * np.asarray(X[:, 0], L) + L(0.25) * np.asarray(X[:, 2], L))
    assert float(np.max(np.abs(ref["v"] - want["v"]))) <= 1e-15


def test_a_shorter_horizon_is_a_prefix_to_the_bit():
    """what lets the horizons of the device test share one set of runs (gate_of)"""
    blocks, params, alpha, sigsq, ys = drawn_case([("trend",), ("seasonal", 4, 3, 1), ("ar", 2, [0.4, 0.2])], 23, 20)
    X = np.random.Generator(np.random.PCG64(5)).standard_normal((20, 3))
    view, g, b = her.model_view(blocks, params), [1, 1, 0], [0.5, -2.0, 0.0]
    runs = her.reference_runs(view, alpha, 41, sigsq, ys, X, g, b)
    for k in (1, 7, 20):
        ref, gate = her.reference_and_gate(view, alpha, 41, sigsq, ys[:k], X[:k], g, b)
        pre, pre_gate = her.gate_of(runs, k)
        assert all(np.array_equal(ref[key], pre[key]) for key in ref) and gate == pre_gate


# ---- (d)
def test_the_abi_is_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "boom_amd.h")).read()
    decl = re.search(r"int\s+ba_ss_holdout_prediction_errors\s*\(([^;]*)\)\s*;", header)
    assert decl, "ba_ss_holdout_prediction_errors is not declared in include/boom_amd.h"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert len(args) == 9 and args[0].startswith("ba_engine") and "horizon" in args[4], args
    import ctypes as C

    from boom_amd import capi
    res, argtypes = capi.SIGNATURES["ba_ss_holdout_prediction_errors"]
    assert res is C.c_int and len(argtypes) == 9
    assert argtypes[:5] == [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32]
    assert callable(getattr(capi.Engine, "ss_holdout_prediction_errors"))
