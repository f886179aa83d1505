"""The yardstick of ba_ss_prediction_errors (tests/prediction_errors_ref.py), pinned without a GPU:
(a) on something that is not a filter -- the joint normal distribution of the observed series,
    built by unrolling the state equation: the filter's log likelihood is that distribution's log
    density and the standardized errors are its Cholesky-whitened residuals, in order (exact
    identities; long double, 1e-12 relative);
(b) on the restatement the Student-t family's tests already pin on the oracle
    (ss_student_oracle.gains / innovations), for a level / trend / seasonal list;
(c) the library, the header and capi.py carry the entry point."""
import os
import re

import numpy as np
import pytest

import prediction_errors_ref as per
from cases import general_data, general_spec, trig_rotations
import student_trend_cases as stc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_cases():
    """T <= 14, m <= 5, two missing steps"""
    rs = np.random.Generator(np.random.PCG64(401))
    out = []

    def add(name, T, desc, student=False, tweak=None):
        y = np.cumsum(rs.standard_normal(T)) + 3.0
        blocks = stc.student_trend_spec(y, desc) if student else general_spec(y, desc)
        params = per.initial_params(blocks)
        for b, q in zip(blocks, params):
            q["var"] = q["var"] * rs.uniform(0.2, 1.5, size=len(q["var"]))
            if b["kind"] == per.STUDENT_TREND:
                q["weights"] = (10.0 ** rs.uniform(-2, 2, T), 10.0 ** rs.uniform(-2, 2, T))
        if tweak:
            tweak(blocks, params)
        obs = np.ones(T, np.uint8)
        obs[[3, T - 2]] = 0
        out.append((name, blocks, params, float(rs.uniform(0.3, 2.0)), y, obs))

    add("level", 14, [("level",)])
    add("trend+seasonal", 14, [("trend",), ("seasonal", 3, 2, 1)])
    add("level+ar2", 12, [("level",), ("ar", 2, [0.5, -0.3])])
    add("intercept+trig", 13, [("intercept",), ("trig", 7.0, [1.0, 2.0])])

    def sl(blocks, params):
        params[0]["phi"] = np.array([0.6, 0.25])
    add("semilocal+seasonal", 14, [("semilocal",), ("seasonal", 3, 1)], tweak=sl)
    add("student trend+seasonal", 14, [("student_trend",), ("seasonal", 4, 1)], student=True)
    return out


SMALL = small_cases()


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_filter_is_the_joint_gaussian(case):
    _, blocks, params, sigsq, y, obs = case
    assert per.Model(blocks, params).m <= 5 and len(y) <= 14 and int((obs == 0).sum()) == 2
    for form in ("update", "filtered"):
        f = per.kalman(blocks, params, sigsq, y, obs, form=form)
        j = per.joint_gaussian(blocks, params, sigsq, y, obs)
        assert abs(f["loglik"] - j["loglik"]) <= 1e-12 * abs(j["loglik"]), (form, f["loglik"], j["loglik"])
        std = f["std"][obs.astype(bool)]
        assert np.all(f["std"][~obs.astype(bool)] == 0) and np.all(f["v"][~obs.astype(bool)] == 0)
        assert np.max(np.abs(std - j["white"]) / np.maximum(1, np.abs(j["white"]))) <= 1e-12, form


def test_agrees_with_the_student_family_restatement():
    import ss_student_oracle as sso
    T, p = 40, 3
    X, y, _, obs = general_data(T, p, 2, [(4, 3)], seed=77, missing_frac=0.1)
    blocks = general_spec(y, [("level",), ("trend",), ("seasonal", 4, 3, 1)])
    params = per.initial_params(blocks)
    gamma, beta, sigsq = np.array([1, 0, 1], np.uint8), np.array([2.5, 0.0, -1.0]), 0.7
    ref, gate = per.reference_and_gate(blocks, params, sigsq, y, X, gamma, beta, obs)
    S = sso.Structure(blocks)
    F, K = sso.gains(S, [q["var"] for q in params], obs, np.full(T, sigsq))
    v = sso.innovations(S, K, y - X[:, [0, 2]] @ beta[[0, 2]], obs)
    dev_v = float(np.max(np.abs(v - ref["v"]) / np.sqrt(ref["F"])))
    dev_F = float(np.max(np.abs(F - ref["F"]) / ref["F"]))
    print("restatement vs long double: v %.3g (gate %.3g), F %.3g (gate %.3g)" % (dev_v, gate["v"], dev_F, gate["F"]))
    assert dev_v <= gate["v"] and dev_F <= gate["F"]
    assert gate["v"] < 1e-9 and gate["F"] < 1e-9   # (P0 <= 1e4: the gate stays far below a wrong entry's effect)


def test_gate_catches_a_wrong_season_boundary():
    """what the gate is for: the season boundary one step off moves the errors by many orders more"""
    T, p = 29, 3
    X, y, _, obs = general_data(T, p, 2, [(4, 3)], seed=78)
    blocks = general_spec(y, [("trend",), ("seasonal", 4, 3, 1)])
    params = per.initial_params(blocks)
    gamma, beta = np.ones(p, np.uint8), np.array([1.0, -2.0, 0.5])
    ref, gate = per.reference_and_gate(blocks, params, 0.5, y, X, gamma, beta, obs)
    wrong = [dict(b, t0=2) if b["kind"] == per.SEASONAL else b for b in blocks]
    off = per.kalman(wrong, params, 0.5, per.ystar(y, X, gamma, beta), obs)
    assert float(np.max(np.abs(off["v"] - ref["v"]) / np.sqrt(ref["F"]))) > 1e6 * gate["v"]


def test_library_header_and_capi_carry_the_entry_point():
    txt = open(os.path.join(ROOT, "include", "boom_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from boom_amd.capi import SIGNATURES
    import boom_amd
    lib = boom_amd.load_library()
    name = "ba_ss_prediction_errors"
    assert re.search(r"\b%s\s*\(" % name, txt)
    assert name in SIGNATURES
    assert hasattr(lib, name)
    assert hasattr(boom_amd.Engine, "ss_prediction_errors")
