"""The restatements of the per-step state models (tests/ss_state_models_oracle.py through its three model
files) pinned on what they computed while each file still had its own copy of the recursion: tests such
as "a regular calendar draws what the seasonal draws" now compare two paths through one loop, and this
fixture is the independence they lost.  No GPU.

tests/golden/ss_state_oracle_pins.npz (written by tests/golden/make_golden_state_oracle_pins.py from the
three separate modules) holds, per list: the first impute_state draw, state_model_suf, the variances
after one draw_state_models, a forecast of HORIZON steps, prediction_errors, and the raw bytes of the
state, forecast and variance generators afterwards.  The stream positions and the counts n are equal
exactly; every floating-point array is within 1e-12 of its largest magnitude (the twin-identity gate of
test_student_trend_cpu.py and test_ss_holiday_cpu.py: `@` goes through the machine's BLAS, so not bits).
"""
import os

import numpy as np
import pytest

import ss_calendar_seasonal_cases as scc
import ss_calendar_seasonal_oracle as sco
import ss_dynreg_cases as sdc
import ss_dynreg_oracle as sdo
import ss_holiday_cases as shc
import ss_holiday_oracle as sho
from test_ss_holiday_cpu import overlap_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ss_state_oracle_pins.npz")
T, SEED, CHAIN, SIGSQ = 70, 4242, 1, 0.7
BETA = np.array([0.5, -0.25, 0.0])
RTOL = 1e-12


def through_the_horizon(blocks, count):
    """the list with every holiday calendar of fewer than `count` entries continued by its own first days"""
    out = []
    for b in blocks:
        if b["kind"] == sho.HOLIDAY and len(b["calendar"]) < count:
            cal = b["calendar"]
            b = dict(b, calendar=np.concatenate([cal, cal[:count - len(cal)]]))
        out.append(b)
    return out


def holiday_lists():
    c = shc.loop_case()
    X, y, obs = shc.data(T)
    yield "loop", c["T"], c["y"], c["X"], c["obs"], c["blocks"]
    yield "list_c", T, y, X, obs, shc.list_c(y, T)
    yield "list_d", T, y, X, obs, shc.list_d(y, T)
    To, yo, obo, blocks, _ = overlap_case()
    yield "overlap", To, yo, None, obo, blocks


def dynreg_lists():
    c = sdc.loop_case()
    X, y, obs = sdc.data(T)
    yield "loop", c["T"], c["y"], c["X"], c["obs"], c["blocks"]
    for name in ("list_edge", "list_two", "list_glob"):
        yield name, T, y, X, obs, getattr(sdc, name)(y, T)


# (a list per calendar, each in another of the shapes: beside a holiday, between seasonals, beside a trig block)
CALENDAR_SHAPES = dict(zip(scc.CALENDARS, ("holiday", "ldc33", "small", "glob")))


def calendar_lists():
    c = scc.loop_case()   # (its calendar ends at T: no step of the forecast starts a season)
    X, y, obs = scc.data(T)
    yield "loop", c["T"], c["y"], c["X"], c["obs"], c["blocks"]
    for name in scc.CALENDARS:
        yield name, T, y, X, obs, scc.calendar_list(y, T, name, CALENDAR_SHAPES[name], extra=scc.HORIZON)


MODULES = dict(holiday=(sho.HolidayOracle, shc.HORIZON, holiday_lists),
               dynreg=(sdo.DynRegOracle, sdc.HORIZON, dynreg_lists),
               calendar=(sco.CalendarOracle, scc.HORIZON, calendar_lists))


def entries():
    for module, (_, _, lists) in MODULES.items():
        for name, *_ in lists():
            yield module, name


def record(oracle, module, name):
    """what one list of one module computes: dict of arrays"""
    cls, horizon, lists = MODULES[module]
    n, y, X, obs, blocks = next(row[1:] for row in lists() if row[0] == name)
    blocks = through_the_horizon(blocks, n + horizon)
    ystar = y if X is None else y - X @ BETA
    o = cls(oracle, n, obs, blocks, SEED, CHAIN)
    out = dict(state=o.impute_state(ystar, SIGSQ).copy())
    out["suf_n"], out["suf_ss"] = np.concatenate(o.suf_n), np.concatenate(o.suf_ss)
    o.draw_state_models()
    out["var"] = np.concatenate(o.var)
    out["forecast"] = o.forecast(out["state"][-1], SIGSQ, np.linspace(-1.0, 1.0, horizon))
    v, F, ll = o.prediction_errors(ystar, SIGSQ)
    out.update(v=v, F=F, loglik=np.array([ll]))
    streams = [o.state_rng, o.forecast_rng] + [r for row in o.var_rng for r in row]
    out["positions"] = np.stack([np.frombuffer(bytes(r), np.uint8) for r in streams])
    return out


EXACT = ("suf_n", "positions")


@pytest.mark.parametrize("module,name", list(entries()))
def test_restatement_computes_what_the_separate_modules_computed(oracle, module, name):
    got = record(oracle, module, name)
    with np.load(GOLDEN) as z:
        want = {k.split("/")[-1]: z[k] for k in z.files if k.startswith("%s/%s/" % (module, name))}
    assert sorted(want) == sorted(got)
    for key in EXACT:
        assert want[key].shape == got[key].shape and np.array_equal(want[key], got[key]), key
    for key in sorted(set(want) - set(EXACT)):
        assert want[key].shape == got[key].shape, key
        err = np.max(np.abs(got[key] - want[key])) / np.abs(want[key]).max()
        print("%s %s %s: relative error %.3e" % (module, name, key, err))
        assert err <= RTOL, key
