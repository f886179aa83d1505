"""With helper wavefronts, EVERY table walk of the sweep kernel runs beside the master's tail
(ssvs_sweep_body.h, PH_FLIPS): not only the one a quiet sweep starts with, but also the walk that
is resumed after a stop -- rebuild or slot switch, table fill, then the rest of the permutation --
and the unforked first walk after a table was built.  The tail's stream position does not depend
on what the walk finds, so the chains must be the same, bit for bit, as with walk policy 4 (fork
at a sweep's start only: the behaviour before) and policy 3 (never fork).  Engines of the same
seed and inputs, one per policy: states, traces, every sweep's recorded draw and the summaries are
compared with np.array_equal, the two counters of the new path excepted."""
import numpy as np
import pytest

from oracle_lib import ssvs_options
from test_partial_rebuild_gpu import CHAINS, _data, _engine
from test_walk_modes_gpu import CASES as WALK_CASES

pytestmark = pytest.mark.gpu

COUNTERS = ("reforks", "refork_rollbacks", "phase_cycles")   # (phase_cycles holds the two counters' slots)
TWO = (150, 150)


def _case(name):
    """(suf, prior, options, tuning, launches, a roll-back is certain)"""
    if name == "A":
        # flips accepted often: resumed walks stop a second time
        return _data("A", "first") + (None, {}, TWO, True)
    if name == "plain_p130":
        # two fill rounds at two wavefronts; a walk longer than one round at four
        suf, prior, opts = WALK_CASES["plain_p130"]
        return suf, prior, opts, {}, TWO, False
    if name == "collinear_swap":
        # a swap proposed by a tail that runs beside a resumed walk
        return _data("A", "first", collinear=[3, 20, 21]) + (ssvs_options(swap_threshold=0.5), {}, TWO, False)
    if name == "prior_means_max_model_size":
        # exact-path stops, rejections, then a resumed walk
        suf, prior, opts = WALK_CASES["general"]
        return suf, prior, opts, {}, TWO, False
    if name == "B_kcap16":
        # a chain that outgrows the capacity inside a resumed walk
        return _data("B", "first") + (None, dict(kcap_start=16), TWO, False)
    assert name == "A_short_launches"
    # pending commits at a launch's end
    return _data("A", "first") + (None, {}, tuple([1] * 7 + [13, 40]), True)


NAMES = ["A", "plain_p130", "collinear_swap", "prior_means_max_model_size", "B_kcap16", "A_short_launches"]


def _run(name, waves, policy):
    import boom_amd
    suf, prior, opts, tuning, launches, _ = _case(name)
    eng = _engine(suf, prior, 0, opts, dict(tuning, waves_per_chain=waves, walk_policy=policy))
    eng.enable_traces(max(launches))
    eng.enable_draws(max(launches))
    out = dict(status=0, draws=[], traces=[])
    try:
        for n in launches:
            eng.sweep(n)
            out["draws"].append([eng.get_draws(c, n) for c in range(CHAINS)])
            out["traces"].append(eng.get_traces(n))
    except boom_amd.BoomAmdError as err:   # (a chain stopped: the same one, the same way, under every policy)
        out["status"] = err.code
    out["states"] = eng.get_states()
    out["summaries"] = eng.get_summaries()
    eng.close()
    return out


def _same(a, b, tag):
    assert a["status"] == b["status"], tag
    for u, v in zip(a["states"], b["states"]):
        assert np.array_equal(u, v), tag
    assert len(a["traces"]) == len(b["traces"]) and len(a["draws"]) == len(b["draws"]), tag
    for ta, tb in zip(a["traces"], b["traces"]):
        for key in ("sigsq", "model_size", "logp"):
            assert np.array_equal(ta[key], tb[key]), (tag, key)
    for la, lb in zip(a["draws"], b["draws"]):
        for c, (da, db) in enumerate(zip(la, lb)):
            for u, v in zip(da, db):
                assert np.array_equal(u, v), (tag, "draw record", c)
    for key, v in a["summaries"].items():
        if key not in COUNTERS:
            assert np.array_equal(v, b["summaries"][key]), (tag, key)


@pytest.mark.parametrize("waves", [2, 4])
@pytest.mark.parametrize("name", NAMES)
def test_resumed_walks_beside_the_tail_give_the_same_chains(name, waves):
    every, start_only, never = (_run(name, waves, policy) for policy in (1, 4, 3))
    _same(every, never, (name, waves, "1 against 3"))
    _same(start_only, never, (name, waves, "4 against 3"))
    se, s4, s3 = every["summaries"], start_only["summaries"], never["summaries"]
    print("%s, %d wavefronts: accepts %d, proposals %d, reforks %d, roll-backs %d"
          % (name, waves, se["accepts"], se["proposals"], se["reforks"], se["refork_rollbacks"]))
    assert se["proposals"] == s4["proposals"] == s3["proposals"], (name, waves)
    # not vacuous: the new path ran, and only under policy 1
    assert se["reforks"] > 0, (name, waves)
    assert se["refork_rollbacks"] <= se["reforks"], (name, waves)
    if _case(name)[5]:
        assert se["refork_rollbacks"] > 0, (name, waves)
    for s in (s4, s3):
        assert s["reforks"] == 0 and s["refork_rollbacks"] == 0, (name, waves)
