"""A forked sweep's shuffle targets are drawn by wave 1 alone when a chain has two wavefronts (the
master goes straight to the tail and the fork has one barrier less: fork_shuffle_targets,
ssvs_device.h) -- behind the last join, ahead of the fork's command, when that join's walk found no
stop and the tail's end told it where the next sweep starts; at the command otherwise (a launch's
first fork, a sweep after a stop that was not walked again, a guess that missed) -- and by all
wavefronts together when it has four.  Which lane computes which Philox block, and when, is all
that moves, so whole chains must be the same, bit for bit, as with walk policy 3, which never
forks and draws the targets with all threads on a command of its own.

Engines of the same seed and inputs, one per policy: states, traces, every sweep's recorded draw
and the summaries are compared with np.array_equal, the path counters excepted.  Cases: plain_p130
(three lanes' worth of blocks, a walk longer than one round) and A (flips accepted often: stops,
rebuilds and forks again in most sweeps).  Launches: two of 150 sweeps, and 1 x 7, 13, 40 -- a
commit is pending at every launch's end, and the sweeps' stream positions start at both
parities."""
import pytest

from test_partial_rebuild_gpu import CHAINS, _data, _engine
from test_refork_gpu import _same
from test_walk_modes_gpu import CASES as WALK_CASES

pytestmark = pytest.mark.gpu

LAUNCHES = {"two_150": (150, 150), "short": (1,) * 7 + (13, 40)}


def _case(name):
    """(suf, prior, options, stops are certain)"""
    if name == "A":
        return _data("A", "first") + (None, True)
    assert name == "plain_p130"
    return WALK_CASES["plain_p130"] + (False,)


def _run(name, waves, policy, launches):
    import boom_amd
    suf, prior, opts, _ = _case(name)
    eng = _engine(suf, prior, 0, opts, dict(waves_per_chain=waves, walk_policy=policy))
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


@pytest.mark.parametrize("launches", sorted(LAUNCHES))
@pytest.mark.parametrize("waves", [2, 4])
@pytest.mark.parametrize("name", ["plain_p130", "A"])
def test_forked_sweeps_give_the_chains_of_unforked_ones(name, waves, launches):
    forked, never = (_run(name, waves, policy, LAUNCHES[launches]) for policy in (1, 3))
    assert forked["status"] == 0, (name, waves, launches)
    _same(forked, never, (name, waves, launches, "1 against 3"))
    sf, sn = forked["summaries"], never["summaries"]
    print("%s, %d wavefronts, %s: accepts %d, proposals %d, reforks %d, roll-backs %d"
          % (name, waves, launches, sf["accepts"], sf["proposals"], sf["reforks"], sf["refork_rollbacks"]))
    assert sf["proposals"] == sn["proposals"] > 0, (name, waves, launches)
    # not vacuous: policy 3 never forked, and where stops are certain policy 1 forked again after them
    assert sn["reforks"] == 0 and sn["refork_rollbacks"] == 0, (name, waves, launches)
    if _case(name)[3]:
        assert sf["accepts"] > 0 and sf["reforks"] > 0, (name, waves, launches)
