"""After ONE variable enters or leaves the model at position q of the sorted list, the sweep
kernels keep columns < q of both Cholesky factors and compute only the new row and the columns
from q on (ssvs_device.h: refactor; ba_set_rebuild_policy 0).  A left-looking column reads
nothing right of itself, so the kept columns ARE what a factorisation from scratch computes --
and so every number the sampler produces must be the same, bit for bit, as with policy 1
(always from scratch), which the oracle-parity tests pin to the reference.  Two engines of the
same seed and inputs, one per policy: states, traces, every sweep's recorded draw and the
summaries are compared with np.array_equal."""
import numpy as np
import pytest

from cases import bsts_priors, regression_data, spike_slab_prior, state_space_data, suf_from_xy
from oracle_lib import ssvs_options

pytestmark = pytest.mark.gpu

CHAINS, LAUNCHES, SEED = 64, (150, 150), 4242
COUNTERS = ("partial_rebuilds", "columns_kept", "phase_cycles")   # (phase_cycles holds the two counters' slots)


def _layout(p, nsig, how):
    """column order of the design: signals first (as generated), columns 1..p-1 reversed
    (signals last: a noise variable enters at the FRONT of the list), signals in the middle"""
    if how == "first":
        return np.arange(p)
    if how == "reversed":
        return np.concatenate([[0], np.arange(p - 1, 0, -1)])
    noise = np.arange(nsig, p)
    h = len(noise) // 2
    return np.concatenate([[0], noise[:h], np.arange(1, nsig), noise[h:]])


_DATA = {}


def _data(case, how, collinear=None):
    """(suf, prior) of case A / B in one column layout: computed once, shared, never changed"""
    key = (case, how, None if collinear is None else tuple(collinear))
    if key not in _DATA:
        n, p, nsig, ems = {"A": (300, 40, 7, 12), "B": (300, 72, 15, 22)}[case]
        X, y, _ = regression_data(n, p, nsig, seed=11, noise_sd=3.0, collinear=collinear)
        X = np.ascontiguousarray(X[:, _layout(p, nsig, how)])
        suf = suf_from_xy(X, y)
        _DATA[key] = (suf, spike_slab_prior(suf, ems))
    return _DATA[key]


def _engine(suf, prior, policy, opts=None, tuning=None):
    import boom_amd
    eng = boom_amd.Engine(CHAINS, seed=SEED)
    if tuning:
        eng.set_tuning(**tuning)
    eng.set_rebuild_policy(policy)
    eng.upload_suf(suf["xtx"], suf["xty"], suf["yty"], suf["n"], suf["sumy"] / suf["n"], suf["xsum"] / suf["n"])
    opts = opts or ssvs_options()
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"],
                   max_model_size=opts["max_model_size"], sigma_upper_limit=opts["sigma_upper_limit"])
    eng.set_options(max_flips=opts["max_flips"], swap_threshold=opts["swap_threshold"])
    p = len(suf["xty"])
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    eng.set_state(g0)
    return eng


def _run(suf, prior, policy, opts=None, tuning=None):
    """300 sweeps in two launches (the second starts from the kept model block: the
    launch-start restore); everything the engine lets a caller see"""
    import boom_amd
    eng = _engine(suf, prior, policy, opts, tuning)
    eng.enable_traces(max(LAUNCHES))    # (traces and the draw record are those of the last sweep call)
    eng.enable_draws(max(LAUNCHES))
    out = dict(status=0, draws=[], traces=[])
    try:
        for n in LAUNCHES:
            eng.sweep(n)
            out["draws"].append([eng.get_draws(c, n) for c in range(CHAINS)])
            out["traces"].append(eng.get_traces(n))
    except boom_amd.BoomAmdError as err:   # (a chain stopped: the same one, the same way, under both policies)
        out["status"] = err.code
    out["states"] = eng.get_states()
    out["summaries"] = eng.get_summaries()
    eng.close()
    if len(out["traces"]) == len(LAUNCHES):
        out["model_size"] = np.concatenate([t["model_size"] for t in out["traces"]], axis=1)
    return out


def _same(a, b, tag):
    assert a["status"] == b["status"], tag
    for u, v in zip(a["states"], b["states"]):
        assert np.array_equal(u, v), tag
    assert len(a["traces"]) == len(b["traces"]) and len(a["draws"]) == len(b["draws"]), tag
    for ta, tb in zip(a["traces"], b["traces"]):
        for name in ("sigsq", "model_size", "logp"):
            assert np.array_equal(ta[name], tb[name]), (tag, name)
    for la, lb in zip(a["draws"], b["draws"]):
        for c, (da, db) in enumerate(zip(la, lb)):
            for u, v in zip(da, db):
                assert np.array_equal(u, v), (tag, "draw record", c)
    for name, v in a["summaries"].items():
        if name not in COUNTERS:
            assert np.array_equal(v, b["summaries"][name]), (tag, name)


def _both(suf, prior, tag, opts=None, tuning=None):
    part = _run(suf, prior, 0, opts, tuning)
    full = _run(suf, prior, 1, opts, tuning)
    _same(part, full, tag)
    # not vacuous: the partial path ran, and only under policy 0
    sp, sf = part["summaries"], full["summaries"]
    print("%s: accepts %d, partial rebuilds %d, columns kept per partial rebuild %.2f, mean model size %.2f"
          % (tag, sp["accepts"], sp["partial_rebuilds"], sp["columns_kept"] / max(sp["partial_rebuilds"], 1),
             sp["k_sum"] / max(sp["sweeps"], 1)))
    assert sp["partial_rebuilds"] > 0, tag
    assert sf["partial_rebuilds"] == 0 and sf["columns_kept"] == 0, tag
    return part


def _crosses(ksize, edge):
    """a chain's model size on both sides of `edge` in consecutive sweeps, each way"""
    lo, hi = ksize[:, :-1] <= edge, ksize[:, 1:] > edge
    up = np.any(lo & hi)
    down = np.any((ksize[:, :-1] > edge) & (ksize[:, 1:] <= edge))
    return bool(up and down)


@pytest.mark.parametrize("how", ["first", "reversed", "middle"])
@pytest.mark.parametrize("case,edge", [("A", 8), ("B", 16)])
def test_both_policies_give_the_same_chains(case, edge, how):
    suf, prior = _data(case, how)
    part = _both(suf, prior, (case, how))
    sm = part["summaries"]
    kept = sm["columns_kept"] / sm["partial_rebuilds"]
    kbar = sm["k_sum"] / sm["sweeps"]
    if how == "first":
        # a noise variable enters at the end of the list (k - 1 columns of the new model kept)
        # and leaves from there (all k kept): within 2 of the mean model size
        assert kept > kbar - 2.0, (case, how, kept, kbar)
    elif how == "reversed":
        # ... right behind the intercept: one column kept
        assert kept < 2.0, (case, how, kept)
    # the 8-row block boundary of the packed factors is crossed, growing and shrinking
    assert _crosses(part["model_size"], edge), (case, how)


def test_capacity_hand_over():
    """case B from capacity 16: chains outgrow it and go on in the next kernel instance"""
    suf, prior = _data("B", "first")
    _both(suf, prior, "B kcap_start 16", tuning=dict(kcap_start=16))


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_wavefronts_per_chain(waves):
    suf, prior = _data("A", "first")
    _both(suf, prior, ("A waves", waves), tuning=dict(waves_per_chain=waves))


@pytest.mark.parametrize("walk", [0, 2])
def test_walk_policies(walk):
    suf, prior = _data("A", "first")
    _both(suf, prior, ("A walk", walk), tuning=dict(walk_policy=walk))


def test_exact_evaluations_reject_and_restore():
    """a non-zero prior mean on three noise variables: their flips are evaluated exactly
    (EV_TRY), most are rejected, and the old factors come back from the chain's block"""
    suf, _ = _data("A", "first")
    pm = np.zeros(40)
    pm[0] = suf["sumy"] / suf["n"]
    pm[[20, 25, 31]] = [0.3, -0.2, 0.25]
    prior = spike_slab_prior(suf, 12, prior_mean=pm)
    _both(suf, prior, "A prior mean")


def test_collinear_design_with_swaps():
    """near copies of a column: the swap move (two flips: always from scratch) runs between
    partial rebuilds, and a factorisation may fail -- the same status and states either way"""
    suf, prior = _data("A", "first", collinear=[3, 20, 21])
    _both(suf, prior, "A collinear", opts=ssvs_options(swap_threshold=0.5))


def test_sigma_conditional_sampler():
    """SpikeSlabSampler (mode 1): the matrices scaled by 1 / sigma^2, which stays put
    inside a launch"""
    import boom_amd
    suf, prior = _data("A", "first")
    p = len(suf["xty"])
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    got = []
    for policy in (0, 1):
        eng = boom_amd.Engine(CHAINS, seed=SEED)
        eng.set_rebuild_policy(policy)
        eng.upload_suf(suf["xtx"], suf["xty"], suf["yty"], suf["n"], suf["sumy"] / suf["n"], suf["xsum"] / suf["n"])
        eng.sss_set_slab(prior["b"], prior["ominv"], scales_with_sigsq=True)
        eng.set_spike(prior["pi"])
        eng.set_state(g0)
        eng.enable_traces(max(LAUNCHES))
        traces = []
        for i, n in enumerate(LAUNCHES):
            eng.set_sigsq(9.0 + i)
            eng.sss_sweep(n)
            traces.append(eng.get_traces(n))
        got.append((eng.get_states(), traces, eng.get_summaries()))
        eng.close()
    (sa, ta, ma), (sb, tb, mb) = got
    for u, v in zip(sa, sb):
        assert np.array_equal(u, v)
    for x, z in zip(ta, tb):
        for name in x:
            assert np.array_equal(x[name], z[name]), name
    for name, v in ma.items():
        if name not in COUNTERS:
            assert np.array_equal(v, mb[name]), name
    assert ma["partial_rebuilds"] > 0 and mb["partial_rebuilds"] == 0


def test_bsts_rounds():
    """the persistent round kernel instantiates the same rebuild site; 40 rounds at the
    smallest shape of test_ss_round_kernel_gpu.py (one signal and an expected model size of
    one, so that the regressors are not all forced in and flips happen)"""
    import boom_amd
    T, p, chains = 17, 3, 16
    X, y, _, obs = state_space_data(T, p, 1, seed=5, missing_frac=0.0)
    prior, ss, sig_up = bsts_priors(X, y, 1)
    got = []
    for policy in (0, 1):
        eng = boom_amd.Engine(chains, seed=77)
        eng.set_rebuild_policy(policy)
        eng.ss_set_data(y, X, obs)
        eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"],
                       sigma_upper_limit=sig_up)
        eng.ss_set_local_level(ss["level_df"], ss["level_sigma_guess"], ss["level_sigma_upper_limit"],
                               ss["initial_state_mean"], ss["initial_state_variance"], ss["initial_level_sigma"])
        eng.set_state(np.zeros(p, np.uint8))
        eng.ss_set_tuning(kernel=5)
        eng.ss_sweep(40)
        st = [eng.ss_get_state(c) for c in range(chains)]
        got.append((eng.get_states(), st, eng.get_summaries()))
        eng.close()
    (sa, xa, ma), (sb, xb, mb) = got
    for u, v in zip(sa, sb):
        assert np.array_equal(u, v)
    for c in range(chains):
        assert xa[c]["level_sigsq"] == xb[c]["level_sigsq"], c
        assert np.array_equal(xa[c]["state"], xb[c]["state"]), c
    for name, v in ma.items():
        if name not in COUNTERS:
            assert np.array_equal(v, mb[name]), name
    print("bsts: accepts %d, partial rebuilds %d" % (ma["accepts"], ma["partial_rebuilds"]))
    assert ma["partial_rebuilds"] > 0 and mb["partial_rebuilds"] == 0
