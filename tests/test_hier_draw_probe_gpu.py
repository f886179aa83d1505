"""rhh_draw_kernel (boom_amd/csrc/hier_holiday_kernel.hip, mvn_wishart_device.h) launched directly through
tests/cpp/hier_probe.hip: one draw of the hierarchical regression holiday's sampler for given sigma^2, totals,
counts, mu, Omega, hyperparameters and stream position, against the restatement
(tests/ss_hier_regholiday_oracle.py) fed the same Philox stream by the compiled oracle's bo_rnorm / bo_rgamma.

Exact: the stream position after the call (the restatement's generator stands there) and the status.
Within a gate taken from the restatement itself: beta, mu and Omega -- per entry
4 |float64 restatement - long double restatement| + 8 ulp of the largest magnitude of the output the entry
belongs to (a holiday's beta_h, mu, Omega) in the float64 restatement.  mu' (step 2's mean) is no output of the
kernel: every entry of mu and Omega depends on it.  The cases are ss_hier_regholiday_cases.probe_cases; every
case runs on 3 chains with their own sigma^2, totals, mu, Omega and positions, the model in slot 1 of the list
at coefficient offset 7 where it fits (a slot or an offset taken for 0 would show).
Worst ratio to the gate seen on an MI355X: see DESIGN.md 3.26."""
import numpy as np
import pytest

import hier_probe_lib as hpl
import ss_hier_regholiday_cases as hrc
import ss_hier_regholiday_oracle as hro

gpu = pytest.mark.gpu
SEED = 0x5EED0123456789
CHAINS = 3
CASES = hrc.probe_cases()


@pytest.fixture(scope="module")
def lib():
    L = hpl.load()
    assert L.hp_stream() == hro.STREAM and L.hp_bad_draw() == hro.BAD_DRAW
    return L


def chain_inputs(case, c):
    """chain c's own inputs: chain 0 the case's, the others scaled copies (exact scalings of mu and the totals,
    another sigma^2 and position)"""
    f = 1.0 + 0.5 * c
    return dict(sigsq=case["sigsq"] * f, totals=case["totals"] * f, mu=case["mu"] * (1.0 - 0.25 * c), omega=case["omega"] * f,
                coef=case["coef"] + c, pos=case["pos"] + 1000 * c)


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_draw_matches_restatement(lib, oracle, case):
    d, H = case["d"], case["H"]
    slot, base = (1, 7) if H * d + 7 <= lib.hp_max_coef() else (0, 0)
    ins = [chain_inputs(case, c) for c in range(CHAINS)]
    hy = hro.hyper(case["model"])
    got = hpl.draw(lib, d, H, case["nu0"], hy, [i["sigsq"] for i in ins], case["counts"].reshape(-1),
                   np.array([i["totals"].reshape(-1) for i in ins]), np.array([i["coef"].reshape(-1) for i in ins]),
                   np.array([i["mu"] for i in ins]), np.array([i["omega"] for i in ins]), [i["pos"] for i in ins], SEED,
                   slot=slot, base=base)
    worst = 0.0
    for c, i in enumerate(ins):
        if case["bad"]:
            assert got["status"][c] == hro.BAD_DRAW
            assert got["pos"][c] == i["pos"]
            assert np.array_equal(got["coef"][c], i["coef"].reshape(-1)) and np.array_equal(got["mu"][c], i["mu"])
            assert np.array_equal(got["omega"][c], i["omega"])
            continue
        src = hro.PhiloxDraws(oracle, SEED, c, pos=i["pos"])
        lo, hi = hro.draw_both(case["model"], i["sigsq"], i["totals"], case["counts"], i["mu"], i["omega"], src)
        assert src.status.value == 0
        assert got["status"][c] == 0, (c, got["status"])
        assert got["pos"][c] == src.pos, (c, got["pos"][c], src.pos, i["pos"])
        assert src.pos - i["pos"] >= hro.count_draws(H, d)
        dev = dict(mu=got["mu"][c], omega=got["omega"][c])
        for h in range(H):
            dev["beta %d" % h] = got["coef"][c].reshape(H, d)[h]
        want = dict(mu=(lo["mu"], hi["mu"]), omega=(lo["omega"], hi["omega"]))
        for h in range(H):
            want["beta %d" % h] = (lo["beta"][h], hi["beta"][h])
        for key, (l, hh) in want.items():
            g = hro.gate(l, hh, float(np.max(np.abs(l))))
            ratio = float(np.max(np.abs(dev[key] - l) / g))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (case["name"], c, key, dev[key], l, g)
        assert np.array_equal(dev["omega"], dev["omega"].T)
    print("%s: worst error / gate %.3e" % (case["name"], worst))
