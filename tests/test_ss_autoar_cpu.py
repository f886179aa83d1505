"""The restatement of ArSpikeSlabSampler (tests/ss_autoar_oracle.py, the yardstick of state model
kind 9) against the oracle's sigma^2-conditional SpikeSlabSampler (bo_sss_*, slab kind 0, shuffle
kind 0), and the properties the GPU tests (tests/test_ss_autoar_gpu.py) lean on.  No GPU."""
import copy
import ctypes as C

import numpy as np
import pytest

import autoar_cases as ac
import ss_autoar_oracle as sao
from oracle_lib import _dp, _u8, f64, fcol

SEED = 9901


def sss_handle(o, S, suf):
    o._declare_sss()
    L = o.lib
    L.bo_sss_log_model_prob.restype = C.c_double
    L.bo_sss_log_model_prob.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_double]
    h = L.bo_sss_create(S.L, _dp(fcol(suf["xtx"])), _dp(f64(suf["xty"])), 0, _dp(f64(S.mu)), _dp(fcol(S.siginv)),
                        _dp(f64(S.pi)))
    L.bo_sss_set_options(h, -1, int(S.max_flips))
    return h


def pi_of(kind, L):
    if kind == "half":
        return np.full(L, 0.5)
    pi = np.full(L, 0.4)
    pi[0] = 1.0
    if L > 1:
        pi[-1] = 0.0
    return pi


CASES = [(L, kind, flips) for L in (1, 2, 4, 16) for kind in ("half", "01") for flips in (-1, 2)]


@pytest.mark.parametrize("L,pikind,flips", CASES)
def test_restatement_matches_spike_slab_sampler(oracle, L, pikind, flips):
    """log_model_prob, the indicator sweep and the coefficient draw: 1e-12 relative, gamma and the
    stream position bit for bit, 8 sweeps on random statistics; the empty model included"""
    o = oracle
    suf = ac.random_suf(L, 40 + L)
    mu, P = ac.slab(L, 7 + L)
    S = sao.AutoArSampler(o, L, mu, P, pi_of(pikind, L), 3.0, 0.5, max_flips=flips)
    h = sss_handle(o, S, suf)
    lib = o.lib
    rs = np.random.Generator(np.random.PCG64(L))
    # log_model_prob on random models, the empty and the full one
    models = [np.zeros(L, np.uint8), np.ones(L, np.uint8)] + [(rs.uniform(size=L) < 0.5).astype(np.uint8) for _ in range(6)]
    for g in models:
        for s2 in (0.3, 2.0):
            a = S.log_model_prob(g, suf["xtx"], suf["xty"], s2)
            b = lib.bo_sss_log_model_prob(h, _u8(np.ascontiguousarray(g)), s2)
            assert (a == b) or abs(a - b) <= 1e-12 * max(abs(b), 1.0), (g, s2, a, b)
    # the sweep and the draw, from every lag included (ArModel's start) and from the empty model
    for start in (np.ones(L, np.uint8), np.zeros(L, np.uint8)):
        lib.bo_rng_seed_philox(lib.bo_sss_rng(h), SEED, L, 12, 0)
        rng = sao.fresh_rng(o, SEED, L, 12)
        g = start.copy()
        lib.bo_sss_set_state(h, _u8(np.ascontiguousarray(g)), _dp(np.zeros(L)))
        gref, bref = np.zeros(L, np.uint8), np.zeros(L)
        for it in range(8):
            s2 = 0.2 + 0.3 * it
            assert lib.bo_sss_draw_model_indicators(h, s2) == 0
            assert lib.bo_sss_draw_beta(h, s2) == 0
            lib.bo_sss_get_state(h, _u8(gref), _dp(bref))
            g = S.draw_model_indicators(rng, g, suf["xtx"], suf["xty"], s2)
            beta = S.draw_beta(rng, g, suf["xtx"], suf["xty"], s2)
            assert np.array_equal(g, gref), (it, g, gref)
            ref_rng = C.cast(lib.bo_sss_rng(h), C.POINTER(sao.BoRng)).contents
            assert rng.pos == ref_rng.pos, (it, rng.pos, ref_rng.pos)
            assert np.all(np.abs(beta - bref) <= 1e-12 * np.maximum(np.abs(bref), 1.0)), (it, beta, bref)
    lib.bo_sss_destroy(h)


def test_empty_model_draws_nothing(oracle):
    """pi = 0 everywhere: make_valid empties the model, draw_beta draws nothing, sigma^2 comes from yty"""
    L = 3
    suf = ac.random_suf(L, 3)
    mu, P = ac.slab(L, 3)
    S = sao.AutoArSampler(oracle, L, mu, P, np.zeros(L), 3.0, 0.5, select=True)
    rng = sao.fresh_rng(oracle, SEED, 0, 12)
    g, phi, s2 = S.draw(rng, np.ones(L, np.uint8), np.full(L, 0.1), 1.0, suf)
    assert not g.any() and not phi.any()
    # shuffle: L - 1 uniforms; L flips: one each; then the gamma draw of sigma^2 alone
    r2 = sao.fresh_rng(oracle, SEED, 0, 12, pos=(L - 1) + L)
    want = 1.0 / oracle.gammas(r2, (suf["n"] + 3.0) / 2, (suf["yty"] + 3.0 * 0.25) / 2, 1)[0]
    assert s2 == want and rng.pos == r2.pos


@pytest.mark.parametrize("L", [2, 4, 16])
def test_univariate_conditionals_match_the_dense_formula(oracle, L):
    """the swept precision's row against m_i - sum_{j != i} P_ij (phi_j - m_j) / P_ii and 1 / P_ii"""
    suf = ac.random_suf(L, 11 + L)
    mu, P = ac.slab(L, 2 + L)
    S = sao.AutoArSampler(oracle, L, mu, P, np.full(L, 0.5), 3.0, 0.5)
    g = np.ones(L, np.uint8)
    if L > 2:
        g[1] = 0
    idx, prec, _, mean = S.posterior(g, suf["xtx"], suf["xty"], 0.7)
    rs = np.random.Generator(np.random.PCG64(L))
    phi = 0.1 * rs.standard_normal(len(idx))
    V = np.linalg.inv(prec)
    for i in range(len(idx)):
        cm, csd = S.univariate_conditional(prec, mean, phi, i)
        others = [j for j in range(len(idx)) if j != i]
        dense = mean[i] - sum(prec[i, j] * (phi[j] - mean[j]) for j in others) / prec[i, i]
        assert abs(cm - dense) <= 1e-12 * max(abs(dense), 1.0)
        assert abs(csd - np.sqrt(1.0 / prec[i, i])) <= 1e-15 * csd
        # ... which is the Gaussian conditional: V_io V_oo^-1 (phi_o - m_o), V_ii - V_io V_oo^-1 V_oi
        Voo = V[np.ix_(others, others)]
        gauss = mean[i] + V[i, others] @ np.linalg.solve(Voo, phi[others] - mean[others])
        assert abs(cm - gauss) <= 1e-9 * max(abs(gauss), 1.0)
        assert abs(csd ** 2 - (V[i, i] - V[i, others] @ np.linalg.solve(Voo, V[others, i]))) <= 1e-9 * csd ** 2


@pytest.mark.parametrize("case", ac.LOOP_CASES + ac.FALLBACK_CASES, ids=lambda c: c["name"])
def test_gpu_cases_decide_with_margin(oracle, case):
    """the GPU tests' priors, seeds and streams on statistics of the cases' size: every decision of the
    reference (flips, stationarity tests) has a margin above 1e-9, and the fallback cases really fail
    100 proposals.  (The GPU tests assert the same of the restatement on the device's own statistics.)"""
    c = ac.loop_case(case)
    b = c["blocks"][c["block"]]
    L = b["lags"]
    S = ac.sampler_of(oracle, b)
    suf = ac.random_suf(L, case["data_seed"], n=c["T"])
    fallback = case in ac.FALLBACK_CASES
    if fallback:
        # a near-unit-root series' statistics
        rs = np.random.Generator(np.random.PCG64(case["data_seed"]))
        u = np.cumsum(0.3 * rs.standard_normal(c["T"] + L))
        Xl = np.stack([u[L - 1 - i:len(u) - 1 - i] for i in range(L)], axis=1)
        suf = dict(xtx=Xl.T @ Xl, xty=Xl.T @ u[L:], yty=float(u[L:] @ u[L:]), n=float(c["T"]))
    for chain in c["check"]:
        rng = sao.fresh_rng(oracle, c["seed"], chain, sao.ar_stream_id(c["blocks"], c["block"]))
        g, phi, s2 = np.ones(L, np.uint8), np.array(b["initial_phi"], float), float(b["initial_sigma"][0]) ** 2
        for _ in range(c["rounds"]):
            g, phi, s2 = S.draw(rng, g, phi, s2, suf)
            if fallback:
                assert S.proposals == 100 and S.univariate and not S.caught
            if b["truncate"]:
                assert oracle.lib.bo_test_ar_check_stationary(L, _dp(np.ascontiguousarray(phi)))
            assert np.all(phi[g == 0] == 0.0)
    assert S.margin > 1e-9, S.margin


def test_long_double_evaluation_reads_the_same_numbers(oracle):
    """the extended-precision evaluation consumes the stream as the double one does and differs from it
    by rounding only: the difference is the GPU tests' gate"""
    L = 4
    suf = ac.random_suf(L, 5)
    mu, P = ac.slab(L, 9)
    out = []
    for ft in (np.float64, np.longdouble):
        S = sao.AutoArSampler(oracle, L, mu, P, np.full(L, 0.5), 3.0, 0.5, dtype=ft)
        rng = sao.fresh_rng(oracle, SEED, 1, 12)
        g, phi, s2 = np.ones(L, np.uint8), np.zeros(L), 1.0
        for _ in range(5):
            g, phi, s2 = S.draw(rng, g, phi, s2, suf)
        out.append((g, phi, s2, rng.pos))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][3] == out[1][3]
    assert np.max(np.abs(out[0][1] - out[1][1])) < 1e-12 and abs(out[0][2] - out[1][2]) < 1e-12 * out[0][2]


@pytest.mark.parametrize("L,upper", [(1, None), (2, np.inf), (4, None), (4, np.inf)])
def test_sigma_step_matches_the_plain_ar_path(oracle, L, upper):
    """every lag included: draw_sigma_full_conditional is ArPosteriorSampler::draw_sigma.  bo_ssm runs
    [local level, Ar(L)] with the proposals' normals on a global generator of their own, so that the
    block's stream is read by the sigma draw alone; a copy of that stream taken before a round, the
    ArSuf before it and phi after it must give the round's sigma^2 and leave the stream where bo_ssm
    left it.  (relative_sse adds yty first where the plain sampler adds it last: 1e-12, not bits.)"""
    from cases import bsts_priors, general_data, general_spec
    from oracle_lib import ssvs_options
    o, lib = oracle, oracle.lib
    T, p, seed, chain = 60, 3, 4400 + L, 1
    X, y, _, _ = general_data(T, p, 2, [], seed=30 + L, ar_coef=[0.5, -0.2][:min(L, 2)])
    blocks = general_spec(y, [("level",), ("ar", L)])
    b = blocks[1]
    b["df"], b["sigma_guess"] = np.array([3.0]), np.array([0.5])
    if upper is not None:
        b["sigma_upper_limit"] = np.array([upper])
    prior, _, sig_up = bsts_priors(X, y, 2)
    m = o._ssg_build(y, X, None, prior, blocks)
    reg = lib.bo_ssm_regression(m)
    opts = ssvs_options(sigma_upper_limit=sig_up)
    lib.bo_ssvs_set_options(reg, opts["max_model_size"], opts["sigma_upper_limit"], opts["swap_threshold"],
                            opts["max_flips"], opts["draw_beta"], opts["draw_sigma"])
    lib.bo_ssvs_set_state(reg, _u8(np.zeros(p, np.uint8)), _dp(np.zeros(p)), 1.0)
    lib.bo_rng_seed_philox(lib.bo_ssvs_rng(reg), seed, chain, 0, 0)
    lib.bo_rng_seed_philox(C.c_void_p(lib.bo_ssm_block_rng(m, 0, 0)), seed, chain, 1, 0)
    ar_rng = C.cast(lib.bo_ssm_block_rng(m, 1, 0), C.POINTER(sao.BoRng))
    lib.bo_rng_seed_philox(ar_rng, seed, chain, 12, 0)
    lib.bo_rng_seed_philox(lib.bo_ssm_state_rng(m), seed, chain, 2, 0)
    glob = sao.fresh_rng(o, seed, chain, 99)
    lib.bo_ssm_set_global_rng.argtypes = [C.c_void_p, C.c_void_p]
    lib.bo_ssm_set_global_rng(m, C.byref(glob))
    lib.bo_ssm_block_get_ar_suf.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                            C.POINTER(C.c_double), C.POINTER(C.c_double)]
    S = sao.AutoArSampler(o, L, np.zeros(L), np.eye(L), np.full(L, 0.5), 3.0, 0.5, float(b["sigma_upper_limit"][0]))
    assert lib.bo_ssm_draw(m) == 0   # (the first round's statistics are empty: compare from the second on)
    moved = 0
    for r in range(6):
        xtx, xty = np.zeros((L, L)), np.zeros(L)
        yty, n = C.c_double(), C.c_double()
        lib.bo_ssm_block_get_ar_suf(m, 1, _dp(xtx), _dp(xty), C.byref(yty), C.byref(n))
        mine = copy.copy(ar_rng.contents)
        before = mine.pos
        assert lib.bo_ssm_draw(m) == 0
        s2, phi = np.zeros(2), np.zeros(16)
        lib.bo_ssm_block_get(m, 1, _dp(s2), None, None, _dp(phi))
        got = S.draw_sigma(mine, np.ones(L, np.uint8), phi[:L], xtx, (xty, yty.value), n.value)
        assert abs(got - s2[0]) <= 1e-12 * s2[0], (r, got, s2[0])
        assert mine.pos == ar_rng.contents.pos, (r, mine.pos, ar_rng.contents.pos)
        moved += mine.pos - before
    assert moved > 0
    lib.bo_ssm_destroy(m)
