"""The spike-and-slab autoregression state model on the device (ba_ss_add_state_model kind 9, bsts
AddAutoAr: an ArStateModel drawn by ArSpikeSlabSampler) -- ar_spike_kernel.hip and its plumbing --
against the restatement tests/ss_autoar_oracle.py.

  sampler alone  ba_ss_impute_state, then 12 x (ba_ss_autoar_draw_parameters; ba_ss_impute_state); each
                 round the restatement is fed the device's own ArSuf and (gamma, phi, sigma^2)
  fallback       cases whose 100 multivariate proposals all fail: draw_phi_univariate
  whole rounds   ba_ss_sweep(1) x 12; ba_ss_sweep(12) the same bits
  equivalence    a kind-9 block is a kind-4 block to the state draw, the forecast and the filter
  look-ahead     8 against 1, bit for bit; the kernel classes launched
  distribution   4096 chains' model frequencies against the exact posterior
  interface      refusals, ba_seed, the pybind classes

The comparison's gate comes from the reference alone: 8 x the deviation between the restatement in
float64 and in long double (same random numbers, same decisions) on that very draw, with a floor of
64 unit roundoffs of the value's scale.  gamma must agree exactly; the stream position is checked by
the restatement's generator running on from round to round without ever being set from the device: a
draw that consumed another count of numbers puts every later round off.
"""
import copy

import numpy as np
import pytest

import autoar_cases as ac
import ss_autoar_oracle as sao
from cases import bsts_priors, general_data, general_spec
from ss_gpu_helpers import refused

gpu = pytest.mark.gpu
U = 2.0 ** -53
RATIOS = {}   # case -> the worst device-to-gate ratios (printed; DESIGN 3.20 tabulates them)


def engine(chains, seed, y, X, obs, blocks, g0=None, kernel=None):
    import boom_amd
    prior, _, sig_up = bsts_priors(X, y, 2)
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_set_data(y, X, obs)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"],
                   sigma_upper_limit=sig_up)
    eng.ss_set_state_models(blocks)
    if kernel is not None:
        eng.ss_set_tuning(kernel=kernel)
    eng.set_state(np.zeros(X.shape[1], np.uint8) if g0 is None else g0)
    return eng


def loop_engine(c):
    eng = engine(c["chains"], c["seed"], c["y"], c["X"], c["obs"], c["blocks"], c["gam"][0])
    for ch in range(c["chains"]):
        eng.set_state(c["gam"][ch], c["beta"][ch], c["sigsq"], chain=ch)
    return eng


def device_state(eng, chain, block):
    sm = eng.ss_get_state_model(chain, block)
    return dict(gamma=eng.ss_get_ar_inclusion(chain, block), phi=sm["phi"], sigsq=float(sm["variances"][0]),
                suf=dict(xtx=sm["xtx"], xty=sm["xty"], yty=sm["yty"], n=sm["n"]))


class Follower:
    """the restatement of one chain's sampler of one block, in float64 and in long double on copies of
    the same generator; check() takes one draw from the state the device had and compares"""

    def __init__(self, o, blocks, block, seed, chain):
        self.S = ac.sampler_of(o, blocks[block])
        self.S80 = ac.sampler_of(o, blocks[block], dtype=np.longdouble)
        self.rng = sao.fresh_rng(o, seed, chain, sao.ar_stream_id(blocks, block))
        self.worst = dict(phi=0.0, sigsq=0.0)

    def check(self, before, after, tag):
        r80 = copy.copy(self.rng)
        g, phi, s2 = self.S.draw(self.rng, before["gamma"], before["phi"], before["sigsq"], before["suf"])
        g80, phi80, s280 = self.S80.draw(r80, before["gamma"], before["phi"], before["sigsq"], before["suf"])
        # (the gate means something only if both evaluations took the same decisions)
        assert np.array_equal(g, g80) and r80.pos == self.rng.pos, tag
        assert np.array_equal(after["gamma"], g), (tag, after["gamma"], g)
        assert np.all(after["phi"][g == 0] == 0.0), tag
        gate_phi = np.maximum(8 * np.abs(phi - phi80), 64 * U * max(np.max(np.abs(phi)), 1e-300))
        gate_s2 = max(8 * abs(s2 - s280), 64 * U * s2)
        rp = float(np.max(np.abs(after["phi"] - phi) / gate_phi)) if len(phi) else 0.0
        rs = abs(after["sigsq"] - s2) / gate_s2
        print("%s  phi ratio %.3f  sigsq ratio %.3f" % (tag, rp, rs))
        self.worst["phi"] = max(self.worst["phi"], rp)
        self.worst["sigsq"] = max(self.worst["sigsq"], rs)
        assert rp <= 1.0, (tag, after["phi"], phi, gate_phi)
        assert rs <= 1.0, (tag, after["sigsq"], s2, gate_s2)


def run_loop(oracle, case, fallback=False):
    c = ac.loop_case(case)
    eng = loop_engine(c)
    k = c["block"]
    eng.ss_impute_state()
    F = {ch: Follower(oracle, c["blocks"], k, c["seed"], ch) for ch in c["check"]}
    for r in range(c["rounds"]):
        before = {ch: device_state(eng, ch, k) for ch in c["check"]}
        eng.ss_autoar_draw_parameters()
        for ch in c["check"]:
            F[ch].check(before[ch], device_state(eng, ch, k), "%s round %d chain %d" % (c["name"], r, ch))
            if fallback:
                assert F[ch].S.proposals == 100 and F[ch].S.univariate and not F[ch].S.caught
        eng.ss_impute_state()
    for ch in c["check"]:
        assert F[ch].S.margin > 1e-9, F[ch].S.margin   # (the reference decided nothing by a hair)
    RATIOS[c["name"]] = {q: max(F[ch].worst[q] for ch in c["check"]) for q in ("phi", "sigsq")}
    print("worst ratios", c["name"], RATIOS[c["name"]])


# ---- 1, 2: the sampler alone --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", ac.LOOP_CASES, ids=lambda c: c["name"])
def test_sampler_alone_matches_restatement(oracle, case):
    run_loop(oracle, case)


@gpu
@pytest.mark.parametrize("case", ac.FALLBACK_CASES, ids=lambda c: c["name"])
def test_univariate_fallback_matches_restatement(oracle, case):
    run_loop(oracle, case, fallback=True)


# ---- 3: whole rounds -----------------------------------------------------------------------------------
ROUND_LISTS = [
    ("trend-autoar4", [("trend",), ("autoar", 4, dict(truncate=1))], [], 3101),
    ("autoar2-ar2-seasonal4", [("autoar", 2, dict(truncate=1, sigma_upper_limit=2.0)), ("ar", 2), ("seasonal", 4, 1)],
     [(4, 1)], 3102),
]


@gpu
@pytest.mark.parametrize("name,desc,seas,seed", ROUND_LISTS, ids=[r[0] for r in ROUND_LISTS])
def test_whole_rounds(oracle, name, desc, seas, seed):
    """12 x ba_ss_sweep(1): the block's sampler inside the round against the restatement, from the state
    the device had before the round (its sampler reads nothing of the round's regression draw);
    ba_ss_sweep(12) gives the same bits"""
    T, p, chains, rounds = 48, 3, 4, 12
    X, y, _, _ = general_data(T, p, 2, seas, seed=seed, ar_coef=[0.5, -0.2])
    blocks = ac.autoar_spec(y, desc)
    k = [i for i, b in enumerate(blocks) if b["kind"] == ac.KIND_AUTO_AR][0]
    eng = engine(chains, seed, y, X, None, blocks)
    eng.ss_impute_state()
    check = [0, chains - 1]
    F = {ch: Follower(oracle, blocks, k, seed, ch) for ch in check}
    for r in range(rounds):
        before = {ch: device_state(eng, ch, k) for ch in check}
        eng.ss_sweep(1)
        for ch in check:
            F[ch].check(before[ch], device_state(eng, ch, k), "%s round %d chain %d" % (name, r, ch))
    for ch in check:
        assert F[ch].S.margin > 1e-9
    RATIOS[name] = {q: max(F[ch].worst[q] for ch in check) for q in ("phi", "sigsq")}
    print("worst ratios", name, RATIOS[name])
    one = engine(chains, seed, y, X, None, blocks)
    one.ss_impute_state()
    one.ss_sweep(rounds)
    for u, v in zip(one.get_states(), eng.get_states()):
        assert np.array_equal(u, v)
    for ch in range(chains):
        assert np.array_equal(one.ss_get_state_draw(ch), eng.ss_get_state_draw(ch))
        assert np.array_equal(one.ss_get_ar_inclusion(ch, k), eng.ss_get_ar_inclusion(ch, k))
        for b in range(len(blocks)):
            u, v = one.ss_get_state_model(ch, b), eng.ss_get_state_model(ch, b)
            assert np.array_equal(u["variances"], v["variances"])
            if "phi" in u:
                assert np.array_equal(u["phi"], v["phi"])


@gpu
def test_whole_rounds_beside_a_student_trend(oracle):
    """a list that also holds a Student local linear trend (kind 8, which brings kernels of its own around
    the state kernel): the block's sampler is launched there too, and matches the restatement"""
    import student_trend_cases as stc
    T, p, chains, seed, rounds = 48, 3, 4, 3103, 6
    X, y, _, _ = general_data(T, p, 2, [], seed=seed, ar_coef=[0.5, -0.2])
    blocks = stc.student_trend_spec(y, [("student_trend",), ("ar", 2)])
    blocks[1] = ac.autoar_spec(y, [("trend",), ("autoar", 2, dict(truncate=1))])[1]
    eng = engine(chains, seed, y, X, None, blocks)
    eng.ss_impute_state()
    check = [0, chains - 1]
    F = {ch: Follower(oracle, blocks, 1, seed, ch) for ch in check}
    for r in range(rounds):
        before = {ch: device_state(eng, ch, 1) for ch in check}
        eng.ss_sweep(1)
        for ch in check:
            F[ch].check(before[ch], device_state(eng, ch, 1), "student-trend-autoar2 round %d chain %d" % (r, ch))
    for ch in check:
        assert F[ch].S.margin > 1e-9


# ---- 4: to every structural kernel it is an autoregression -------------------------------------------------
@gpu
def test_equivalent_to_a_plain_autoregression():
    T, p, chains, seed = 50, 3, 4, 91
    X, y, _, obs = general_data(T, p, 2, [], seed=5, ar_coef=[0.4], missing_frac=0.05)
    phi0 = np.array([0.5, 0.0, -0.2, 0.0])
    blocks = ac.autoar_spec(y, [("level",), ("autoar", 4, dict(truncate=1, initial_phi=phi0))])
    gam, beta = ac.chain_parameters(p, chains, 3)
    engs = []
    for bl in (blocks, ac.as_plain_ar(blocks)):
        e = engine(chains, seed, y, X, obs, bl, gam[0])
        for ch in range(chains):
            e.set_state(gam[ch], beta[ch], 0.6, chain=ch)
        e.ss_impute_state()
        engs.append(e)
    a, b = engs
    newX = np.random.Generator(np.random.PCG64(1)).standard_normal((6, p))
    assert np.array_equal(a.ss_forecast(newX), b.ss_forecast(newX))
    ea, eb = a.ss_prediction_errors(variances=True, log_likelihood=True), b.ss_prediction_errors(variances=True, log_likelihood=True)
    for q in ("errors", "variances", "log_likelihood"):
        assert np.array_equal(ea[q], eb[q]), q
    for ch in range(chains):
        assert np.array_equal(a.ss_get_state_draw(ch), b.ss_get_state_draw(ch))
        u, v = a.ss_get_state_model(ch, 1), b.ss_get_state_model(ch, 1)
        for q in ("phi", "variances", "xtx", "xty", "yty", "n"):
            assert np.array_equal(u[q], v[q]), q
        assert np.array_equal(a.ss_get_ar_inclusion(ch, 1), np.ones(4, np.uint8))
    # after draws: the excluded lags are exactly 0.0
    a.ss_sweep(6)
    seen_excluded = False
    for ch in range(chains):
        g, ph = a.ss_get_ar_inclusion(ch, 1), a.ss_get_state_model(ch, 1, suf=False)["phi"]
        assert np.all(ph[g == 0] == 0.0) and np.all(ph[g == 1] != 0.0)
        seen_excluded = seen_excluded or not g.all()
    assert seen_excluded


# ---- 5: the look-ahead ------------------------------------------------------------------------------------
@gpu
def test_lookahead_is_bit_identical_and_takes_the_general_kernel():
    T, p, chains, seed, draws = 48, 3, 4, 57, 20
    X, y, _, _ = general_data(T, p, 2, [], seed=9, ar_coef=[0.5, -0.2])
    # (the shape the template kernel is compiled for, were the block a plain autoregression)
    blocks = ac.autoar_spec(y, [("trend",), ("autoar", 4, dict(truncate=1))])
    rec = []
    for la in (8, 1):
        eng = engine(chains, seed, y, X, None, blocks)
        eng.set_kernel_timing(True)
        eng.ss_set_lookahead(la)
        out = []
        for _ in range(draws):
            eng.ss_draw_next()
            g, b, s = eng.get_states()
            row = [g.copy(), b.copy(), s.copy()]
            for ch in range(chains):
                sm = eng.ss_get_state_model(ch, 1, suf=False)
                row += [sm["phi"].copy(), sm["variances"].copy(), eng.ss_get_ar_inclusion(ch, 1).copy()]
            out.append(row)
        rec.append(out)
        # the classes launched, for both look-aheads: the sampler ahead of EVERY drawing state launch
        # (batches enqueued ahead and the replays that ba_ss_get_ar_inclusion's settling makes included),
        # one state launch more for the first impute_state, and never the persistent round kernel.  The
        # counts cannot tell the shape-specialised kernel from the general one -- both are launched in
        # the "ssm_simsmooth_kernel" class: that is what the run with the general kernel forced, below,
        # is for (the shape-specialised kernel would redraw phi by ArPosteriorSampler on top of the
        # block's sampler, and the bits would differ).
        kt = eng.kernel_times()
        assert kt["ar_spike_kernel"][1] >= draws, kt["ar_spike_kernel"]
        assert kt["ssm_simsmooth_kernel"][1] == kt["ar_spike_kernel"][1] + 1, (kt["ssm_simsmooth_kernel"], kt["ar_spike_kernel"])
        assert kt.get("ss_round_kernel", (0.0, 0))[1] == 0
        if la == 1:
            assert kt["ar_spike_kernel"][1] == draws
    for i, (u, v) in enumerate(zip(*rec)):
        for j, (x, z) in enumerate(zip(u, v)):
            assert np.array_equal(x, z), (i, j)
    # the default tuning runs the general kernel for such a list: the same bits with it forced
    forced = engine(chains, seed, y, X, None, blocks, kernel=0)
    for _ in range(draws):
        forced.ss_sweep(1)
    for x, z in zip(forced.get_states(), eng.get_states()):
        assert np.array_equal(x, z)
    for ch in range(chains):
        assert np.array_equal(forced.ss_get_state_model(ch, 1, suf=False)["phi"], rec[1][-1][3 + 3 * ch])


# ---- 6: the distribution ---------------------------------------------------------------------------------
def exact_model_posterior(xtx, xty, yty, n, mu, P, pi, prior_df, prior_ss, nodes=80, half_width=3.0):
    """p(gamma | the statistics) of the 8 models of L = 3 for MANY chains at once (xtx: C x 3 x 3, xty:
    C x 3, yty, n: C), sigma^2 integrated by quadrature: the joint of (gamma, sigma^2) is the spike x the
    marginal likelihood of the included coefficients' slab (the sampler's log_model_prob) x sigma^-n
    exp(-yty / 2 sigma^2) x the prior of sigma^2 (1 / sigma^2 ~ Gamma(df / 2, ss / 2)).  Gauss-Legendre
    nodes in log sigma^2, +- half_width around every chain's own scale (yty + ss) / (n + df): the
    integrand is a bump of width sqrt(2 / n) ~ 0.2 there, 80 nodes put one every 0.12 at the centre (the
    posteriors agree with 600 nodes over +- 9 to 1e-15)"""
    L = 3
    x, w = np.polynomial.legendre.leggauss(nodes)
    centre = np.log((yty + prior_ss) / (n + prior_df))
    ls = centre[:, None] + half_width * x[None]    # C x G
    s2 = np.exp(ls)
    with np.errstate(divide="ignore"):
        lpi, lcpi = np.log(pi), np.log(1 - pi)
    # (+ ls: d sigma^2 = sigma^2 d log sigma^2)
    base = -(n[:, None] / 2) * ls - yty[:, None] / (2 * s2) - (prior_df / 2 + 1) * ls - prior_ss / (2 * s2) + ls
    logj = np.zeros((8,) + ls.shape)
    for m in range(8):
        g = np.array([(m >> i) & 1 for i in range(L)], bool)
        lp = float(np.sum(np.where(g, lpi, lcpi)))
        if not g.any():
            logj[m] = lp + base
            continue
        Pg, mg = P[np.ix_(g, g)], mu[g]
        Xg, xyg = xtx[:, g][:, :, g], xty[:, g]
        A = Pg[None, None] + Xg[:, None] / s2[:, :, None, None]
        b = (Pg @ mg)[None, None] + xyg[:, None] / s2[:, :, None]
        sol = np.linalg.solve(A, b[..., None])[..., 0]
        logj[m] = lp + .5 * np.linalg.slogdet(Pg)[1] - .5 * mg @ Pg @ mg - .5 * np.linalg.slogdet(A)[1] \
            + .5 * np.sum(b * sol, axis=-1) + base
    top = logj.max(axis=(0, 2), keepdims=True)
    pm = (np.exp(logj - top) * w[None, None]).sum(axis=2)    # 8 x C
    return (pm / pm.sum(axis=0, keepdims=True)).T


@gpu
def test_model_frequencies_match_the_exact_posterior():
    """L = 3, truncate off, 4096 chains, the statistics held fixed by not imputing again: after 50 x
    ba_ss_autoar_draw_parameters the chains' models are draws of p(gamma | their statistics).  Every
    chain has its own statistics (its own state draw), so the count of model k is a sum of independent
    indicators with the chains' exact probabilities: z = (count - sum p) / sqrt(sum p (1 - p)),
    Bonferroni over the 8 models at 1e-3"""
    from scipy.stats import norm
    T, p, chains, seed = 40, 3, 4096, 1234
    X, y, _, _ = general_data(T, p, 2, [], seed=21, ar_coef=[0.6, -0.3])
    mu, P = ac.slab(3, 77)
    pi = np.array([0.5, 0.3, 0.6])
    blocks = ac.autoar_spec(y, [("level",), ("autoar", 3, dict(truncate=0, slab_mean=mu, slab_precision=P,
                                                                 inclusion_probabilities=pi))])
    eng = engine(chains, seed, y, X, None, blocks)
    eng.ss_impute_state()
    for _ in range(50):
        eng.ss_autoar_draw_parameters()
    b = blocks[1]
    pdf, pss = float(b["df"][0]), float(b["df"][0] * b["sigma_guess"][0] ** 2)
    counts = np.zeros(8)
    xtx, xty, yty, n = np.zeros((chains, 3, 3)), np.zeros((chains, 3)), np.zeros(chains), np.zeros(chains)
    for ch in range(chains):
        sm = eng.ss_get_state_model(ch, 1)
        g = eng.ss_get_ar_inclusion(ch, 1)
        counts[int(g[0]) + 2 * int(g[1]) + 4 * int(g[2])] += 1
        xtx[ch], xty[ch], yty[ch], n[ch] = sm["xtx"], sm["xty"], sm["yty"], sm["n"]
    pm = exact_model_posterior(xtx, xty, yty, n, mu, P, pi, pdf, pss)
    expect, var = pm.sum(axis=0), (pm * (1 - pm)).sum(axis=0)
    z = (counts - expect) / np.sqrt(var)
    bound = float(norm.isf(1e-3 / (2 * 8)))
    print("counts", counts, "expected", np.round(expect, 1), "z", np.round(z, 2), "bound %.3f" % bound)
    assert np.abs(z).max() < bound


# ---- 7: the interface ------------------------------------------------------------------------------------
@gpu
def test_refusals_and_their_texts():
    import boom_amd
    T, p = 30, 3
    X, y, _, _ = general_data(T, p, 1, [], seed=2)
    eng = boom_amd.Engine(2, seed=1)
    eng.ss_set_data(y, X, None)

    def spec(L=2, **opt):
        return ac.autoar_spec(y, [("level",), ("autoar", L, opt)])

    spd = "the slab's precision must be symmetric positive definite"
    refused(lambda: eng.ss_set_state_models(spec(slab_precision=np.array([[1.0, 2.0], [2.0, 1.0]]))), spd)
    refused(lambda: eng.ss_set_state_models(spec(slab_precision=np.array([[1.0, 0.5], [0.2, 1.0]]))), spd)
    refused(lambda: eng.ss_set_state_models(spec(slab_precision=np.array([[1.0, 0.0], [0.0, 0.0]]))), spd)
    for bad in ([0.5, 1.5], [-0.1, 0.5], [np.nan, 0.5]):
        refused(lambda: eng.ss_set_state_models(spec(inclusion_probabilities=bad)),
                "prior inclusion probabilities must lie in [0, 1]")
    refused(lambda: eng.ss_set_state_models(spec(truncate=1, initial_phi=np.array([1.2, 0.1]))),
            "the initial autoregression coefficients are not stationary")
    eng.ss_set_state_models(spec(truncate=0, initial_phi=np.array([1.2, 0.1])))   # (not truncating: any start)
    b17 = dict(spec(16)[1], lags=17)
    refused(lambda: eng.ss_set_state_models([spec()[0], b17]), "more than 16 lags")
    five = ac.autoar_spec(y, [("autoar", 1, {}), ("ar", 1), ("autoar", 1, {}), ("ar", 1), ("autoar", 1, {})])
    refused(lambda: eng.ss_set_state_models(five), "more than 4 autoregression state models")
    # the sampler's entry points on a list without such a block
    eng.ss_set_state_models(general_spec(y, [("level",), ("ar", 2)]))
    refused(lambda: eng.ss_autoar_draw_parameters(), "the list of state models holds no spike-and-slab autoregression")
    eng.set_priors(*[bsts_priors(X, y, 2)[0][q] for q in ("b", "ominv", "pi", "df", "sigma_guess")])
    eng.set_state(np.zeros(p, np.uint8))
    eng.ss_sweep(1)
    refused(lambda: eng.ss_get_ar_inclusion(0, 1), "not a spike-and-slab autoregression state model")
    # the other observation families
    text = "the spike-and-slab autoregression is built for the Gaussian observation model only"
    blocks = spec()
    e2 = boom_amd.Engine(2, seed=1)
    e2.ss_student_set_data(y, X, None)
    refused(lambda: e2.ss_set_state_models(blocks), text)
    counts = np.round(np.exp(0.1 * y - np.mean(0.1 * y))).astype(float)
    e4 = boom_amd.Engine(2, seed=1)
    e4.ss_logit_set_data(np.minimum(counts, 3.0), np.full(T, 3.0), X)
    refused(lambda: e4.ss_set_state_models(blocks), text)
    # ... and the list first, the family's data after it
    e3 = boom_amd.Engine(2, seed=1)
    e3.ss_set_data(y, X, None)
    e3.ss_set_state_models(blocks)
    e3.ss_student_set_data(y, X, None)
    e3.sss_set_slab(np.zeros(p), 0.1 * np.eye(p), scales_with_sigsq=True)
    e3.set_spike(np.full(p, 0.5))
    e3.set_sigma_prior(1.0, 1.0)
    e3.set_state(np.zeros(p, np.uint8))
    refused(lambda: e3.ss_student_sweep(1), text)


@gpu
def test_poisson_family_refuses_the_block():
    import boom_amd
    from ss_family_cases import count_series, golden_mix
    T, p = 30, 3
    X, counts, exposure, y = count_series(T, p, 4)
    e = boom_amd.Engine(2, seed=1)
    e.ss_poisson_set_data(counts, exposure, X, golden_mix(), None)
    refused(lambda: e.ss_set_state_models(ac.autoar_spec(y, [("level",), ("autoar", 2, {})])),
            "the spike-and-slab autoregression is built for the Gaussian observation model only")


@gpu
def test_seed_reproduces_a_run():
    """the regression-free loop of the sampler tests, run, reseeded with the chains' state models set up
    anew by ba_ss_set_data, and run again, gives the same bits; another seed gives other draws.  (That
    ba_seed by itself rewinds the block's stream is the next test's.)"""
    c = ac.loop_case(ac.LOOP_CASES[2])

    def run(eng):
        for ch in range(c["chains"]):
            eng.set_state(c["gam"][ch], c["beta"][ch], c["sigsq"], chain=ch)
        eng.ss_impute_state()
        out = []
        for _ in range(4):
            eng.ss_autoar_draw_parameters()
            eng.ss_impute_state()
            for ch in range(c["chains"]):
                sm = eng.ss_get_state_model(ch, c["block"], suf=False)
                out += [sm["phi"].copy(), sm["variances"].copy(), eng.ss_get_ar_inclusion(ch, c["block"]).copy(),
                        eng.ss_get_state_draw(ch).copy()]
        return out

    eng = engine(c["chains"], c["seed"], c["y"], c["X"], c["obs"], c["blocks"], c["gam"][0])
    first = run(eng)
    eng.seed(c["seed"])
    eng.ss_set_data(c["y"], c["X"], c["obs"])
    again = run(eng)
    assert all(np.array_equal(u, v) for u, v in zip(first, again))
    eng.seed(c["seed"] + 1)
    eng.ss_set_data(c["y"], c["X"], c["obs"])
    other = run(eng)
    assert not all(np.array_equal(u, v) for u, v in zip(first, other))


@gpu
def test_seed_alone_rewinds_the_samplers_stream(oracle):
    """ba_seed and nothing else (no new data, so nothing re-initialises the chains): after rounds that
    moved the block's stream on, the next ba_ss_autoar_draw_parameters is the restatement's draw from
    position 0 of the NEW seed's stream, on the state the device then has; the round after it follows on
    from there.  A position that ba_seed left where it was would give other draws"""
    c = ac.loop_case(ac.LOOP_CASES[2])
    eng = loop_engine(c)
    k, new_seed = c["block"], c["seed"] + 40
    eng.ss_impute_state()
    for _ in range(3):
        eng.ss_autoar_draw_parameters()
        eng.ss_impute_state()
    eng.seed(new_seed)
    F = {ch: Follower(oracle, c["blocks"], k, new_seed, ch) for ch in c["check"]}
    for r in range(2):
        before = {ch: device_state(eng, ch, k) for ch in c["check"]}
        eng.ss_autoar_draw_parameters()
        for ch in c["check"]:
            F[ch].check(before[ch], device_state(eng, ch, k), "reseeded round %d chain %d" % (r, ch))
            assert F[ch].rng.pos > 0
    for ch in c["check"]:
        assert F[ch].S.margin > 1e-9


@gpu
def test_pybind_classes_agree_with_the_c_abi():
    """boom.ArStateModel.set_spike_slab_prior in a StateSpaceRegressionModel, served from the façade's
    default look-ahead: five draws == the engine through the C-ABI on the same seed, bit for bit"""
    import boom_amd
    import boom_amd._boom as boom
    assert "ArSpikeSlabSampler" in boom.ArStateModel.set_spike_slab_prior.__doc__
    assert "ArSpikeSlabSampler" in boom.StateSpaceRegressionModel.ar_inclusion.__doc__
    T, p, chains, seed = 40, 3, 3, 29
    X, y, _, _ = general_data(T, p, 2, [], seed=8, ar_coef=[0.5, -0.2])
    blocks = ac.autoar_spec(y, [("level",), ("autoar", 4, dict(truncate=1, max_flips=3, sigma_upper_limit=2.0))])
    prior, _, sig_up = bsts_priors(X, y, 2)
    model = boom.StateSpaceRegressionModel(y, X, chains=chains, seed=seed)
    b = blocks[0]
    level = boom.LocalLevelStateModel(float(b["initial_sigma"][0]))
    level.set_initial_state_mean(float(b["a0"][0]))
    level.set_initial_state_variance(float(b["P0"][0]))
    level.set_prior(b["df"][0], b["sigma_guess"][0], b["sigma_upper_limit"][0])
    model.add_state(level)
    b = blocks[1]
    ar = boom.ArStateModel(4)
    ar.set_sigma(float(b["initial_sigma"][0]))
    ar.set_initial_state_mean(b["a0"])
    ar.set_initial_state_variance(float(b["P0"][0]))
    ar.set_spike_slab_prior(b["slab_mean"], b["slab_precision"], b["inclusion_probabilities"], b["df"][0],
                            b["sigma_guess"][0], b["sigma_upper_limit"][0], truncate=True, max_flips=3)
    model.add_state(ar)
    sampler = boom.StateSpacePosteriorSampler(model, boom.MvnGivenScalarSigma(prior["b"], prior["ominv"]),
                                              boom.ChisqModel(prior["df"], prior["sigma_guess"]),
                                              boom.VariableSelectionPrior(prior["pi"]), sig_up)
    model.set_method(sampler)
    eng = engine(chains, seed, y, X, None, blocks)
    for _ in range(5):
        model.sample_posterior()
        eng.ss_sweep(1)
    for u, v in zip(model.chain_states(), eng.get_states()):
        assert np.array_equal(u, v)
    for ch in range(chains):
        assert np.array_equal(model.ar_inclusion(ch, 0), eng.ss_get_ar_inclusion(ch, 1).astype(bool))
        assert np.array_equal(model.ar_phi(ch, 0), eng.ss_get_state_model(ch, 1, suf=False)["phi"])
        assert model.ar_sigsq(ch, 0) == eng.ss_get_state_model(ch, 1, suf=False)["variances"][0]
