"""The cases of tests/test_mlogit_gpu.py and the helpers they share with tests/test_mlogit_cpu.py
(which checks every parity case's margins on the CPU, where the seeds were chosen).  Not a test.

A case is a dict: y, Xs (n x psub or None), Xc ((n M) x pch or None), M, D, the slab (mu, prec),
the spike pi, the start g0, chains, seed, the engine's chain_offset, the restated chains, the
flip order (None: identity), max_flips, nsweeps, slot_limit.
Unless a case says otherwise coefficient 0 (choice 1's intercept) is forced in (pi = 1): with
the reference's sign of the empty model's value (log prior + wss / 2, MLVS.cpp:166-168) the empty
model, once reached, is never left, and a chain without a forced variable soon sits there.
"""
import numpy as np

from mlogit_oracle import MlogitOracle

RTOL_BETA, ATOL_U, RTOL_WSS = 1e-8, 1e-9, 1e-9
MIN_FLIP_MARGIN, MIN_UNMIX_MARGIN = 1e-8, 1e-9


def relerr(a, b, floor=1e-3):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def make_case(n, M, psub, pch, seed, chains=3, which=None, y=None, pi_rest=0.4, nsweeps=5, **kw):
    rng = np.random.default_rng(1000 + seed)
    Xs = None
    if psub:
        Xs = rng.standard_normal((n, psub))
        Xs[:, 0] = 1.0
    Xc = rng.standard_normal((n * M, pch)) if pch else None
    D = (M - 1) * psub + pch
    truth = np.where(rng.random(D) < 0.5, rng.choice([-1.5, -0.7, 0.8, 1.2], D), 0.0)
    if y is None:
        from mlogit_oracle import expand_design
        eta = (expand_design(Xs, Xc, n, M) @ truth).reshape(n, M)
        pr = np.exp(eta - eta.max(axis=1, keepdims=True))
        pr /= pr.sum(axis=1, keepdims=True)
        y = np.array([rng.choice(M, p=pr[i]) for i in range(n)])
    pi = np.full(D, pi_rest)
    pi[0] = 1.0
    g0 = np.zeros(D, np.uint8)
    g0[:min(D, 2)] = 1
    case = dict(y=np.asarray(y), Xs=Xs, Xc=Xc, M=M, D=D, mu=np.zeros(D), prec=0.5 * np.eye(D), pi=pi, g0=g0,
                chains=chains, seed=seed, chain_offset=0, which=which or (0, 1, chains - 1), order=None,
                max_flips=-1, nsweeps=nsweeps, slot_limit=0)
    case.update(kw)
    return case


def make_engine(case):
    import boom_amd
    kw = dict(chain_offset=case["chain_offset"]) if case.get("chain_offset") else {}
    eng = boom_amd.Engine(case["chains"], seed=case["seed"], **kw)
    eng.mlogit_set_data(case["y"], case["Xs"], case["Xc"], case["M"])
    if case.get("order") is not None:
        eng.mlogit_set_flip_order(case["order"])
    eng.sss_set_slab(case["mu"], case["prec"], scales_with_sigsq=False, max_flips=case.get("max_flips", -1))
    eng.set_spike(case["pi"])
    eng.set_state(case["g0"], case.get("beta0"))
    return eng


def make_oracles(o, case, rules="mlvs"):
    """local chain -> its restatement"""
    return {c: MlogitOracle(o, case["y"], case["Xs"], case["Xc"], case["M"], case["mu"], case["prec"], case["pi"],
                            case["seed"], case.get("chain_offset", 0) + c, case["g0"], beta0=case.get("beta0"),
                            flip_order=case.get("order"), max_flips=case.get("max_flips", -1), rules=rules)
            for c in sorted(set(case["which"]))}


def margins_ok(ora):
    return all(min(o.flip_margin) > MIN_FLIP_MARGIN and min(o.unmix_margin) > MIN_UNMIX_MARGIN for o in ora.values())


def check_parity(eng, ora, nsweeps, each=None):
    """nsweeps single sweeps of the engine against the restatements at the file's bars"""
    for s in range(nsweeps):
        eng.mlogit_sweep(1)
        gam, beta, sig = eng.get_states()
        assert np.all(sig == 1.0)
        if each is not None:
            each(s, gam, beta)
        for c, o in ora.items():
            g, b = o.draw()
            assert o.flip_margin[-1] > MIN_FLIP_MARGIN and o.unmix_margin[-1] > MIN_UNMIX_MARGIN, \
                (c, s, o.flip_margin[-1], o.unmix_margin[-1])
            u, w = eng.mlogit_get_latent(c)
            assert np.array_equal(w, o.w), (c, s)                      # the mixture components
            assert float(np.max(np.abs(u - o.u))) < ATOL_U, (c, s)
            assert abs(eng.mlogit_get_wss(c) - o.wss) <= RTOL_WSS * o.wss, (c, s)
            assert np.array_equal(gam[c], g), (c, s)
            assert relerr(beta[c], b) < RTOL_BETA, (c, s)


def _grid():
    """n in {37, 256, 257} (the impute block's edges) x M in {2, 3, 7} x (psub, pch) in
    {(1, 0), (5, 0), (3, 2)}, the third rotating over the first two"""
    out = {}
    ns, Ms, pps = (37, 256, 257), (2, 3, 7), ((1, 0), (5, 0), (3, 2))
    for a, n in enumerate(ns):
        for b, M in enumerate(Ms):
            psub, pch = pps[(a + b) % 3]
            out["n%d_M%d_p%d_%d" % (n, M, psub, pch)] = (
                lambda n=n, M=M, psub=psub, pch=pch, a=a, b=b: make_case(n, M, psub, pch, seed=10 * a + b + 1))
    return out


def _wide():
    """D = 520 (M = 5, psub = 130): three chunks of the compaction of included coefficients, the
    included ones in all three (0, 256 and 519 are forced in), at most 8 of them"""
    n, M, psub = 48, 5, 130
    case = make_case(n, M, psub, 0, seed=52, chains=2, which=(0, 1), pi_rest=0.001)
    idx = [0, 255, 256, 511, 512, 519]
    case["pi"][idx] = 0.9
    case["pi"][[0, 256, 519]] = 1.0
    case["g0"][:] = 0
    case["g0"][idx] = 1

    def each(s, gam, beta):
        for c in range(2):
            inc = np.flatnonzero(gam[c])
            assert inc.size <= 8 and inc.min() < 256 and inc.max() >= 512 and np.any((inc >= 256) & (inc < 512)), (c, s, inc)
    case["each"] = each
    return case


def _order_case():
    case = make_case(64, 3, 4, 1, seed=77, chains=3, pi_rest=0.5, nsweeps=5)
    rng = np.random.default_rng(5)
    case["order"] = rng.permutation(case["D"]).astype(np.int32)
    case["max_flips"] = 3
    case["g0"][:] = 1
    return case


def _empty_case():
    """no forced variable and a sparse prior: the chains reach the empty model within the sweeps"""
    case = make_case(60, 3, 2, 0, seed=91, chains=3, pi_rest=0.2, nsweeps=4)
    case["pi"][:] = 0.2
    return case


PARITY = dict(_grid())
PARITY.update({
    "M16": lambda: make_case(37, 16, 2, 1, seed=16, pi_rest=0.3),
    "D520": _wide,
    "chains1024": lambda: make_case(37, 3, 2, 0, seed=24, chains=1024, which=(0, 511, 1023)),
    "chain_offset": lambda: make_case(70, 3, 3, 2, seed=31, chains=2, which=(0, 1), chain_offset=5),
    "y_never_0": lambda: make_case(80, 3, 3, 2, seed=41, y=1 + np.random.default_rng(41).integers(0, 2, 80)),
    "y_constant": lambda: make_case(80, 3, 3, 2, seed=43, y=np.full(80, 2)),
    "spill": lambda: make_case(90, 3, 3, 2, seed=47, slot_limit=4),   # (below 2 M = 6; the engine takes even limits)
    "maxflips3": _order_case,
    "empty": _empty_case,
})

# ---- the distributional case: M = 3, intercepts only (D = 2), n = 200, selection off -----------
# The mixture approximation's own bias: the gap between the posterior means of a 40 000-draw run
# of the restatement (after 500) and the quadrature, per coordinate, measured once with
#   python tests/mlogit_cases.py bias
# which printed: bias [0.010119748738888434, 0.013777375603295616]
# (that run's own Monte-Carlo standard errors, from 100 batch means, are 0.0064 and 0.0077: the
# gap is the mixture's bias and that noise together)
MIXTURE_BIAS = np.array([0.0102, 0.0138])


def intercept_case():
    rng = np.random.default_rng(200)
    n, M = 200, 3
    y = rng.choice(M, n, p=[0.5, 0.3, 0.2])
    return dict(y=y, Xs=np.ones((n, 1)), Xc=None, M=M, D=2, mu=np.zeros(2), prec=0.25 * np.eye(2), pi=np.ones(2),
                g0=np.ones(2, np.uint8), chains=1, seed=200, chain_offset=0, which=(0,), order=None, max_flips=-1)


def intercept_quadrature(case):
    """posterior means of (beta_1, beta_2): density proportional to
    exp(n_1 b_1 + n_2 b_2 - n log(1 + e^b1 + e^b2) - b' P b / 2), trapezoid rule on a grid"""
    cnt = np.bincount(case["y"], minlength=3).astype(float)
    n = cnt.sum()
    g = np.linspace(-3.5, 2.5, 1201)
    b1, b2 = np.meshgrid(g, g, indexing="ij")
    P = case["prec"]
    lp = (cnt[1] * b1 + cnt[2] * b2 - n * np.log1p(np.exp(b1) + np.exp(b2))
          - 0.5 * (P[0, 0] * b1 * b1 + 2 * P[0, 1] * b1 * b2 + P[1, 1] * b2 * b2))
    d = np.exp(lp - lp.max())
    wts = np.ones_like(g)
    wts[0] = wts[-1] = 0.5
    d = d * wts[:, None] * wts[None, :]
    return np.array([float((d * b1).sum() / d.sum()), float((d * b2).sum() / d.sum())])


def restatement_run(case, burn, keep, seed):
    o = MlogitOracle(None, case["y"], case["Xs"], case["Xc"], case["M"], case["mu"], case["prec"], case["pi"], 0, 0,
                     case["g0"], select=False, rng=np.random.default_rng(seed))
    for _ in range(burn):
        o.draw()
    return np.array([o.draw()[1] for _ in range(keep)])


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["bias"]:
        c = intercept_case()
        d = restatement_run(c, 500, 40000, 40000)
        print("bias", np.abs(d.mean(axis=0) - intercept_quadrature(c)).tolist())
