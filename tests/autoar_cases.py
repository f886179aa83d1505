"""Cases of the spike-and-slab autoregression state model (kind 9, bsts AddAutoAr), shared by
tests/test_ss_autoar_cpu.py and tests/test_ss_autoar_gpu.py."""
import numpy as np

from cases import general_data, general_spec

KIND_AUTO_AR = 9


def slab(L, seed, diagonal=False):
    """(mean, precision) of a slab: a well conditioned precision, non-diagonal unless asked"""
    rs = np.random.Generator(np.random.PCG64(seed))
    if diagonal:
        return np.zeros(L), np.diag(1.0 + rs.uniform(size=L))
    A = rs.standard_normal((L, L + 2))
    P = A @ A.T / (L + 2) + np.eye(L)
    return 0.05 * rs.standard_normal(L), (P + P.T) / 2


def autoar_spec(y, desc):
    """general_spec with ("autoar", lags, options) entries: the block as general_spec makes an ("ar",
    lags), with kind 9 and the options -- slab_mean, slab_precision, inclusion_probabilities, truncate,
    max_flips, allow_model_selection, initial_phi, sigma_upper_limit (None: general_spec's), df"""
    where = [i for i, b in enumerate(desc) if b[0] == "autoar"]
    blocks = general_spec(y, [("ar", b[1]) if b[0] == "autoar" else b for b in desc])
    for i in where:
        L, opt = desc[i][1], dict(desc[i][2])
        mu, P = slab(L, 100 + L)
        b = dict(blocks[i], kind=KIND_AUTO_AR, slab_mean=opt.pop("slab_mean", mu),
                 slab_precision=opt.pop("slab_precision", P),
                 inclusion_probabilities=np.asarray(opt.pop("inclusion_probabilities", np.full(L, 0.5)), float),
                 truncate=int(opt.pop("truncate", 1)), max_flips=int(opt.pop("max_flips", -1)),
                 allow_model_selection=int(opt.pop("allow_model_selection", 1)),
                 initial_phi=np.asarray(opt.pop("initial_phi", np.zeros(L)), float))
        up = opt.pop("sigma_upper_limit", None)
        if up is not None:
            b["sigma_upper_limit"] = np.array([float(up)])
        # (bsts's 0.01 prior degrees of freedom give a first draw -- before any state draw -- of no
        # use as a scale: the cases take a prior that says something)
        b["df"] = np.array([float(opt.pop("df", 3.0))])
        b["sigma_guess"] = np.array([float(opt.pop("sigma_guess", 0.5))])
        assert not opt, opt
        blocks[i] = b
    return blocks


def as_plain_ar(blocks):
    out = []
    for b in blocks:
        if b["kind"] == KIND_AUTO_AR:
            b = dict(b, kind=4)
        out.append(b)
    return out


def chain_parameters(p, chains, seed):
    rs = np.random.Generator(np.random.PCG64(seed))
    gam = (rs.uniform(size=(chains, p)) < 0.6).astype(np.uint8)
    gam[:, 0] = 1
    return gam, rs.standard_normal((chains, p)) * gam


# ---- the sampler alone: ba_ss_impute_state, then 12 x (ba_ss_autoar_draw_parameters; ba_ss_impute_state)
# with gamma, beta, sigma^2 of the regression fixed.  [local level, AutoAr(L)], T = 48, p = 3, 4 chains.
def _pi01(L):
    pi = np.full(L, 0.5)
    pi[0] = 1.0
    pi[-1] = 0.0
    return pi


LOOP_ROUNDS, LOOP_T, LOOP_P, LOOP_CHAINS, LOOP_SIGSQ = 12, 48, 3, 4, 0.5
LOOP_CHECK = [0, LOOP_CHAINS - 1]
LOOP_CASES = [
    dict(name="L1", lags=1, seed=2301, data_seed=71, opt=dict(truncate=1)),
    dict(name="L2-free-upper", lags=2, seed=2302, data_seed=72, opt=dict(truncate=0, sigma_upper_limit=1.5)),
    dict(name="L4-flips2-pi01", lags=4, seed=2303, data_seed=73,
         opt=dict(truncate=1, max_flips=2, inclusion_probabilities=_pi01(4))),
    dict(name="L4-noselect-missing", lags=4, seed=2304, data_seed=74, opt=dict(truncate=1, allow_model_selection=0),
         missing=[7]),
    dict(name="L16", lags=16, seed=2305, data_seed=75, opt=dict(truncate=1, inclusion_probabilities=np.full(16, 0.3))),
    dict(name="L16-free-pi01", lags=16, seed=2306, data_seed=76, opt=dict(truncate=0, inclusion_probabilities=_pi01(16))),
]
# the fallback: a near-unit-root series and a tight slab centred (just) outside the stationary region --
# sd 0.002 a coefficient, phi_1 + phi_2 = 1.016 +- 0.0028 -- so that all 100 multivariate proposals fail
# and the reference goes through draw_phi_univariate: phi_1 given the initial phi_2 = -0.5 is accepted at
# once, phi_2 given phi_1 ~ 0.9 has to come down 8 standard deviations to 0.1 and narrows its interval some
# 30 times (N standard deviations cost about N^2 / 2 truncated draws: a slab further out would run
# into the reference's 1000 attempts).  L = 1 takes the only-one-included `continue`.
FALLBACK_CASES = [
    dict(name="fallback-L2", lags=2, seed=2311, data_seed=81, rounds=3,
         opt=dict(truncate=1, allow_model_selection=0, slab_mean=np.array([0.9, 0.116]),
                  slab_precision=np.array([[2.5e5, 1e3], [1e3, 2.5e5]]), initial_phi=np.array([0.0, -0.5])),
         ar_coef=[0.99]),
    dict(name="fallback-L1", lags=1, seed=2312, data_seed=82, rounds=3,
         opt=dict(truncate=1, slab_mean=np.array([1.05]), slab_precision=np.array([[2.5e5]]),
                  inclusion_probabilities=np.array([1.0]), initial_phi=np.array([0.5])),
         ar_coef=[0.99]),
]


def loop_case(c):
    T, p = LOOP_T, LOOP_P
    X, y, _, _ = general_data(T, p, 2, [], seed=c["data_seed"], ar_coef=c.get("ar_coef", [0.6, -0.2]))
    obs = None
    if c.get("missing"):
        obs = np.ones(T, np.uint8)
        obs[c["missing"]] = 0
    blocks = autoar_spec(y, [("level",), ("autoar", c["lags"], c["opt"])])
    gam, beta = chain_parameters(p, LOOP_CHAINS, c["data_seed"] + 7)
    return dict(c, T=T, p=p, X=X, y=y, obs=obs, blocks=blocks, gam=gam, beta=beta, sigsq=LOOP_SIGSQ,
                chains=LOOP_CHAINS, check=LOOP_CHECK, rounds=c.get("rounds", LOOP_ROUNDS), block=1)


def sampler_of(o, b, dtype=np.float64):
    """the restatement's sampler of a kind-9 block dict"""
    import ss_autoar_oracle as sao
    return sao.AutoArSampler(o, b["lags"], b["slab_mean"], b["slab_precision"], b["inclusion_probabilities"],
                             float(b["df"][0]), float(b["sigma_guess"][0]), float(b["sigma_upper_limit"][0]),
                             bool(b["truncate"]), int(b["max_flips"]), bool(b["allow_model_selection"]), dtype=dtype)


def random_suf(L, seed, n=60):
    """ArSuf-like statistics of a random stationary series"""
    rs = np.random.Generator(np.random.PCG64(seed))
    u = np.zeros(n + L + 20)
    e = rs.standard_normal(len(u))
    for t in range(1, len(u)):
        u[t] = 0.5 * u[t - 1] + e[t]
    u = u[20:]
    Xl = np.stack([u[L - 1 - i:len(u) - 1 - i] for i in range(L)], axis=1)
    yv = u[L:]
    return dict(xtx=Xl.T @ Xl, xty=Xl.T @ yv, yty=float(yv @ yv), n=float(len(yv)))
