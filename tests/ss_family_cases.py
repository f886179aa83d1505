"""What the tests of the Student-t, Poisson and logit state space families share, and what the tests of
the state models borrow from them: data builders, engines, the whole-round cases with their restatements,
and the data of the signal-recovery tests.  (Not a test module: nothing here is collected.)"""
import ctypes as C

import numpy as np

from cases import bsts_priors, general_data, general_spec
from golden_lib import _golden_mix, load

MAX_COUNT = 26   # (tests/golden/poisson_exposure.npz holds the mixture of every count 1 .. 26)
CLT = 5


def relerr(a, b, floor=1e-3):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def golden_mix():
    return _golden_mix(load("poisson_exposure"))


def student_slab_of(p):
    return np.zeros(p), 0.1 * np.eye(p), np.full(p, min(0.9, 2.5 / p))


def slab_of(p, expected=2.5):
    """the fixed-precision slab of the Poisson and logit families"""
    return np.zeros(p), np.eye(p), np.full(p, min(0.9, expected / p))


def spec(series, desc, upper=np.inf):
    blocks = general_spec(series, desc)
    for b in blocks:
        b["sigma_upper_limit"] = np.full(len(b["sigma_upper_limit"]), float(upper))
    return blocks


def chain_parameters(p, chains, seed):
    rs = np.random.Generator(np.random.PCG64(seed))
    gam = (rs.uniform(size=(chains, p)) < 0.6).astype(np.uint8)
    gam[:, 0] = 1
    return gam, rs.standard_normal((chains, p)) * gam


def state_stream(oracle, seed, chain):
    L = oracle.lib
    L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_rnorm.restype = C.c_double
    rng = oracle.rng_philox(seed, chain, 2, 0)
    return lambda mu, sd: L.bo_rnorm(C.byref(rng), float(mu), float(sd))


# ---- data ----------------------------------------------------------------------------------------
def count_series(T, p, seed, coef=(0.5, -0.4), seasons=0, with_path=False):
    """counts from a known log-rate path (a random walk, X beta, a seasonal pattern), clipped to
    MAX_COUNT; returns X, counts, exposures and log(counts + 1/2), which sizes the state priors
    (with_path: the state's part of the log rate too)"""
    rs = np.random.Generator(np.random.PCG64(seed))
    X = rs.standard_normal((T, p))
    beta = np.zeros(p)
    beta[:len(coef)] = coef
    path = 1.0 + np.cumsum(0.05 * rs.standard_normal(T))
    if seasons:
        pattern = 0.4 * rs.standard_normal(seasons)
        path = path + (pattern - pattern.mean())[np.arange(T) % seasons]
    exposure = rs.uniform(0.5, 2.0, T)
    counts = np.minimum(rs.poisson(exposure * np.exp(path + X @ beta)), MAX_COUNT).astype(float)
    if with_path:
        return X, counts, exposure, np.log(counts + 0.5), path
    return X, counts, exposure, np.log(counts + 0.5)


def binomial_series(T, p, seed, max_trials=1, coef=(0.8, -0.6), seasons=0, with_path=False, fixed_trials=0):
    """successes from a known logit path (a random walk, X beta, a seasonal pattern) at 1 ..
    max_trials trials per step (fixed_trials: that many at every step); returns X, successes,
    trials and the empirical logit log((y + 1/2) / (n - y + 1/2)), which sizes the state priors
    (with_path: the state's part of the logit too)"""
    rs = np.random.Generator(np.random.PCG64(seed))
    X = rs.standard_normal((T, p))
    beta = np.zeros(p)
    beta[:len(coef)] = coef
    path = -0.3 + np.cumsum(0.05 * rs.standard_normal(T))
    if seasons:
        pattern = 0.4 * rs.standard_normal(seasons)
        path = path + (pattern - pattern.mean())[np.arange(T) % seasons]
    trials = (np.full(T, fixed_trials) if fixed_trials else rs.integers(1, max_trials + 1, T)).astype(float)
    successes = rs.binomial(trials.astype(int), 1 / (1 + np.exp(-(path + X @ beta)))).astype(float)
    series = np.log((successes + 0.5) / (trials - successes + 0.5))
    if with_path:
        return X, successes, trials, series, path
    return X, successes, trials, series


# ---- engines -------------------------------------------------------------------------------------
def gaussian_engine(chains, seed, y, X, obs, blocks, g0):
    import boom_amd
    prior, _, sig_up = bsts_priors(X, y, 2)
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_set_data(y, X, obs)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"],
                   sigma_upper_limit=sig_up)
    eng.ss_set_state_models(blocks)
    eng.ss_set_tuning(kernel=0)   # the general kernel: the one the H_t instances are instances of
    eng.set_state(g0)
    return eng


def student_engine(chains, seed, y, X, obs, blocks, g0, nu_prior=(0, 0.1, 100.0), sigma_prior=(1.0, 1.0),
                   sigma_max=np.inf):
    import boom_amd
    p = X.shape[1]
    mu, prec, pi = student_slab_of(p)
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_student_set_data(y, X, obs)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=True)
    eng.set_spike(pi)
    eng.set_sigma_prior(sigma_prior[0], sigma_prior[1], sigma_max)
    eng.student_set_nu_prior(*nu_prior)
    eng.ss_set_state_models(blocks)
    eng.set_state(g0)
    return eng


def poisson_engine(chains, seed, counts, exposure, X, obs, blocks, g0, pi=None, max_flips=-1):
    import boom_amd
    p = X.shape[1]
    mu, prec, pi0 = slab_of(p)
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_poisson_set_data(counts, exposure, X, golden_mix(), obs)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=False, max_flips=max_flips)
    eng.set_spike(pi0 if pi is None else pi)
    eng.ss_set_state_models(blocks)
    eng.set_state(g0)
    return eng


def logit_engine(chains, seed, successes, trials, X, obs, blocks, g0, pi=None, max_flips=-1, clt=5):
    import boom_amd
    p = X.shape[1]
    mu, prec, pi0 = slab_of(p)
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_logit_set_data(successes, trials, X, obs, clt_threshold=clt)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=False, max_flips=max_flips)
    eng.set_spike(pi0 if pi is None else pi)
    eng.ss_set_state_models(blocks)
    eng.set_state(g0)
    return eng


# ---- whole rounds --------------------------------------------------------------------------------
ROUND_CASES = dict(
    student=[
        # blocks, missing steps, sigma upper limit, nu prior
        ([("trend",), ("seasonal", 4, 1)], [], 1.5, (1, 2.0, 0.1)),
        ([("level",)], [5, 23], np.inf, (0, 0.1, 100.0)),
    ],
    poisson=[
        # blocks, T, rounds, missing steps, the state models' sigma upper limit, slot limit, seed
        ([("level",)], 40, 12, [], np.inf, 0, 57),
        ([("trend",), ("seasonal", 4, 1)], 40, 12, [5, 23], np.inf, 0, 58),
        ([("trend",)], 40, 12, [], 0.2, 0, 59),
        ([("level",)], 300, 3, [], np.inf, 0, 60),     # two workgroups of the imputation, five blocks of 64 steps
        ([("level",)], 40, 12, [7], np.inf, 2, 61),    # a slot serves 2 uniforms: the imputation reads its spill streams
    ],
    logit=[
        # blocks, T, rounds, largest number of trials, missing steps, slot limit, seed
        ([("level",)], 40, 12, 1, [], 0, 57),                               # Bernoulli
        ([("trend",), ("seasonal", 4, 1)], 40, 12, 4, [5, 23], 0, 58),
        ([("level",)], 40, 12, 40, [], 0, 59),     # both branches in one series (clt_threshold 5); n min(p, q) <= 20: no BTPE
        ([("level",)], 300, 3, 4, [], 0, 60),      # two workgroups of the imputation, five blocks of 64 steps
        ([("level",)], 40, 12, 4, [7], 2, 61),     # a slot serves 2 uniforms: the imputation reads its spill streams
    ],
)


def round_case(family, k):
    """case k of the family: its data, its engine (`engine()`) and its restatement (`oracle(o, chain)`)"""
    return dict(student=_student_round_case, poisson=_poisson_round_case, logit=_logit_round_case)[family](k)


def _latent_round_case(desc, T, rounds, miss, upper, slots, seed, data):
    """what a Poisson and a logit case share; data: (X, the family's two series, the series that sizes the priors)"""
    p, chains = 5, 4
    obs = np.ones(T, np.uint8)
    obs[miss] = 0
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    return dict(T=T, p=p, chains=chains, seed=seed, rounds=rounds, X=data[0], obs=obs, blocks=spec(data[3], desc, upper),
                g0=g0, slots=slots, check=[0, chains - 1], slab=slab_of(p))


def _seasons(desc):
    return max([b[1] for b in desc if b[0] == "seasonal"], default=0)


def _poisson_round_case(k):
    import ss_poisson_oracle as spo
    desc, T, rounds, miss, upper, slots, seed = ROUND_CASES["poisson"][k]
    X, counts, exposure, _ = data = count_series(T, 5, 31 + k, seasons=_seasons(desc))
    c = _latent_round_case(desc, T, rounds, miss, upper, slots, seed, data)
    obs, blocks, g0, (mu, prec, pi) = c["obs"], c["blocks"], c["g0"], c["slab"]
    c.update(counts=counts, exposure=exposure,
             oracle=lambda o, chain: spo.SsPoissonOracle(o, counts, exposure, X, obs, blocks, golden_mix(), mu, prec, pi,
                                                         seed, chain, g0),
             engine=lambda: poisson_engine(c["chains"], seed, counts, exposure, X, obs, blocks, g0))
    return c


def _logit_round_case(k):
    import ss_logit_oracle as slo
    desc, T, rounds, max_trials, miss, slots, seed = ROUND_CASES["logit"][k]
    X, successes, trials, _ = data = binomial_series(T, 5, 31 + k, max_trials=max_trials, seasons=_seasons(desc))
    c = _latent_round_case(desc, T, rounds, miss, np.inf, slots, seed, data)
    obs, blocks, g0, (mu, prec, pi) = c["obs"], c["blocks"], c["g0"], c["slab"]
    c.update(successes=successes, trials=trials,
             oracle=lambda o, chain: slo.SsLogitOracle(o, successes, trials, X, obs, blocks, mu, prec, pi, seed, chain, g0,
                                                       clt_threshold=CLT),
             engine=lambda: logit_engine(c["chains"], seed, successes, trials, X, obs, blocks, g0, clt=CLT))
    return c


def _student_round_case(k):
    import ss_student_oracle as sso
    desc, miss, smax, nup = ROUND_CASES["student"][k]
    T, p, chains, seed, rounds = 40, 5, 4, 57 + k, 12
    seas = [(b[1], b[2]) for b in desc if b[0] == "seasonal"]
    X, y, _, _ = general_data(T, p, 2, seas, seed=31 + k)
    rs = np.random.Generator(np.random.PCG64(9 + k))
    y = y + np.where(rs.uniform(size=T) < 0.1, 6.0 * rs.standard_normal(T), 0.0)   # a few outliers
    obs = np.ones(T, np.uint8)
    obs[miss] = 0
    blocks = general_spec(y, desc)
    g0 = np.zeros(p, np.uint8)
    g0[0] = 1
    mu, prec, pi = student_slab_of(p)

    def make_oracle(o, chain):
        return sso.SsStudentOracle(o, y, X, obs, blocks, mu, prec, pi, seed, chain, g0, nu_prior=nup,
                                   sigma_max=smax)
    return dict(T=T, p=p, chains=chains, seed=seed, rounds=rounds, X=X, y=y, obs=obs, blocks=blocks, g0=g0,
                smax=smax, nup=nup, check=[0, chains - 1], oracle=make_oracle,
                engine=lambda: student_engine(chains, seed, y, X, obs, blocks, g0, nu_prior=nup, sigma_max=smax))


# ---- signal recovery -----------------------------------------------------------------------------
RECOVERY_SHAPE, RECOVERY_TRIALS, RECOVERY_SEED, RECOVERY_COEF = (200, 6), 20, 11, (0.5, -0.5)


def recovery_data(family, with_path=False):
    """a series whose rate (success probability, at RECOVERY_TRIALS trials a step) depends on 2 of 6 predictors"""
    T, p = RECOVERY_SHAPE
    if family == "poisson":
        return count_series(T, p, RECOVERY_SEED, coef=RECOVERY_COEF, with_path=with_path)
    return binomial_series(T, p, RECOVERY_SEED, coef=RECOVERY_COEF, fixed_trials=RECOVERY_TRIALS, with_path=with_path)
