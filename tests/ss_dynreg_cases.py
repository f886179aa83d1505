"""The lists, predictors and data of the dynamic regression tests (tests/test_ss_dynreg_cpu.py,
tests/test_ss_dynreg_gpu.py).  T = 70 crosses one edge of the kernel's 64-step time blocks, T = 130 two
(63 | 64 and 127 | 128): every list below keeps bl = 64, so the predictor rows cross them too."""
import numpy as np

import ss_dynreg_oracle as sdo
from cases import general_data, general_spec, kernel_instance

P = 3            # regression coefficients
HORIZON = 10


def predictors(rows, d, seed, hard=None):
    """rows x d predictors of mixed signs (rounded to 1/64: their products with the doubling identity's
    powers of two are exact).  hard = T: test (b)'s rows -- column 1 is 0 over [0, 5) and [T - 6, T), a
    stretch that holds t = 0 and one that holds T - 1; row 9 is all zero; row 63 too where it exists
    (the last step of the first time block)"""
    rs = np.random.Generator(np.random.PCG64(seed))
    x = np.round(rs.standard_normal((rows, d)) * 64) / 64
    x[:, 0] += 1.0
    if hard is not None:
        T = int(hard)
        if d > 1:
            x[:5, 1] = 0.0
            x[T - 6:T, 1] = 0.0
        x[9, :] = 0.0
        if T > 64:
            x[63, :] = 0.0
    return x


MISSING = (12, 64)   # (64: the first step of the second time block)


def data(T, seasonal=((4, 1),), seed=5, missing=MISSING, trig=None, p=P):
    X, y, _, _ = general_data(T, p, 2, list(seasonal), seed=seed + T, trig=trig)
    obs = np.ones(T, np.uint8)
    obs[[t for t in missing if t < T]] = 0
    return X, y, obs


def sdy_of(y):
    return float(np.std(y, ddof=1))


def list_small(y, T):
    """SMALL: level + 4 seasons + dynamic regression d = 3 (first = 4), m = 7"""
    return general_spec(y, [("level",), ("seasonal", 4, 1)]) + [
        sdo.dynreg_block(predictors(T + HORIZON, 3, 31, hard=T), sdy_of(y), [0.3, 0.0, 0.5])]


def list_edge(y, T):
    """SMALL at its edge: d = 16 alone, m = 16, all 16 variance slots"""
    return [sdo.dynreg_block(predictors(T + HORIZON, 16, 32, hard=T) * 0.25, sdy_of(y), np.linspace(0.1, 0.4, 16))]


def list_ldc33(y, T):
    """LDC 33: 20 seasons + dynamic regression d = 3, m = 22"""
    return general_spec(y, [("seasonal", 20, 1)]) + [sdo.dynreg_block(predictors(T + HORIZON, 3, 33, hard=T), sdy_of(y))]


def list_glob(y, T):
    """GLOB: a trig block + dynamic regression d = 3"""
    return general_spec(y, [("trig", 12.0, [1.0, 2.0])]) + [
        sdo.dynreg_block(predictors(T + HORIZON, 3, 34, hard=T), sdy_of(y))]


def list_two(y, T):
    """two dynamic blocks in one list, d = 3 and 2, a level between them (column offsets 0 and 3)"""
    s = sdy_of(y)
    return [sdo.dynreg_block(predictors(T + HORIZON, 3, 35, hard=T), s)] + general_spec(y, [("level",)]) + [
        sdo.dynreg_block(predictors(T + HORIZON, 2, 36, hard=T), s, [0.2, 0.4])]


def list_instance(y, T, seasons, glob):
    """[a one-frequency trig block: GLOB +] a duration-1 seasonal that pads the state to the leading dimension
    wanted (18, 34, 61 seasons: 33, 61, 65) + dynamic regression d = 2: the kernel instances the lists above
    do not reach"""
    pad = ([("trig", 12.0, [1.0])] if glob else []) + [("seasonal", seasons, 1)]
    return general_spec(y, pad) + [sdo.dynreg_block(predictors(T + HORIZON, 2, 40, hard=T), sdy_of(y), [0.3, 0.5])]


def instance_case(seasons, glob):
    """(T, make, data arguments) of test_impute_state_matches_restatement: two time blocks and three steps"""
    T = 2 * kernel_instance(list_instance(np.arange(8.0), 8, seasons, glob))[2] + 3
    return T, lambda y, T: list_instance(y, T, seasons, glob), dict(seasonal=(), missing=(5, T - 2), p=2)


def chain_parameters(chains, seed, p=P):
    """every chain its own regression parameters"""
    rs = np.random.Generator(np.random.PCG64(seed))
    gam = (rs.uniform(size=(chains, p)) < 0.6).astype(np.uint8)
    gam[:, 0] = 1
    return gam, rs.standard_normal((chains, p)) * gam




# ---- the whole-rounds loop of the GPU test: level + 4 seasons + d = 3, T = 70
LOOP = dict(T=70, chains=4, seed=913, rounds=12, sig0=0.7, check=(0, 3))


def loop_case():
    c = dict(LOOP)
    c["X"], c["y"], c["obs"] = data(c["T"])
    s = sdy_of(c["y"])
    c["blocks"] = general_spec(c["y"], [("level",), ("seasonal", 4, 1)]) + [
        sdo.dynreg_block(predictors(c["T"] + HORIZON, 3, 37, hard=c["T"]), s, [0.3, 0.2, 0.5])]
    c["g0"] = np.zeros(P, np.uint8)
    c["g0"][0] = 1
    c["b0"] = np.zeros(P)
    return c
