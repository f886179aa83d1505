"""The lists, predictors and data of the AR dynamic regression's tests (tests/test_ss_dynreg_ar_cpu.py,
tests/test_ss_dynreg_ar_gpu.py).  The data and the predictors' hard rows are tests/ss_dynreg_cases.py's: T = 70
crosses one edge of the kernel's 64-step time blocks and T = 130 two; the LDC 33 list below runs 32 steps a
block (its four autoregression slots and four predictor columns take the room), so its edges are 31 | 32,
63 | 64 ... and the all-zero row 63 still ends a block, the missing step 64 still starts one."""
import numpy as np

import ss_dynreg_ar_oracle as sda
import ss_dynreg_cases as sdc
import ss_dynreg_oracle as sdo
from cases import general_spec

P, HORIZON = sdc.P, sdc.HORIZON

PHI2 = np.array([[0.5, -0.2], [0.3, 0.2], [-0.4, 0.1], [0.6, 0.25]])
PHI3 = np.array([[0.5, -0.2, 0.1], [0.3, 0.2, 0.0], [-0.4, 0.1, 0.2], [0.2, 0.25, -0.3]])


def list_small(y, T):
    """SMALL: level + 4 seasons + xdim = 2, lags = 2 (first = 4), m = 8"""
    return general_spec(y, [("level",), ("seasonal", 4, 1)]) + sda.dynreg_ar_blocks(
        sdc.predictors(T + HORIZON, 2, 61, hard=T), 2, sdc.sdy_of(y), [0.3, 0.5], PHI2[:2])


def list_plain_ahead(y, T):
    """a plain dynamic regression d = 2 ahead of the model: its first column is 2; xdim = 3, lags = 1; m = 6"""
    s = sdc.sdy_of(y)
    return [sdo.dynreg_block(sdc.predictors(T + HORIZON, 2, 62, hard=T), s, [0.2, 0.4])] + general_spec(y, [("level",)]) + \
        sda.dynreg_ar_blocks(sdc.predictors(T + HORIZON, 3, 63, hard=T), 1, s, [0.3, 0.2, 0.5], [[0.6], [-0.3], [0.0]])


def list_ldc33(y, T):
    """LDC 33: 20 seasons + xdim = 4, lags = 3, m = 31: every autoregression slot"""
    return general_spec(y, [("seasonal", 20, 1)]) + sda.dynreg_ar_blocks(
        sdc.predictors(T + HORIZON, 4, 64, hard=T), 3, sdc.sdy_of(y), [0.3, 0.2, 0.5, 0.4], PHI3)


def list_glob(y, T):
    """GLOB: a trig block + xdim = 1, lags = 2"""
    return general_spec(y, [("trig", 12.0, [1.0, 2.0])]) + sda.dynreg_ar_blocks(
        sdc.predictors(T + HORIZON, 1, 65, hard=T), 2, sdc.sdy_of(y), [0.4], PHI2[:1])


GLOB_DATA = dict(seasonal=(), trig=[(12.0, [1.0, 2.0])], missing=(31, 64, 128))
EDGE_CASES = {
    "small, T=70": (70, list_small, {}),
    "small, T=130": (130, list_small, {}),
    "plain ahead, lags 1, T=70": (70, list_plain_ahead, dict(seasonal=())),
    "plain ahead, lags 1, T=130": (130, list_plain_ahead, dict(seasonal=())),
    "LDC 33, xdim 4, T=70": (70, list_ldc33, dict(seasonal=((20, 1),))),
    "LDC 33, xdim 4, T=130": (130, list_ldc33, dict(seasonal=((20, 1),))),
    "GLOB, xdim 1, T=70": (70, list_glob, GLOB_DATA),
    "GLOB, xdim 1, T=130": (130, list_glob, GLOB_DATA),
}


# ---- the whole-rounds loops of the GPU test, T = 70
LOOP = dict(T=70, chains=4, seed=917, rounds=12, sig0=0.7, check=(0, 3))


def loop_case():
    """level + 4 seasons + xdim = 2, lags = 2"""
    c = dict(LOOP)
    c["X"], c["y"], c["obs"] = sdc.data(c["T"])
    c["blocks"] = general_spec(c["y"], [("level",), ("seasonal", 4, 1)]) + sda.dynreg_ar_blocks(
        sdc.predictors(c["T"] + HORIZON, 2, 66, hard=c["T"]), 2, sdc.sdy_of(c["y"]), [0.3, 0.5], PHI2[:2])
    c["g0"] = np.zeros(P, np.uint8)
    c["g0"][0] = 1
    c["b0"] = np.zeros(P)
    return c


def fallback_case():
    """xdim = 1, lags = 2, x = 1 on a series that grows by 6 % a step: the coefficient's least-squares phi lies
    outside the stationary region and the proposals' variance is small, so all 3 multivariate proposals fail
    and every round goes through draw_phi_univariate (tests/test_ss_dynreg_ar_cpu.py checks that it does)"""
    T = 70
    X, _, obs = sdc.data(T, seasonal=())
    t = np.arange(T)
    y = 0.5 * 1.06 ** t + 0.01 * np.sin(t)
    blocks = sda.dynreg_ar_blocks(np.ones((T + HORIZON, 1)), 2, sdc.sdy_of(y), [1.0], [[0.5, 0.1]], P0=np.full((1, 2), sdc.sdy_of(y) ** 2))
    g0 = np.zeros(P, np.uint8)
    g0[0] = 1
    return dict(T=T, chains=2, seed=919, rounds=4, sig0=0.7, check=(0, 1), X=X, y=y, obs=obs, blocks=blocks, g0=g0, b0=np.zeros(P))
