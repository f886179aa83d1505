"""A restatement of the AR dynamic regression (StateModels/DynamicRegressionArStateModel.cpp with
PosteriorSamplers/DynamicRegressionArPosteriorSampler.cpp; bsts AddDynamicRegression with
DynamicRegressionArOptions(lags); ba_ss_add_dynamic_regression_ar), one chain, on the device's substreams: the
parity yardstick of the autoregression blocks with a row of data that the general structural kernel's DR
instances serve.  The recursion is tests/ss_state_models_oracle.py's; this file adds the model's block class
(registered in that file's KINDS at import), ArPosteriorSampler in numpy, and the oracle that runs both.

The model, xdim coefficients of `lags` lags, is xdim blocks, one per coefficient (as the device stores it):
  state of block i = (beta_{t,i}, beta_{t-1,i}, .., beta_{t-lags+1,i});
  T = the companion matrix of phi_i (AutoRegressionTransitionMatrix: first row phi, ones below the diagonal);
  Z_t = x_{t,i} at the block's first component, 0 on its lags;  RQR = sigma_i^2 at the first component;
  the state error of a step: one rnorm_mt(0, sigma_i) at the first component;
  observe_state(then, now), t = 1 .. T - 1: ArModel i's add_mixture_data(now[0], then, 1.0):
      xtx += then then', xty += now[0] then, yty += now[0]^2, n += 1;
  initial state StateModelBase::simulate_initial_state: `lags` standard normals, sqrt(P0) z + a0;
  DynamicRegressionArPosteriorSampler::draw(): one ArPosteriorSampler::draw() per coefficient.

ArPosteriorSampler::draw() (ArPosteriorSampler.cpp:52-143) reads ONE generator in sequence: draw_phi -- up to
3 proposals rmvn_ivar(phi_hat, xtx / sigsq) of `lags` normals each, the first stationary one taken; none:
draw_phi_univariate, coefficient by coefficient a two-sided truncated normal on an interval that narrows
until the vector is stationary -- then draw_sigma with df = n and ss = phi'xtx phi - 2 phi'xty + yty.  The
arithmetic follows oracle/boom_oracle.c's ar_draw operation for operation (its Cholesky factor and its
solve are called through the oracle), so the two agree bit for bit: tests/test_ss_dynreg_ar_cpu.py pins it.

CONVENTIONS (the device's): block i reads the AR family's sampler id, 12 + 16 per earlier autoregression of
the list; in the state draw it reads one stream-2 normal per step t >= 1 whatever sigma_i.

A list for the oracle holds the model's blocks one dict each (dynreg_ar_blocks); engine_blocks() folds them
into the one dict per model that boom_amd.Engine.ss_set_state_models takes.
"""
import ctypes as C
import itertools

import numpy as np

import ss_state_models_oracle as ssm
from ss_autoar_oracle import stationarity_margin
from ss_state_models_oracle import Structure, dense_posterior, f64, impute_state  # noqa: F401

DYNREG_AR = "dynamic_regression_ar"


def companion(phi):
    L = len(phi)
    T = np.zeros((L, L))
    T[0, :] = phi
    T[np.arange(1, L), np.arange(L - 1)] = 1.0
    return T


def ar_suf(x):
    """ArStateModel::observe_state over a block's columns of a draw, in the reference's order"""
    T, L = x.shape
    xtx, xty, yty, n = np.zeros((L, L)), np.zeros(L), 0.0, 0.0
    for t in range(1, T):
        then, yy = x[t - 1], x[t, 0]
        for j in range(L):
            for i in range(L):
                xtx[i, j] += then[i] * then[j] * 1.0
        for i in range(L):
            xty[i] += (yy * 1.0) * then[i]
        yty += yy * yy * 1.0
        n += 1.0
    return dict(xtx=xtx, xty=xty, yty=yty, n=n)


class DynamicRegressionAr(ssm.Block):
    """one coefficient of an AR dynamic regression: an autoregression whose row of Z_t is its predictor.
    b["phi"] (default b["initial_phi"]) is the coefficient vector in hand: the Structure that holds the block
    is built again when it changes.  suf() leaves the ArModel statistics in self.ar; the block has no (n, sum
    of squares)."""

    family = "ar"

    def __init__(self, b):
        super().__init__(b)
        self.x = f64(b["predictors"]).reshape(-1)
        self.phi = f64(b.get("phi", b["initial_phi"]))
        assert len(self.phi) == self.dim == int(b["lags"])
        self.T = companion(self.phi)
        self.ar = None

    def z(self, t):
        return self.unit(0, self.x[t])

    def moves(self, t):
        return True

    def transition(self, t):
        return self.T

    def error(self, t, s, rnorm):
        return self.unit(0, np.sqrt(s[0]) * rnorm(0.0, 1.0))   # (one per step, whatever sigma)

    def forecast_error(self, t, s, rnorm):
        return self.unit(0, rnorm(0.0, 1.0) * np.sqrt(s[0]))

    def suf(self, x):
        self.ar = ar_suf(x)
        return self.one_slot(0.0, 0.0)

    def sampler_ids(self, ahead):
        return [12 + 16 * ahead]


ssm.KINDS[DYNREG_AR] = DynamicRegressionAr


# ---- ArPosteriorSampler --------------------------------------------------------------------------------------
class ArSampler:
    """ArPosteriorSampler for one ArModel.  After draw(): proposals (multivariate proposals made), univariate
    (the draw went through draw_phi_univariate), narrowed (candidates draw_phi_univariate refused); margin: the
    smallest distance of a stationarity decision from its boundary seen so far."""

    def __init__(self, o, lags, df, sigma_guess, sigma_upper_limit=np.inf):
        self.o, self.lib = o, o.lib
        lib = self.lib
        lib.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
        lib.bo_rnorm.restype = C.c_double
        lib.bo_rtrun_norm_2.argtypes = [C.c_void_p] + [C.c_double] * 4 + [C.POINTER(C.c_int)]
        lib.bo_rtrun_norm_2.restype = C.c_double
        self.L = int(lags)
        # ChisqModel(df, sigma_guess): 2 alpha = df, 2 beta = df sigma_guess^2
        self.prior_df = 2 * (df / 2.0)
        self.prior_ss = 2 * (df * sigma_guess * sigma_guess / 2.0)
        self.sigma_max = float(sigma_upper_limit)
        self.margin = np.inf
        self.proposals, self.univariate, self.narrowed = 0, False, 0

    def stationary(self, phi):
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        self.margin = min(self.margin, float(stationarity_margin(phi)))
        return bool(self.lib.bo_test_ar_check_stationary(len(phi), phi.ctypes.data_as(C.POINTER(C.c_double))))

    @staticmethod
    def ltsolve(Lc, x):
        """x: Lc' x = b, in place, from the last row up"""
        n = len(x)
        for i in range(n - 1, -1, -1):
            s = x[i]
            for j in range(i + 1, n):
                s -= Lc[j, i] * x[j]
            x[i] = s / Lc[i, i]
        return x

    def draw_phi(self, rng, phi, sigsq, xtx, xty):
        L = self.L
        self.proposals, self.univariate, self.narrowed = 0, False, 0
        phi_hat, ok = self.o.solve(xtx, xty)
        if not ok:
            raise RuntimeError("xtx is not positive definite")
        for _ in range(3):
            # rmvn_ivar(phi_hat, xtx / sigsq)
            Lc, pd = self.o.chol(xtx / sigsq)
            if not pd:
                raise RuntimeError("xtx / sigsq is not positive definite")
            z = np.array([self.lib.bo_rnorm(C.byref(rng), 0.0, 1.0) for _ in range(L)])
            cand = self.ltsolve(Lc, z) + phi_hat
            self.proposals += 1
            if self.stationary(cand):
                return cand
        # draw_phi_univariate
        self.univariate = True
        phi = np.array(phi, dtype=np.float64)
        if not self.stationary(phi):
            raise RuntimeError("draw_phi_univariate was called with an illegal initial value of phi")
        for i in range(L):
            initial_phi = phi[i]
            lo, hi = -1.0, 1.0
            ivar = xtx[i, i]
            dot = 0.0
            for j in range(L):
                dot += phi[j] * xtx[j, i]
            mu = (xty[i] - (dot - phi[i] * xtx[i, i])) / ivar
            while True:
                st = C.c_int(0)
                cand = self.lib.bo_rtrun_norm_2(C.byref(rng), mu, np.sqrt(1.0 / ivar), lo, hi, C.byref(st))
                if st.value:
                    raise RuntimeError("rtrun_norm_2")
                phi[i] = cand
                if self.stationary(phi):
                    break
                self.narrowed += 1
                if cand > initial_phi:
                    hi = cand
                else:
                    lo = cand
        return phi

    def draw_sigma(self, rng, phi, xtx, xty, yty, n):
        quad = lin = 0.0
        for i in range(self.L):
            row = 0.0
            for j in range(self.L):
                row += xtx[i, j] * phi[j]
            quad += phi[i] * row
            lin += phi[i] * xty[i]
        ss = quad - 2 * lin + yty
        DF, SS = n + self.prior_df, ss + self.prior_ss
        if self.sigma_max == 0.0:
            return 0.0
        if np.isinf(self.sigma_max):
            return 1.0 / self.o.gammas(rng, DF / 2, SS / 2, 1)[0]
        return 1.0 / self.o.trun_gammas(rng, DF / 2, SS / 2, 1.0 / (self.sigma_max * self.sigma_max), 1)[0]

    def draw(self, rng, phi, sigsq, suf):
        """one ArPosteriorSampler::draw() on suf = dict(xtx, xty, yty, n): (phi, sigsq)"""
        xtx, xty = f64(suf["xtx"]), f64(suf["xty"])
        phi = self.draw_phi(rng, phi, float(sigsq), xtx, xty)
        return phi, float(self.draw_sigma(rng, phi, xtx, xty, float(suf["yty"]), float(suf["n"])))


# ---- the blocks -------------------------------------------------------------------------------------------------
_model = itertools.count(1)


def dynreg_ar_blocks(predictors, lags, sdy, initial_sigma=None, initial_phi=None, a0=None, P0=None):
    """the xdim block dicts of one AR dynamic regression, bsts-style priors per coefficient as
    ss_dynreg_oracle.dynreg_block: sd prior guess 0.01 sd(y), df 0.01, upper limit sd(y); the initial state is
    bsts's N(0, 1) per component unless given (a0, P0: xdim x lags); initial_phi: xdim x lags, default zeros"""
    x = f64(predictors)
    d, L = x.shape[1], int(lags)
    sig = np.full(d, 0.3) if initial_sigma is None else f64(initial_sigma)
    phi = np.zeros((d, L)) if initial_phi is None else f64(initial_phi).reshape(d, L)
    a0 = np.zeros((d, L)) if a0 is None else f64(a0).reshape(d, L)
    P0 = np.ones((d, L)) if P0 is None else f64(P0).reshape(d, L)
    model = next(_model)
    return [dict(kind=DYNREG_AR, model=model, dim=L, lags=L, predictors=x[:, i:i + 1].copy(), nseasons=0, duration=1, t0=0,
                 df=np.full(1, 0.01), sigma_guess=np.full(1, 0.01 * sdy), sigma_upper_limit=np.full(1, sdy),
                 initial_sigma=sig[i:i + 1].copy(), initial_phi=phi[i].copy(), a0=a0[i].copy(), P0=P0[i].copy())
            for i in range(d)]


def engine_blocks(blocks):
    """the list as boom_amd.Engine.ss_set_state_models takes it: a model's consecutive block dicts folded into
    one dict of kind "dynamic_regression_ar"; every other dict as it is"""
    out = []
    for model, run in itertools.groupby(blocks, key=lambda b: b.get("model") if b["kind"] == DYNREG_AR else None):
        run = list(run)
        if model is None:
            out += run
            continue
        cat = {k: np.concatenate([f64(b[k]) for b in run]) for k in
               ("df", "sigma_guess", "sigma_upper_limit", "initial_sigma", "initial_phi", "a0", "P0")}
        out.append(dict(kind=DYNREG_AR, lags=run[0]["lags"], predictors=np.hstack([b["predictors"] for b in run]), **cat))
    return out


def scaled(blocks):
    """x -> 2 x with a0, sigma, sigma_guess, sigma_max -> 1/2 and P0 -> 1/4 on every block of an AR dynamic
    regression; phi unchanged.  Every scaling is a power of two: the coefficients' draws halve exactly."""
    out = []
    for b in blocks:
        if b["kind"] == DYNREG_AR:
            b = dict(b, predictors=2.0 * b["predictors"], a0=0.5 * b["a0"], P0=0.25 * b["P0"],
                     initial_sigma=0.5 * b["initial_sigma"], sigma_guess=0.5 * b["sigma_guess"],
                     sigma_upper_limit=0.5 * b["sigma_upper_limit"])
        out.append(b)
    return out


class DynRegArOracle(ssm.StateOracle):
    """the state half of one chain's draw for a list that holds AR dynamic regressions: StateOracle with the
    coefficients' phi (self.phi[k], None for the other blocks), their ArModel statistics (self.ar_suf[k]) and
    their samplers.  fallbacks: draws that went through draw_phi_univariate; ar_margin: the smallest distance
    of a stationarity decision from its boundary."""

    def __init__(self, o, T, observed, blocks, seed, chain):
        super().__init__(o, T, observed, blocks, seed, chain)
        self.base = blocks
        self.is_ar = [b["kind"] == DYNREG_AR for b in blocks]
        self.phi = [f64(b["initial_phi"]).copy() if ar else None for b, ar in zip(blocks, self.is_ar)]
        self.ar_suf = [None] * len(blocks)
        self.samplers = [ArSampler(o, b["lags"], float(b["df"][0]), float(b["sigma_guess"][0]), float(b["sigma_upper_limit"][0]))
                         if ar else None for b, ar in zip(blocks, self.is_ar)]
        self.fallbacks = 0

    @property
    def ar_margin(self):
        return min([s.margin for s in self.samplers if s is not None] + [np.inf])

    def restructure(self):
        """the matrices at the coefficients in hand (Structure's transition cache does not key on phi)"""
        self.blocks = [dict(b, phi=self.phi[k]) if ar else b for k, (b, ar) in enumerate(zip(self.base, self.is_ar))]
        self.S = Structure(self.blocks)

    def impute_state(self, ystar, sigsq_obs):
        st = super().impute_state(ystar, sigsq_obs)
        self.ar_suf = [k.ar if ar else None for k, ar in zip(self.S.parts, self.is_ar)]
        return st

    def draw_state_models(self):
        for k, model in enumerate(self.S.parts):
            if self.is_ar[k]:
                s = self.samplers[k]
                self.phi[k], self.var[k][0] = s.draw(self.var_rng[k][0], self.phi[k], self.var[k][0], self.ar_suf[k])
                self.fallbacks += int(s.univariate)
                continue
            pdf, pss, smax = self.var_prior[k]
            for v in range(len(self.var[k])):
                d = self._draw_variance(self.var_rng[k][v], self.suf_n[k][v] + pdf[v], self.suf_ss[k][v] + pss[v], smax[v])
                self.var[k][v] = model.variance(d)
        self.restructure()
