"""A restatement of StudentLocalLinearTrendStateModel and its posterior sampler (bsts
AddStudentLocalLinearTrend) inside StateSpacePosteriorSampler::draw(), one chain, in Python over the
oracle's primitives on the device's substreams: the parity yardstick of the state model kind 8
(ba_ss_add_state_model), built as tests/ss_student_oracle.py is and on its filter.

The block is a local linear trend -- state (level, slope), T = [[1, 1], [0, 1]], Z = (1, 0) --
whose errors of the step t -> t + 1 have the variances sigma_c^2 / w_c[t] (c = level, slope):
  * state_error_variance(t): RQR_t carries sigma_level^2 / w_level[t], sigma_slope^2 / w_slope[t];
  * simulate_state_error: two normals per step, eta_c = (sigma_c / sqrt(w_c[t - 1])) z for the step
    into t (sigma divided by sqrt(w), the reference's form);
  * observe_state(then, now, t), t = 1 .. T - 1, after clear_data(): r_level = level_t - (level_{t-1}
    + slope_{t-1}), r_slope = slope_t - slope_{t-1}, kept; WeightedGaussianSuf::update_raw with the OLD
    weight (n += 1, sumsq += r^2 w_old[t - 1]); then w_new[t - 1] ~ Gamma((nu + 1) / 2, rate (nu +
    r^2 / sigma^2) / 2); GammaSuf of the new weights (n, sum w, sum log w).  Entry T - 1 is never
    redrawn.  Weight c of step t -> t + 1 in the chain's s-th state draw reads stream 161 at slot
    (s T + t) 2 + c of 256 uniforms;
  * the sampler's draw(): sigma_level^2, nu_level, sigma_slope^2, nu_slope from stream 160, read in
    sequence.  sigma^2: GenericGaussianVarianceSampler::draw(n, sumsq).  nu: a NEW
    ScalarSliceSampler(logpost, unimodal = true) per draw, lower limit 0, suggested dx 1.0 --
    unimodal: find_upper_limit doubles only while logp(hi) >= the slice level, without the random
    extra doublings of student_oracle.slice_draw_nu.  The target by the CURRENT nu: <= 10
    NuPosteriorFast (the GammaSuf), > 10 NuPosteriorRobust (sum of dstudent over the kept residuals,
    sigma the value just drawn).
The other blocks' samplers read the streams the engine gives them (level 1, slope 6, seasonal 7, + 16
per earlier block of the family; the Student trend is in no family).

Round (StateSpacePosteriorSampler::draw): [first call: impute_state] | regression draw | the state
models' samplers | impute_state (the state draw with the weights in hand, then observe_state).
"""
import ctypes as C

import numpy as np
from scipy.special import gammaln

import ss_student_oracle as sso
from oracle_lib import BoRng
from ss_student_oracle import LEVEL, SEASONAL, TREND
from student_oracle import SliceError, nu_log_post, nu_log_prior

STUDENT_TREND = 8
PARAM_STREAM, WEIGHT_STREAM, WEIGHT_STRIDE = 160, 161, 256


class TrendStructure(sso.Structure):
    """sso.Structure with one Student local linear trend: a trend block whose rqr(t, .) divides by
    the weights self.w (2 x T: level, slope)"""

    def __init__(self, blocks, T):
        self.qt = [i for i, b in enumerate(blocks) if b["kind"] == STUDENT_TREND]
        assert len(self.qt) == 1
        self.qt = self.qt[0]
        super().__init__([dict(b, kind=TREND) if b["kind"] == STUDENT_TREND else b for b in blocks])
        self.w = np.ones((2, T))

    def rqr(self, t, sigsq):
        d = super().rqr(t, sigsq)
        f = self.first[self.qt]
        d[f] = sigsq[self.qt][0] / self.w[0, t]
        d[f + 1] = sigsq[self.qt][1] / self.w[1, t]
        return d


def simulate_forward(S, sigsq, H, rnorm):
    """sso.simulate_forward with the Student trend's simulate_state_error"""
    T, m = len(H), S.m
    st = np.zeros((T, m))
    ys = np.zeros(T)
    for t in range(T):
        if t == 0:
            for b, f in zip(S.blocks, S.first):
                if b["kind"] == LEVEL:
                    st[0, f] = rnorm(S.a0[f], np.sqrt(S.P0[f]))
                else:
                    z = [rnorm(0.0, 1.0) for _ in range(b["dim"])]
                    for i in range(b["dim"]):
                        st[0, f + i] = np.sqrt(S.P0[f + i]) * z[i] + S.a0[f + i]
        else:
            eta = np.zeros(m)
            for k, (b, f, s) in enumerate(zip(S.blocks, S.first, sigsq)):
                if b["kind"] == LEVEL:
                    eta[f] = rnorm(0.0, np.sqrt(s[0]))
                elif k == S.qt:
                    z0, z1 = rnorm(0.0, 1.0), rnorm(0.0, 1.0)
                    eta[f] = (np.sqrt(s[0]) / np.sqrt(S.w[0, t - 1])) * z0
                    eta[f + 1] = (np.sqrt(s[1]) / np.sqrt(S.w[1, t - 1])) * z1
                elif b["kind"] == TREND:
                    z0, z1 = rnorm(0.0, 1.0), rnorm(0.0, 1.0)
                    eta[f], eta[f + 1] = np.sqrt(s[0]) * z0 + 0.0, np.sqrt(s[1]) * z1 + 0.0
                elif sso.new_season(b, t):
                    eta[f] = rnorm(0.0, np.sqrt(s[0]))
            st[t] = S.Tmat(t - 1) @ st[t - 1] + eta
        ys[t] = rnorm(S.Z @ st[t], np.sqrt(H[t]))
    return st, ys


def impute_state(S, sigsq, ystar, observed, H, rnorm):
    """sso.impute_state on simulate_forward above (the filter, the smoother and the mean correction
    read the per-step state variance through S.rqr)"""
    return sso.impute_state(S, sigsq, ystar, observed, H, rnorm, simulate=simulate_forward)


def residuals(S, st):
    """observe_state's residuals of the steps 0 -> 1, ..., T - 2 -> T - 1: (2, T - 1)"""
    f = S.first[S.qt]
    return np.stack([st[1:, f] - (st[:-1, f] + st[:-1, f + 1]), st[1:, f + 1] - st[:-1, f + 1]])


def nu_posterior_fast(nu, n, sumw, sumlog, prior):
    """NuPosteriorFast"""
    nu2 = nu / 2.0
    ans = nu_log_prior(nu, prior)
    if ans == -np.inf:
        return ans
    ans += n * (nu2 * np.log(nu2) - gammaln(nu2))
    ans += (nu2 - 1) * sumlog
    ans -= nu2 * sumw
    return float(ans)


def nu_posterior_robust(nu, res, sigma, prior):
    """NuPosteriorRobust: prior + sum_t dstudent(r_t, 0, sigma, nu, log)"""
    res = np.asarray(res, dtype=float)
    return nu_log_post(nu, (res / sigma) ** 2, len(res) * np.log(sigma), prior)


def slice_draw_unimodal(unif, rexp1, logf, x, dx=1.0, info=None):
    """ScalarSliceSampler(logf, unimodal = true)::draw with lower limit 0: student_oracle.slice_draw_nu
    without the random doublings.  Returns (new x, smallest relative margin of the slice
    comparisons); info["uniforms_in_doubling"] counts the uniforms read before the first candidate"""
    margin = [np.inf]
    reads = [0]

    def u():
        reads[0] += 1
        return unif()

    def note(a, b):
        if np.isfinite(a) and np.isfinite(b):
            margin[0] = min(margin[0], abs(a - b) / max(abs(a), abs(b), 1e-300))

    logp_slice = logf(x) - rexp1()
    if not np.isfinite(logp_slice):
        raise SliceError("initial value leads to infinite probability")
    lo, hi = 0.0, x + dx
    logphi = logf(hi)
    note(logphi, logp_slice)
    doublings = 0
    while logphi >= logp_slice:
        hi = x + 2 * (hi - x)
        if not np.isfinite(hi):
            raise SliceError("infinite upper limit")
        logphi = logf(hi)
        note(logphi, logp_slice)
        doublings += 1
        if doublings > 100:
            raise SliceError("more than 100 doublings")
    if np.isnan(logphi):
        raise SliceError("upper limit gives NaN probability")
    if info is not None:
        info["uniforms_in_doubling"] = reads[0]
        info["doublings"] = doublings
    tries = 0
    while True:
        cand = lo + (hi - lo) * u()
        lp = logf(cand)
        note(lp, logp_slice)
        if not lp < logp_slice:
            return cand, margin[0]
        if cand > x:
            hi = cand
        else:
            lo = cand
        tries += 1
        if tries > 100:
            raise SliceError("number of tries exceeded")


def block_stream_ids(blocks):
    """the engine's sampler ids of the level / trend / seasonal blocks' variance samplers"""
    fam = {LEVEL: 0, SEASONAL: 0}
    out = []
    for b in blocks:
        k = b["kind"]
        if k == STUDENT_TREND:
            out.append([PARAM_STREAM, PARAM_STREAM])
        elif k == SEASONAL:
            out.append([7 + 16 * fam[SEASONAL]])
            fam[SEASONAL] += 1
        elif k == LEVEL:
            out.append([1 + 16 * fam[LEVEL]])
            fam[LEVEL] += 1
        elif k == TREND:
            out.append([1 + 16 * fam[LEVEL], 6 + 16 * fam[LEVEL]])
            fam[LEVEL] += 1
        else:
            raise AssertionError("parity cases: level, trend, seasonal, Student trend")
    return out


class StudentTrendOracle(sso.StateModelSamplers):
    """the state half of one chain's StateSpacePosteriorSampler::draw for a list of level / trend /
    seasonal blocks and one Student local linear trend, on the device's substreams; the regression
    half (the adjusted series y - X beta, the observation variance) is given by the caller"""

    def __init__(self, o, T, observed, blocks, seed, chain):
        sso.StateModelSamplers.__init__(self, o, blocks, seed, chain, block_stream_ids(blocks))
        self.L.bo_rng_slot.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
        self.L.bo_rng_slot.restype = None
        self.T = int(T)
        self.obs = np.ones(self.T, bool) if observed is None else np.asarray(observed).astype(bool)
        self.S = TrendStructure(blocks, self.T)
        self.qt = self.S.qt
        q = blocks[self.qt]
        self.nu = np.array(q["initial_nu"], dtype=float)
        self.nu_prior = [tuple(q["nu_priors"][0]), tuple(q["nu_priors"][1])]
        self.param_rng = o.rng_philox(self.seed, self.chain, PARAM_STREAM, 0)
        self.res = np.zeros((2, 0))
        self.wsuf = np.zeros(6)
        self.state = None
        self.draws = 0
        self.margin = np.inf
        self.slice_info = []

    @property
    def w(self):
        return self.S.w

    def set_weights(self, level_w, slope_w):
        self.S.w = np.stack([np.array(level_w, dtype=float), np.array(slope_w, dtype=float)])

    def _slot(self, stream, index, stride):
        r = BoRng()
        self.L.bo_rng_seed_philox(C.byref(r), self.seed, self.chain, stream, 0)
        self.L.bo_rng_slot(C.byref(r), int(index), int(stride))
        return r

    def observe_state(self):
        """over the draw in hand: residuals, the weighted statistics (old weights), the new weights"""
        T, s, k = self.T, self.draws, self.qt
        self.res = residuals(self.S, self.state)
        w = self.S.w.copy()
        self.suf_n[k] = np.full(2, float(T - 1))
        self.suf_ss[k] = np.array([float(np.sum(self.res[c] ** 2 * w[c, :T - 1])) for c in range(2)])
        for t in range(T - 1):
            for c in range(2):
                r = self.res[c, t]
                rng = self._slot(WEIGHT_STREAM, (s * T + t) * 2 + c, WEIGHT_STRIDE)
                w[c, t] = self.o.gammas(rng, .5 * (1 + self.nu[c]), .5 * (self.nu[c] + r * r / self.var[k][c]), 1)[0]
        self.S.w = w
        self.wsuf = np.concatenate([[T - 1, np.sum(w[c, :T - 1]), np.sum(np.log(w[c, :T - 1]))] for c in range(2)])
        self.draws += 1

    def impute_state(self, ystar, sigsq_obs):
        """Base::impute_state: the state draw with the weights in hand, then observe_state"""
        H = np.full(self.T, float(sigsq_obs))
        self.state = impute_state(self.S, self.var, np.asarray(ystar, float), self.obs, H, self._rnorm)
        self.suf_n, self.suf_ss = sso.state_model_suf(self.S, self.state)
        self.observe_state()
        return self.state

    def draw_parameters(self):
        """StudentLocalLinearTrendPosteriorSampler::draw"""
        L, k, rng = self.L, self.qt, self.param_rng
        pdf, pss, smax = self.var_prior[k]
        unif = lambda: L.bo_unif(C.byref(rng))               # noqa: E731
        rexp1 = lambda: 1.0 * L.bo_exp_rand(C.byref(rng))    # noqa: E731
        for c in range(2):
            self.var[k][c] = self._draw_variance(rng, self.suf_n[k][c] + pdf[c], self.suf_ss[k][c] + pss[c], smax[c])
            prior = self.nu_prior[c]
            if self.nu[c] > 10:
                res, sigma = self.res[c], np.sqrt(self.var[k][c])
                logf = lambda nu: nu_posterior_robust(nu, res, sigma, prior)   # noqa: E731
            else:
                n, sw, sl = self.wsuf[3 * c:3 * c + 3]
                logf = lambda nu: nu_posterior_fast(nu, n, sw, sl, prior)       # noqa: E731
            info = {}
            self.nu[c], m = slice_draw_unimodal(unif, rexp1, logf, self.nu[c], 1.0, info)
            self.margin = min(self.margin, m)
            self.slice_info.append(info)

    def draw_state_models(self):
        """every state model's sampler, in model order"""
        for k in range(len(self.blocks)):
            if k == self.qt:
                self.draw_parameters()
            else:
                self.draw_block_variances(k)
