"""A restatement of MLVS::draw() (multinomial logit spike and slab, mlm.spike's data-augmentation
move) on the device's substreams, in Python over the oracle's uniforms and normals
(oracle_lib.Oracle): the parity yardstick of ba_mlogit_sweep.  Not a test.

One draw() (Models/Glm/PosteriorSamplers/MLVS.cpp:71-75) = impute -> inclusion sweep -> beta.

  impute (MLVS_data_imputer.cpp:51-82), per observation i with response y, on stream 48 at slot
  s n + i of 64 (spill as the oracle's bo_rng_slot does):
    eta_m = row (i, m) of the expanded design times beta; loglam = lse(eta);
    logzmin = rlexp(loglam); u_y = -logzmin; for m = 0 .. M - 1 in order: if m != y,
    u_m = -lse2(logzmin, rlexp(eta_m)); k = unmix(u_m - eta_m); u_m -= mu_k; w_m = sigsq_inv_k.
    rlexp(l) = log(-log(U)) - l, U redrawn while that is not finite (distributions/rlexp.cpp:25-31).
    unmix: log_mixing_weights + dnorm(., mu, sd, log), normalize_logprob (max-subtract, exp,
    divide by the sum), rmulti_mt (one uniform on (0, probsum), the first k with tmp <= psum).
  suf (MultinomialLogitCompleteDataSuf.cpp:41-50): X'WX, X'Wu, weighted_sum_of_squares.
  sweep (MLVS.cpp:120-190): log_model_prob from scratch per flip; the one fixed visiting order,
    its first min(D, max_flips) entries; a flip is kept iff u < logit_inv(logp_new - logp_old),
    evaluated as the device does, log(u) - log1p(-u) <= logp_new - logp_old; the empty model's
    value is log prior + wss / 2.  Every flip consumes its uniform (the reference skips it when
    logp_new is not finite): stream positions are known up front.  Stream 3: the sweep's
    max_flips uniforms, then the k normals of beta.
  beta (MLVS.cpp:101-118): rmvn_ivar about V_g^{-1}(X'Wu_g + Omega^{-1}_g mu_g).

Recorded per sweep: the smallest |delta - logit(u)| over the flips with a finite logp_new, the
smallest unmix margin min |tmp - psum_k| / probsum, and the number of rlexp retries.
"""
import ctypes as C
import math

import numpy as np

from oracle_lib import BoRng, f64

IMPUTE_STREAM, IMPUTE_STRIDE = 48, 64
LN_SQRT_2PI = 0.918938533204672741780329736406

# the normal mixture for the extreme value distribution: the three literal vectors of
# MLVS_data_imputer.cpp:39-43 (means, variances, weights) and what the constructor derives
MIX_MU = np.array([5.09, 3.29, 1.82, 1.24, 0.76, 0.39, 0.04, -0.31, -0.67, -1.06])
MIX_VAR = np.array([4.5, 2.02, 1.1, 0.42, 0.2, 0.11, 0.08, 0.08, 0.09, 0.15])
MIX_WEIGHT = np.array([0.004, 0.04, 0.168, 0.147, 0.125, 0.101, 0.104, 0.116, 0.107, 0.088])
MIX_PREC = np.array([math.pow(v, -1.0) for v in MIX_VAR])
MIX_SD = np.array([math.pow(v, -0.5) for v in MIX_PREC])
MIX_LOGSD = np.array([math.log(v) for v in MIX_SD])
MIX_LOGW = np.array([math.log(v) for v in MIX_WEIGHT])
# (plain floats for the scalar code below)
_MU, _SD, _PREC, _LOGSD, _LOGW = (a.tolist() for a in (MIX_MU, MIX_SD, MIX_PREC, MIX_LOGSD, MIX_LOGW))


def expand_design(Xsubject, Xchoice, n, M):
    """ChoiceData::write_x(false) (Models/Glm/ChoiceData.cpp:93-115) for every (i, m): N = n M
    rows (row i M + m) by D = (M - 1) psub + pch columns"""
    psub = 0 if Xsubject is None else np.asarray(Xsubject).shape[1]
    pch = 0 if Xchoice is None else np.asarray(Xchoice).shape[1]
    X = np.zeros((n * M, (M - 1) * psub + pch))
    for m in range(1, M):
        if psub:
            X[m::M, (m - 1) * psub:m * psub] = Xsubject
    if pch:
        X[:, (M - 1) * psub:] = Xchoice
    return X


def lse(eta, M=math):
    """lse_safe (cpputil/lse.cpp:27-40)"""
    m = max(eta)
    if m == -math.inf:
        return m
    tot = 0.0
    for e in eta:
        tot += M.exp(e - m)
    return m + M.log(tot) if tot > 0 else -math.inf


def lse2(x, y, M=math):
    """cpputil/lse.hpp:31-39"""
    if x < y:
        x, y = y, x
    return x + M.log1p(M.exp(y - x))


# The scalar functions here (lse and lse2 above too) take the math functions they call as `M` (exp, log, log1p, isfinite,
# inf), the module `math` unless the caller says otherwise: tests/latent_ref.py passes
# imputer_ref's table, which moves the results as another library would.
def _fused(v, M):
    """an a + b c the device may round once: a table's replays move it by an ulp (M.fused); the
    value itself on the plain module"""
    f = getattr(M, "fused", None)
    return v if f is None else f(v)


def unmix_posterior(v, M=math):
    """the ten normalised posterior terms of unmix (MLVS_data_imputer.cpp:76-82)"""
    pp = []
    for c in range(10):
        xs = (v - _MU[c]) / _SD[c]
        pp.append(_LOGW[c] + -_fused(LN_SQRT_2PI + 0.5 * xs * xs + _LOGSD[c], M))
    mx = max(pp)
    nc = 0.0
    for c in range(10):
        pp[c] = M.exp(pp[c] - mx)
        nc += pp[c]
    return [q / nc for q in pp]


def unmix(v, unif, M=math):
    """(component, margin): rmulti_mt (distributions/rmulti.cpp:41-78) on the posterior terms"""
    pp = unmix_posterior(v, M)
    probsum = 0.0
    for q in pp:
        probsum += q
    tmp = 0.0 + (probsum - 0.0) * unif()
    psum, ind, margin = 0.0, -1, math.inf
    for c in range(10):
        psum += pp[c]
        margin = min(margin, abs(tmp - psum) / probsum)
        if ind < 0 and tmp <= psum:
            ind = c
    if ind < 0:
        raise RuntimeError("rmulti failed")
    return ind, margin


def rlexp(loglam, unif, stats, M=math):
    """distributions/rlexp.cpp:25-31"""
    while True:
        u = unif()
        a = -M.log(u)
        ans = M.log(a) if a > 0 else -math.inf
        if math.isfinite(ans):
            return ans - loglam
        stats["retries"] += 1


def impute_point(eta, y, unif, stats=None, shift=True, M=math):
    """(u, w) of one observation, one per choice; unif() reads the observation's slot.  shift=False
    leaves the component's mean in (the utilities themselves).  stats["comps"], where the caller
    put a list there, gets every choice's mixture component"""
    stats = stats if stats is not None else {"retries": 0, "unmix_margin": math.inf}
    nch = len(eta)
    loglam = lse(eta, M)
    if not math.isfinite(loglam) or not all(math.isfinite(e) for e in eta):
        raise RuntimeError("non-finite linear predictor")
    logzmin = rlexp(loglam, unif, stats, M)
    u, w = [0.0] * nch, [0.0] * nch
    for m in range(nch):
        um = -logzmin
        if m != y:
            um = -lse2(logzmin, rlexp(eta[m], unif, stats, M), M)
        k, mg = unmix(um - eta[m], unif, M)
        stats["unmix_margin"] = min(stats.get("unmix_margin", math.inf), mg)
        if "comps" in stats:
            stats["comps"].append(k)
        if shift:
            um -= _MU[k]
        u[m] = um
        w[m] = _PREC[k]
    return u, w


def impute_batch(eta, y, U0, U1, U2):
    """impute_point for n observations at once (numpy), given the uniforms: U0 n for
    rlexp(loglam), U1 n x M for rlexp(eta_m) (column y_i unused), U2 n x M for unmix.  The
    statistical tests' imputer (the law is impute_point's; tests/test_mlogit_cpu.py holds the two
    together on the same uniforms).  No rlexp retries: a uniform whose log(-log(U)) is not
    finite is an error here."""
    eta = np.asarray(eta, dtype=np.float64)
    n, M = eta.shape
    rows = np.arange(n)
    mx = eta.max(axis=1)
    loglam = mx + np.log(np.exp(eta - mx[:, None]).sum(axis=1))
    with np.errstate(divide="ignore"):
        a0, a1 = np.log(-np.log(U0)), np.log(-np.log(U1))
    a1[rows, y] = 0.0
    if not (np.all(np.isfinite(a0)) and np.all(np.isfinite(a1))):
        raise RuntimeError("a uniform whose double logarithm is not finite")
    logzmin = a0 - loglam
    tmp = a1 - eta
    hi, lo = np.maximum(logzmin[:, None], tmp), np.minimum(logzmin[:, None], tmp)
    u = -(hi + np.log1p(np.exp(lo - hi)))
    u[rows, y] = -logzmin
    xs = ((u - eta)[:, :, None] - MIX_MU) / MIX_SD
    pp = MIX_LOGW + -(LN_SQRT_2PI + 0.5 * xs * xs + MIX_LOGSD)
    pp = np.exp(pp - pp.max(axis=2, keepdims=True))
    pp /= pp.sum(axis=2, keepdims=True)
    cum = np.cumsum(pp, axis=2)
    k = np.argmax((cum[:, :, -1] * U2)[:, :, None] <= cum, axis=2)
    return u - MIX_MU[k], MIX_PREC[k], k


class MlogitOracle:
    """One chain of MLVS on the device's substreams.  rng=None: the oracle's Philox streams
    (parity with the device); a numpy Generator: the same law on its uniforms and normals
    (the statistical tests; impute_batch).  rules="logit" swaps the sweep's three MLVS traits
    for BinomialLogitSpikeSlabSampler's -- its whole-range shuffle of the identity (D uniforms
    first), log(u) <= delta, no wss in the empty model's value: what the sweep's mode 2 would
    draw on the same latent data (the test that mode 3 is not mode 2)."""

    def __init__(self, o, y, Xsubject, Xchoice, nchoices, mu, prec, pi, seed, chain, gamma0, beta0=None,
                 flip_order=None, max_flips=-1, max_model_size=-1, select=True, rng=None, rules="mlvs"):
        self.o = o
        self.rules = rules
        self.y = np.asarray(y, dtype=np.int64)
        self.n, self.M = self.y.shape[0], int(nchoices)
        self.X = expand_design(Xsubject, Xchoice, self.n, self.M)
        self.N, self.D = self.X.shape
        self.mu, self.prec, self.pi = f64(mu), np.asarray(prec, dtype=np.float64), f64(pi)
        self.seed, self.chain = int(seed), int(chain)
        self.gamma = np.ascontiguousarray(gamma0, dtype=np.uint8).copy()
        self.beta = np.zeros(self.D) if beta0 is None else f64(beta0) * self.gamma
        self.order = np.arange(self.D) if flip_order is None else np.asarray(flip_order, dtype=np.int64)
        self.max_flips, self.max_model_size, self.select = int(max_flips), int(max_model_size), bool(select)
        self.gen = rng
        if rng is None:
            L = o.lib
            L.bo_rng_slot.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
            L.bo_rng_slot.restype = None
            self.sweep_rng = BoRng()
            L.bo_rng_seed_philox(C.byref(self.sweep_rng), self.seed, self.chain, 3, 0)
        self.sweep = 0
        with np.errstate(divide="ignore"):
            self.l1, self.l0 = np.log(self.pi), np.log1p(-self.pi)
        self.u = self.w = None
        self.wss = 0.0
        self.flip_margin, self.unmix_margin, self.retries = [], [], []

    # ---- random numbers ------------------------------------------------------------------
    def _slot_unif(self, index):
        if self.gen is not None:
            return self.gen.random
        r = BoRng()
        L = self.o.lib
        L.bo_rng_seed_philox(C.byref(r), self.seed, self.chain, IMPUTE_STREAM, 0)
        L.bo_rng_slot(C.byref(r), int(index), IMPUTE_STRIDE)
        return lambda: L.bo_unif(C.byref(r))

    def _sweep_unif(self):
        return self.gen.random() if self.gen is not None else self.o.lib.bo_unif(C.byref(self.sweep_rng))

    def _sweep_norms(self, k):
        return self.gen.standard_normal(k) if self.gen is not None else self.o.norms(self.sweep_rng, k)

    # ---- impute --------------------------------------------------------------------------
    def impute(self):
        n, M, s = self.n, self.M, self.sweep
        inc = np.flatnonzero(self.gamma)
        eta = (self.X[:, inc] @ self.beta[inc]).reshape(n, M)
        if self.gen is not None:
            ub, wb, _ = impute_batch(eta, self.y, self.gen.random(n), self.gen.random((n, M)), self.gen.random((n, M)))
            self.u, self.w = ub.ravel(), wb.ravel()
            self.wss = float(np.sum(self.w * self.u * self.u))
            self.xtwu = self.X.T @ (self.w * self.u)
            self.retries.append(0)
            self.unmix_margin.append(math.inf)
            return
        u, w = np.zeros(self.N), np.zeros(self.N)
        stats = {"retries": 0, "unmix_margin": math.inf}
        for i in range(n):
            ui, wi = impute_point([float(e) for e in eta[i]], int(self.y[i]), self._slot_unif(s * n + i), stats)
            u[i * M:(i + 1) * M] = ui
            w[i * M:(i + 1) * M] = wi
        self.u, self.w = u, w
        self.wss = float(np.sum(w * u * u))
        self.xtwu = self.X.T @ (w * u)
        self.retries.append(stats["retries"])
        self.unmix_margin.append(stats["unmix_margin"])

    # ---- log_model_prob (MLVS.cpp:163-190) -----------------------------------------------
    def log_prior(self, g):
        lp = 0.0
        for j in range(self.D):
            t = self.l1[j] if g[j] else self.l0[j]
            if t == -math.inf:
                return -math.inf
            lp += t
        if self.max_model_size >= 0 and int(g.sum()) > self.max_model_size:
            return -math.inf
        return lp

    def _posterior(self, g):
        """(chol(Ominv), Ominv mu, chol(Ominv + X'WX), L^{-1}(X'Wu + Ominv mu)) of model g, or None"""
        idx = np.flatnonzero(g)
        Xg = self.X[:, idx]
        Ominv = self.prec[np.ix_(idx, idx)]
        try:
            Lo = np.linalg.cholesky(Ominv)
            L = np.linalg.cholesky(Ominv + Xg.T @ (Xg * self.w[:, None]))
        except np.linalg.LinAlgError:
            return None
        Om = Ominv @ self.mu[idx]
        S = np.linalg.solve(L, self.xtwu[idx] + Om)   # (a triangular system: exact to rounding)
        return Lo, Om, L, S

    def log_model_prob(self, g):
        num = self.log_prior(g)
        if num == -math.inf:
            return num
        idx = np.flatnonzero(g)
        if idx.size == 0:
            if self.rules == "logit":
                return num
            return num - -.5 * self.wss   # (the reference's sign, MLVS.cpp:166-168)
        po = self._posterior(g)
        if po is None:
            return -math.inf
        Lo, Om, L, S = po
        num += .5 * (2.0 * float(np.sum(np.log(np.diag(Lo)))))
        num -= .5 * float(self.mu[idx] @ Om)
        denom = float(np.sum(np.log(np.diag(L)))) - .5 * float(S @ S)
        return num - denom

    # ---- draw ----------------------------------------------------------------------------
    def draw_inclusion_vector(self):
        g = self.gamma.copy()
        logp = self.log_model_prob(g)
        if not math.isfinite(logp):
            raise RuntimeError("MLVS did not start with a legal configuration.")
        hi = self.D if self.max_flips <= 0 else min(self.D, self.max_flips)
        margin = math.inf
        order = self.order
        if self.rules == "logit":   # BinomialLogitSpikeSlabSampler.cpp:181-187
            order = np.arange(self.D)
            if self.D > 1:
                for i in range(self.D):
                    j = int(math.floor(self.D * self._sweep_unif()))
                    order[i], order[j] = order[j], order[i]
        for i in range(hi):
            j = int(order[i])
            g[j] ^= 1
            logp_new = self.log_model_prob(g)
            u = self._sweep_unif()
            ell = math.log(u) if self.rules == "logit" else math.log(u) - math.log1p(-u)
            delta = logp_new - logp
            if math.isfinite(logp_new):
                margin = min(margin, abs(delta - ell))
            if ell <= delta:
                logp = logp_new
            else:
                g[j] ^= 1
        self.gamma = g
        self.flip_margin.append(margin)

    def draw_beta(self):
        beta = np.zeros(self.D)
        idx = np.flatnonzero(self.gamma)
        if idx.size:
            po = self._posterior(self.gamma)
            if po is None:
                raise RuntimeError("The posterior information matrix is not positive definite.")
            _, _, L, S = po
            z = self._sweep_norms(idx.size)
            beta[idx] = np.linalg.solve(L.T, S + z)   # rmvn_ivar: mean + L^{-T} z
        self.beta = beta

    def draw(self):
        self.impute()
        if self.select:
            self.draw_inclusion_vector()
        else:
            self.flip_margin.append(math.inf)
        self.draw_beta()
        self.sweep += 1
        return self.gamma.copy(), self.beta.copy()
