"""A restatement of HierarchicalRegressionHolidayStateModel's sampler, HierGaussianRegressionAsisSampler::draw
(Models/Hierarchical/PosteriorSamplers/HierGaussianRegressionAsisSampler.cpp; bsts
AddHierarchicalRegressionHoliday; ba_ss_add_hierarchical_regression_holiday), in numpy, one chain, built on
ss_regholiday_oracle.py: to the state space model the hierarchical model is the plain one.

The draw, given sigma^2, the totals s_h and counts n_h of the last state draw (holiday h's regression
sufficient statistics are xtx = diag(n_h), xty = s_h) and the current mu and Omega, in this order of random
numbers:
  1  h = 0 .. H - 1: beta_h = L'^-1 z + A^-1 b, A = diag(n_h) / sigma^2 + Omega = L L', b = s_h / sigma^2 + Omega mu,
     z = d normals                                    (RegressionCoefficientSampler.cpp:34-46, mvn.cpp:114-122)
  2  (a) I = H Omega + Sigma0^-1, mu' = rmvn_ivar(I^-1 (H (Omega betabar) + Sigma0^-1 mu0), I): d normals; betabar is
         MvnSuf::update_raw's running mean                                      (MvnMeanSampler.cpp:101-110)
     (b) rWish(nu0 + H, ...): overwritten by step 3 without being read -- its numbers are consumed, its matrix
         (step 3's) is not formed                                     (MvnVarSampler.cpp:48-61, Wishart.cpp:32-60)
  3  c_h = beta_h - mu'; mu = the coefficient draw with A = sum_h diag(n_h) / sigma^2 + Sigma0^-1,
     b = sum_h (s_h - n_h c_h) / sigma^2 + Sigma0^-1 mu0: d normals; Omega = rWish(nu0 + H, (sum_h c_h c_h' + S0)^-1),
     S0 = nu0 x variance_guess (WishartModel.cpp:117).  The beta_h stay as step 1 drew them.

Every function takes `dt`, numpy.float64 or numpy.longdouble, and runs the same loops in that type: the sums in
the order boom_amd/csrc/mvn_wishart_device.h writes down, one operation at a time (no fused multiply-add), so
the float64 run is the device's arithmetic and the long double run measures its rounding error.  The normals and
gammas are callables: rnorm() a standard normal, rgamma(shape, scale).

CONVENTIONS (the device's): all hierarchical models of a chain read Philox sampler id 163 at one position per
chain, in (model, step) order; a plain model on the same list keeps id 162.
"""
import ctypes as C

import numpy as np

import ss_regholiday_oracle as sro
from ss_regholiday_oracle import f64

HIER = "hierarchical_regression_holiday"
STREAM = 163
BAD_DRAW = 16   # RHH_BAD_DRAW


class NotPositiveDefinite(Exception):
    pass


def hier_model(nholidays, width, mean_prior, variance_prior, calendar, coefficients=None):
    """mean_prior = (mu0, Sigma0), variance_prior = (variance_guess, variance_guess_weight): a block of
    Engine.ss_set_state_models; `widths` and `prior` make it a model ss_regholiday_oracle's functions take"""
    n = int(nholidays) * int(width)
    cal = None if calendar is None else np.asarray(calendar, dtype=np.int32)
    assert cal is None or (cal.min() >= -1 and cal.max() < n)
    return dict(kind=HIER, nholidays=int(nholidays), width=int(width), widths=[int(width)] * int(nholidays), prior=(0.0, 1.0),
                mean_prior=(f64(mean_prior[0]), f64(mean_prior[1])), variance_prior=(f64(variance_prior[0]), float(variance_prior[1])),
                calendar=cal, coefficients=np.zeros(n) if coefficients is None else f64(coefficients))


def is_model(b):
    return b["kind"] in (sro.REGHOLIDAY, HIER)


def split(blocks):
    return [b for b in blocks if not is_model(b)], [b for b in blocks if is_model(b)]


# ---- the linear algebra, in the device's order -------------------------------------------------------------
def chol(A, dt=np.float64):
    """left-looking by column: s = a_rj - l_r0 l_j0 - l_r1 l_j1 - ..."""
    d = A.shape[0]
    L = np.zeros((d, d), dtype=dt)
    for j in range(d):
        for r in range(j, d):
            s = dt(A[r, j])
            for k in range(j):
                s = s - L[r, k] * L[j, k]
            if r == j:
                if not (s > 0 and np.isfinite(s)):
                    raise NotPositiveDefinite()
                L[j, j] = np.sqrt(s)
            else:
                L[r, j] = s / L[j, j]
    return L


def forward(L, b, dt=np.float64):
    d = len(b)
    x = np.zeros(d, dtype=dt)
    for r in range(d):
        v = dt(b[r])
        for k in range(r):
            v = v - L[r, k] * x[k]
        x[r] = v / L[r, r]
    return x


def backward(L, b, dt=np.float64):
    """L'x = b"""
    d = len(b)
    x = np.zeros(d, dtype=dt)
    for r in range(d - 1, -1, -1):
        v = dt(b[r])
        for k in range(d - 1, r, -1):
            v = v - L[k, r] * x[k]
        x[r] = v / L[r, r]
    return x


def inverse_from_factor(L, dt=np.float64):
    """(L L')^-1 = W'W, W = L^-1 by columns"""
    d = L.shape[0]
    W = np.zeros((d, d), dtype=dt)
    for c in range(d):
        for i in range(c, d):
            s = dt(1.0 if i == c else 0.0)
            for k in range(c, i):
                s = s - L[i, k] * W[k, c]
            W[i, c] = s / L[i, i]
    V = np.zeros((d, d), dtype=dt)
    for r in range(d):
        for c in range(d):
            s = dt(0.0)
            for k in range(max(r, c), d):
                s = s + W[k, r] * W[k, c]
            V[r, c] = s
    return V


def mvn_draw(A, b, z, dt=np.float64):
    """sample_regression_coefficients: N(A^-1 b, A^-1) as L'^-1 z + L'^-1 L^-1 b"""
    L = chol(A, dt)
    m = backward(L, forward(L, b, dt), dt)
    return backward(L, np.asarray(z, dtype=dt), dt) + m


def bartlett(d, nu, rnorm, rgamma, dt=np.float64):
    """WishartTriangle: row i = sqrt(rchisq(nu - i)) on the diagonal, then i normals to its left;
    rchisq(df) = rgamma(df / 2, scale 2)"""
    T = np.zeros((d, d), dtype=dt)
    for i in range(d):
        T[i, i] = np.sqrt(dt(rgamma((nu - i) / 2.0, 2.0)))
        for j in range(i):
            T[i, j] = dt(rnorm())
    return T


def wishart_product(Cf, T, dt=np.float64):
    """(C T)(C T)' for two lower triangles"""
    d = Cf.shape[0]
    P = np.zeros((d, d), dtype=dt)
    for r in range(d):
        for c in range(r + 1):
            s = dt(0.0)
            for k in range(c, r + 1):
                s = s + Cf[r, k] * T[k, c]
            P[r, c] = s
    out = np.zeros((d, d), dtype=dt)
    for r in range(d):
        for c in range(d):
            s = dt(0.0)
            for k in range(min(r, c) + 1):
                s = s + P[r, k] * P[c, k]
            out[r, c] = s
    return out


def rwish(nu, V, rnorm, rgamma, dt=np.float64):
    """rWish_mt(nu, V): the triangle first, then V's factor"""
    T = bartlett(V.shape[0], nu, rnorm, rgamma, dt)
    return wishart_product(chol(V, dt), T, dt)


def hyper(model, dt=np.float64):
    """Sigma0^-1, Sigma0^-1 mu0 and S0, formed once -- in float64 whatever dt is: they are the host's, inputs
    of the draw"""
    mu0, Sigma0 = model["mean_prior"]
    guess, weight = model["variance_prior"]
    sinv0 = inverse_from_factor(chol(f64(Sigma0)))
    d = len(mu0)
    sinv0mu0 = np.zeros(d)
    for r in range(d):
        for c in range(d):
            sinv0mu0[r] += sinv0[r, c] * mu0[c]
    return dict(sinv0=sinv0.astype(dt), sinv0mu0=sinv0mu0.astype(dt), s0=(f64(guess) * weight).astype(dt), nu0=float(weight))


def draw(model, sigsq, totals, counts, mu, omega, rnorm, rgamma, dt=np.float64):
    """one draw of the sampler: dict(beta (H x d), mu1 -- step 2's mu' --, mu, omega); NotPositiveDefinite or
    FloatingPointError-free NaNs are the caller's to judge (see draw_or_none)"""
    H, d = model["nholidays"], model["width"]
    hy = hyper(model, dt)
    sig = dt(sigsq)
    s = np.asarray(totals, dtype=dt).reshape(H, d)
    n = np.asarray(counts, dtype=dt).reshape(H, d)
    mu = np.asarray(mu, dtype=dt)
    om = np.asarray(omega, dtype=dt)
    # step 1
    z = np.array([[rnorm() for _ in range(d)] for _ in range(H)], dtype=dt)
    om_mu = np.zeros(d, dtype=dt)
    for r in range(d):
        for c in range(d):
            om_mu[r] = om_mu[r] + om[r, c] * mu[c]
    beta = np.zeros((H, d), dtype=dt)
    for h in range(H):
        A = om.copy()
        for r in range(d):
            A[r, r] = n[h, r] / sig + om[r, r]
        beta[h] = mvn_draw(A, s[h] / sig + om_mu, z[h], dt)
    # step 2 (a)
    bar = np.zeros(d, dtype=dt)
    for h in range(H):
        bar = bar + (beta[h] - bar) / dt(h + 1)
    Hn = dt(H)
    I = Hn * om + hy["sinv0"]
    b = np.zeros(d, dtype=dt)
    for r in range(d):
        acc = dt(0.0)
        for c in range(d):
            acc = acc + om[r, c] * bar[c]
        b[r] = Hn * acc + hy["sinv0mu0"][r]
    mu1 = mvn_draw(I, b, [rnorm() for _ in range(d)], dt)
    # step 2 (b): consumed
    bartlett(d, hy["nu0"] + H, rnorm, rgamma, dt)
    # step 3
    c = beta - mu1
    xtx = np.zeros(d, dtype=dt)
    xty = np.zeros(d, dtype=dt)
    for h in range(H):
        xtx = xtx + n[h]
        xty = xty + (s[h] - n[h] * c[h])
    A = hy["sinv0"].copy()
    for r in range(d):
        A[r, r] = xtx[r] / sig + hy["sinv0"][r, r]
    mu2 = mvn_draw(A, xty / sig + hy["sinv0mu0"], [rnorm() for _ in range(d)], dt)
    SS = np.zeros((d, d), dtype=dt)
    for r in range(d):
        for cc in range(d):
            acc = dt(0.0)
            for h in range(H):
                acc = acc + c[h, r] * c[h, cc]
            SS[r, cc] = acc + hy["s0"][r, cc]
    V = inverse_from_factor(chol(SS, dt), dt)
    omega = rwish(hy["nu0"] + H, V, rnorm, rgamma, dt)
    return dict(beta=beta, mu1=mu1, mu=mu2, omega=omega)


def count_draws(H, d):
    """the normals and gammas a round consumes: H d + 2 d + 2 (d + d (d - 1) / 2)"""
    return H * d + 2 * d + 2 * (d + d * (d - 1) // 2)


# ---- the oracle's generator as the callables ------------------------------------------------------------------
class PhiloxDraws:
    """rnorm / rgamma on the compiled oracle's Philox stream: what the device's d_rnorm / d_rgamma_scale read"""

    def __init__(self, o, seed, chain, pos=0, stream=STREAM):
        self.L = o.lib
        self.L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
        self.L.bo_rnorm.restype = C.c_double
        self.rng = o.rng_philox(int(seed), int(chain), stream, int(pos))
        self.status = C.c_int(0)

    @property
    def pos(self):
        return int(self.rng.pos)

    def rnorm(self):
        return self.L.bo_rnorm(C.byref(self.rng), 0.0, 1.0)

    def rgamma(self, shape, scale):
        return self.L.bo_rgamma(C.byref(self.rng), float(shape), 1.0 / float(scale), C.byref(self.status))


class Replay:
    """records a generator's numbers, or replays a record: the long double run reads what the float64 run read"""

    def __init__(self, source=None, record=None):
        self.source, self.record, self.at = source, [] if record is None else record, 0

    def _next(self, make):
        if self.source is not None:
            self.record.append(make())
            return self.record[-1]
        self.at += 1
        return self.record[self.at - 1]

    def rnorm(self):
        return self._next(lambda: self.source.rnorm())

    def rgamma(self, shape, scale):
        return self._next(lambda: self.source.rgamma(shape, scale))


def draw_both(model, sigsq, totals, counts, mu, omega, source):
    """the float64 draw on `source` and the long double draw on the same numbers"""
    rec = Replay(source)
    lo = draw(model, sigsq, totals, counts, mu, omega, rec.rnorm, rec.rgamma, np.float64)
    rep = Replay(record=rec.record)
    hi = draw(model, sigsq, totals, counts, mu, omega, rep.rnorm, rep.rgamma, np.longdouble)
    assert rep.at == len(rec.record)
    return lo, hi


EPS = 2.0 ** -52


def gate(lo, hi, scale):
    """per output: 4 |float64 - long double| + 8 ulp of `scale`, the largest magnitude entering it"""
    return 4.0 * np.abs(lo.astype(np.longdouble) - hi).astype(np.float64) + 8.0 * EPS * scale


# ---- one chain of a list with plain and hierarchical models --------------------------------------------------------
class HierRegHolidayOracle(sro.RegHolidayOracle):
    """RegHolidayOracle with the hierarchical models' sampler: their draws come first (the device launches
    rhh_draw_kernel ahead of rh_draw_kernel), each kind from its own stream"""

    def __init__(self, o, base, models, y, X, seed, chain):
        super().__init__(o, base, models, y, X, seed, chain)
        self.hrng = PhiloxDraws(o, seed, chain)
        self.mu = [np.zeros(m["width"]) if m["kind"] == HIER else None for m in models]
        self.omega = [np.eye(m["width"]) if m["kind"] == HIER else None for m in models]
        self.last = [None] * len(models)   # (float64 draw, long double draw) of the last round

    def draw_coefficients(self, sigsq):
        out = [None] * len(self.models)
        for k, m in enumerate(self.models):
            if m["kind"] != HIER:
                continue
            lo, hi = draw_both(m, sigsq, self.totals[k], self.counts[k], self.mu[k], self.omega[k], self.hrng)
            self.last[k] = (lo, hi)
            out[k], self.mu[k], self.omega[k] = lo["beta"].reshape(-1), lo["mu"], lo["omega"]
        for k, m in enumerate(self.models):
            if m["kind"] == HIER:
                continue
            out[k] = sro.draw([m], [self.totals[k]], [self.counts[k]], sigsq, self._rnorm)[0]
        self.coefs = out
        return out
