"""Per-observation references of the imputation kernels of boom_amd/csrc/probit_kernel.hip, for
tests/test_imputer_ref_cpu.py (which pins them, here, without a GPU) and
tests/test_imputer_kernels_gpu.py (which compares the kernels' output with them).

One function per family gives what the kernel writes for ONE observation from (seed, chain,
sweep, i, n, eta, y, trials / exposure, clt threshold, slot limit):

  probit_obs   BinomialProbitDataImputer::impute, restated here over bo_rnorm, a Python
               restatement of TnSampler on bo_unif / bo_exp_rand (so that it can say how many
               points the hull had at acceptance and how close its comparisons were) and
               ss_logit_oracle.trun_norm_moments;
  logit_obs    ss_logit_oracle.impute_point (not restated);
  poisson_obs  ss_poisson_oracle.impute_parts (not restated), combined in either order;
  pg_obs       a restatement of the oracle's pg_draw, pinned on bo_test_rpg draw for draw (equal
               values, equal stream positions), so that its functions go through the table below
               and its comparisons are under the record.

The tolerance is derived.  Every math function of the restatements -- the wrapped modules'
too: their name `math` is bound to the table while a reference runs -- goes through one small
table (MathTable).  A replay re-runs the observation as another library would compute it:
  * every result of exp, log, log1p, sqrt, tanh, sinh, cosh moved by up to 2 ulp, of erfc by up to
    4 (no statement of the device library's errors is at hand: these are the figures of
    DESIGN 3.8);
  * arithmetic order.  The device's compiler fuses a + b c into one rounding, the host's rounds
    twice: at most one ulp of the result.  The replays move by up to one ulp the results of the
    expressions that can be fused where that ulp is not already inside the 8 ulp of the value:
    runif's a + (b - a) u (a logistic draw next to 1 loses 1 / (1 - u) of it), the adaptive
    rejection sampler's candidate, hull value, knots and truncated exponential, the Poisson
    imputer's delta + exp_rand / exp(eta) under its logarithm and the product of its second
    sum + weight x residual (ss_poisson_oracle asks the table for both), d_rnorm's mu + sigma z of the central-limit draws and the inverse-Gaussian root of the
    Polya-Gamma draw;
  * the Kinderman-Ramage normal itself (evaluated inside the oracle's C code): 4 ulp for the
    outer branches' logarithm and square root, and for the first branch A (c u1 + u2 - 1) the
    ulp of the sum in [1, 2) times A, an ABSOLUTE 4.9e-16 however small the normal
    (MathTable.norm_rand); rbeta's logarithms and exponentials through ss_poisson_oracle's own
    restatement of it.
An observation's bound is 4 x the spread of its outputs over 8 replays + 8 ulp of the value
(bounded()).  What else the oracle's C code evaluates inside itself (exp_rand, rbinom, rmulti)
has no rounding of its own in the result and is taken as it is.

Every run also returns a SIGNATURE -- hull sizes, mixture components / binomial counts through
the exact information, the stream position the draw ended at -- and the smallest margin of the
comparisons it recorded; a replay whose signature differs took another branch."""
import contextlib
import ctypes as C
import functools
import math
import struct
import zlib

import numpy as np

import ss_logit_oracle as slo
import ss_poisson_oracle as spo
from oracle_lib import BoRng, Oracle

PROBIT_STREAM, PROBIT_STRIDE = 8, 4096
PG_STREAM, PG_STRIDE = 10, 4096
LOGIT_STREAM, LOGIT_STRIDE = slo.LOGIT_STREAM, slo.LOGIT_STRIDE
POISSON_STREAM, POISSON_STRIDE = spo.POISSON_STREAM, spo.POISSON_STRIDE
HULL_CAP = 64          # BO_ARS_CAP = TN_BIG_CAP: the largest hull
ULPS = dict(exp=2, log=2, log1p=2, sqrt=2, tanh=2, sinh=2, cosh=2, erfc=4)
FUSED_ULPS, NORM_ULPS, KR_A = 1, 4, 2.216035867166471
REPLAYS = 8


class MathTable:
    """the math functions of the restatements; replay = None: the host's own results, else each
    result moved by a whole number of ulps in [-U, U], a fixed pseudo-random function of the
    replay's number, the function and the result (so one replay is one consistent 'other
    library': the same call gives the same answer wherever it is made)"""

    def __init__(self, replay=None):
        self.rnd = None if replay is None else int(replay)

    def __getattr__(self, name):          # (pi, fabs, floor, ...: the host's)
        return getattr(math, name)

    def nudge(self, name, v, U):
        if self.rnd is None or v == 0.0 or not math.isfinite(v):
            return v
        k = zlib.crc32(struct.pack("<dI", v, self.rnd) + name.encode()) % (2 * U + 1) - U
        return v + k * math.ulp(v)

    def norm_rand(self, z):
        """a Kinderman-Ramage normal as another library gives it: NORM_ULPS ulp of it for the
        outer branches' logarithm and square root, and for the first branch, A (c u1 + u2 - 1)
        with A = 2.216..., the ulp of the sum c u1 + u2 in [1, 2) times A -- fused or not, it is
        rounded there before the 1 is taken off, so the error does not shrink with the normal"""
        if self.rnd is None:
            return z
        z = self.nudge("norm_rand", z, NORM_ULPS)
        j = zlib.crc32(struct.pack("<dI", z, self.rnd) + b"first branch") % 5 - 2
        return z + j * (0.5 * KR_A * 2.0 ** -52)

    def fma(self, a, b, c):
        """a * b + c as the host computes it: two roundings (Fused: the device's one)"""
        return a * b + c

    def fused(self, v):
        """the result of an expression a + b * c: the device's compiler may round it once
        (a fused multiply-add), the host's rounds it twice -- at most one ulp apart"""
        return self.nudge("fused", v, FUSED_ULPS)


def _nudged(name, U):
    real = getattr(math, name)

    def f(self, x):
        try:
            v = real(x)
        except OverflowError:             # (the C library's answer)
            return math.inf
        return self.nudge(name, v, U)
    f.__name__ = name
    return f


for _name, _U in ULPS.items():
    setattr(MathTable, _name, _nudged(_name, _U))
HOST = MathTable()


class Fused(MathTable):
    """the host's functions with a * b + c rounded ONCE at the sites named in `sites` -- what the
    device's compiler makes of the same expressions when it contracts them.  For finding which
    expression a disagreement comes from (tests/test_imputer_ref_cpu.py), not a reference"""

    def __init__(self, sites):
        MathTable.__init__(self)
        self.sites = frozenset(sites)

    def at(self, site):
        return _Site(self, site in self.sites)


class _Site:
    def __init__(self, M, on):
        self.M, self.on = M, on

    def fma(self, a, b, c):
        if not self.on:
            return a * b + c
        from fractions import Fraction
        if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
            return a * b + c
        return float(Fraction(a) * Fraction(b) + Fraction(c))


def _at(M, site):
    return M.at(site) if isinstance(M, Fused) else M


class _ReplayLib:
    """the oracle's library as a replay sees it.  Three of its primitives hold arithmetic the
    device does in its own way, out of the math table's sight:
      bo_runif   a + (b - a) u, an expression the device may fuse: one ulp;
      bo_rnorm   mu + sigma norm_rand(): the normal as MathTable.norm_rand moves it, then the same
                 fusable expression;
      bo_test_rbeta_a1   logarithms and exponentials: ss_poisson_oracle's own restatement of it,
                 whose functions are the table's.
    Everything else (bo_unif, bo_exp_rand, bo_rmulti, bo_test_rbinom, ...) is the library's."""

    def __init__(self, L, M):
        self._L, self._M = L, M

    def __getattr__(self, name):
        return getattr(self._L, name)

    def bo_runif(self, rng, a, b):
        if a == b:
            return a
        return self._M.fused(a + (b - a) * self._L.bo_unif(rng))

    def bo_rnorm(self, rng, mu, sigma):
        if sigma == 0.0:
            return mu
        z = self._M.norm_rand(self._L.bo_norm_rand(rng))
        if mu == 0.0 and sigma == 1.0:        # (the rejection loop's plain normal: nothing to fuse)
            return z
        return self._M.fused(mu + sigma * z)

    def bo_test_rbeta_a1(self, rng, aa):
        return spo.rbeta_a1_margin(self._L, rng._obj, aa)[0]   # (rng: a byref)


def _lib(M):
    L = oracle().lib
    return L if M.rnd is None else _ReplayLib(L, M)


@contextlib.contextmanager
def _table(M):
    """the wrapped restatements' `math` is the table while the block runs"""
    saved = slo.math, spo.math
    slo.math = spo.math = M
    try:
        yield
    finally:
        slo.math, spo.math = saved


@functools.lru_cache(maxsize=None)
def oracle():
    o = Oracle()
    L = o.lib
    slo.declare(L)
    spo.declare(L)
    L.bo_norm_rand.argtypes = [C.c_void_p]
    L.bo_rtrun_norm.restype = C.c_double
    L.bo_rtrun_norm.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int)]
    L.bo_test_rpg.restype = C.c_double
    L.bo_test_rpg.argtypes = [C.c_void_p, C.c_long, C.c_double, C.c_long, C.POINTER(C.c_int)]
    return o


def slot_rng(seed, chain, stream, stride, index, slot_limit=0):
    """slot `index` of the chain's stream, serving `slot_limit` uniforms before its spill stream"""
    L = oracle().lib
    rng = BoRng()
    L.bo_rng_seed_philox(C.byref(rng), int(seed), int(chain), int(stream), 0)
    L.bo_set_slot_limit(int(slot_limit))
    try:
        L.bo_rng_slot(C.byref(rng), int(index), int(stride))
    finally:
        L.bo_set_slot_limit(0)
    return rng


def _where(rng):
    return int(rng.stream), int(rng.pos)


_gap = spo._gap
_copy = spo._copy


class Overflow(Exception):
    """a hull of more than 64 points (the oracle: BO_ERR_UNSUPPORTED_RNG_BRANCH)"""


class Degenerate(Exception):
    """the hull's integrals are not finite numbers (a candidate beyond 1e150): the uniform falls
    behind the last of them, where the reference reads past its arrays"""


class Trace:
    def __init__(self):
        self.margin, self.hulls, self.arms = np.inf, [], set()

    def see(self, a, b):
        self.margin = min(self.margin, _gap(a, b))


# ---- TnSampler (distributions/trun_norm.cpp:108-241), after oracle/boom_oracle.c tn_draw ----
def _lower_bound(v, n, value, tr):
    first, count = 0, n
    while count > 0:
        step = count // 2
        tr.see(v[first + step], value)
        if v[first + step] < value:
            first += step + 1
            count -= step + 1
        else:
            count = step
    return first


def _rtrun_exp(L, M, rng, lam, lo, hi, tr):
    slope = -lam
    tr.margin = min(tr.margin, abs(abs(hi - lo) - 1e-7))
    if abs(hi - lo) < 1e-7:
        return lo
    u, eps = 0.0, 2.2250738585072014e-308
    while u < eps or u >= 1.0 - eps:
        u = L.bo_runif(C.byref(rng), 0.0, 1.0)
    F = _at(M, "trun_exp")
    x = M.fused(F.fma(slope, hi, M.log(u)))
    y = M.fused(F.fma(slope, lo, M.log(1 - u)))
    if x < y:
        x, y = y, x
    return (x + M.log1p(M.exp(y - x))) / slope


def tn_draw(L, M, rng, a, tr):
    """a standard normal given x > a, a > 0; the hull size at acceptance goes to tr.hulls"""
    xs, ys, ds, kn = [a], [-.5 * a * a], [-a], [a]
    for _level in range(1002):
        n = len(xs)
        cdf, last, y0 = [], 0.0, ys[0]
        for k in range(n):                                  # update_cdf
            d, y, z = ds[k], ys[k] - y0, xs[k]
            dinv = 1.0 / d
            F = _at(M, "integral")
            inc1 = 0 if k == n - 1 else dinv * M.exp(F.fma(d, kn[k + 1], F.fma(-d, z, y)))
            inc2 = dinv * M.exp(F.fma(d, kn[k], F.fma(-d, z, y)))
            last = last + inc1 - inc2
            cdf.append(last)
        u = L.bo_runif(C.byref(rng), 0.0, cdf[n - 1])
        k = _lower_bound(cdf, n, u, tr)
        if k >= n:
            raise Degenerate()
        if k + 1 == n:
            cand = M.fused(_at(M, "candidate").fma(1.0 / (-1 * ds[n - 1]), L.bo_exp_rand(C.byref(rng)), kn[n - 1]))
        else:
            cand = _rtrun_exp(L, M, rng, -1 * ds[k], kn[k], kn[k + 1], tr)
        target = -.5 * cand * cand
        hull = M.fused(_at(M, "hull").fma(ds[k], cand - xs[k], ys[k]))
        logu = hull - (1.0 / 1.0) * L.bo_exp_rand(C.byref(rng))
        tr.see(logu, target)
        if logu < target:
            tr.hulls.append(n)
            return cand
        if n >= HULL_CAP:
            tr.hulls.append(n + 1)
            raise Overflow()
        pos = _lower_bound(kn, n, cand, tr)
        xs.insert(pos, cand)
        ys.insert(pos, -.5 * cand * cand)
        ds.insert(pos, -cand)
        kn.append(0.0)
        kn[0] = xs[0]                                       # ars_refresh
        for j in range(1, n + 1):
            if ds[j] == ds[j - 1]:
                kn[j] = xs[j - 1]
            else:
                F = _at(M, "knot")
                kn[j] = (M.fused(F.fma(-ds[j - 1], xs[j - 1], ys[j - 1])) - M.fused(F.fma(-ds[j], xs[j], ys[j]))) / (ds[j] - ds[j - 1])
    raise Overflow()


def trun_norm_std(L, M, rng, a, tr):
    if a <= 0:
        while True:
            x = L.bo_rnorm(C.byref(rng), 0.0, 1.0)
            tr.see(x, a)
            if x > a:
                return x
    return tn_draw(L, M, rng, a, tr)


def rtrun_norm(L, M, rng, mu, sigma, a, gt, tr):
    """rtrun_norm_mt(rng, mu, sigma, a, gt), trun_norm.cpp:36-47"""
    if gt:
        return mu + sigma * trun_norm_std(L, M, rng, (a - mu) / sigma, tr)
    return mu - sigma * trun_norm_std(L, M, rng, (mu - a) / sigma, tr)


class Obs:
    """one observation's reference: out (name -> value), the signature of its branches, the
    smallest recorded margin, and what the family counts"""

    def __init__(self, out, sig, margin, status=0, **facts):
        self.out, self.sig, self.margin, self.status, self.facts = out, sig, margin, status, facts


def probit_route(seed, chain, sweep, i, n, eta, y, nt, clt, slot_limit=0):
    """which way phase (1) of probit_impute_kernel sends the observation"""
    nt, y = int(round(nt)), int(round(y))
    far = (0 < y <= clt and eta < 0.0) or (0 < nt - y <= clt and eta > 0.0)
    if far:
        return "far"
    serve = slot_limit if 0 < slot_limit < PROBIT_STRIDE else PROBIT_STRIDE
    if nt != 1 or clt < 1 or serve < 2:
        return "queued"
    L = oracle().lib
    rng = slot_rng(seed, chain, PROBIT_STREAM, PROBIT_STRIDE, sweep * n + i, slot_limit)
    u1 = L.bo_unif(C.byref(rng))
    if not u1 < 0.884070402298758:
        return "miss_u1"
    u2 = L.bo_unif(C.byref(rng))
    x = 2.216035867166471 * (1.131131635444180 * u1 + u2 - 1)
    cut = 0.0 - eta if y == 1 else eta - 0.0
    return "hit" if x > cut else "miss_cut"


def probit_obs(seed, chain, sweep, i, n, eta, y, nt, clt, slot_limit=0, M=HOST):
    """BinomialProbitDataImputer::impute (BinomialProbitDataImputer.cpp:30-73): z"""
    L = _lib(M)
    nt, y, eta = int(round(nt)), int(round(y)), float(eta)
    rng = slot_rng(seed, chain, PROBIT_STREAM, PROBIT_STRIDE, sweep * n + i, slot_limit)
    tr, ans = Trace(), 0.0
    try:
        with _table(M):
            if y > clt:
                mean, variance = slo.trun_norm_moments(eta, 1.0, 0.0, True)
                ans += L.bo_rnorm(C.byref(rng), y * mean, M.sqrt(y * variance))
            else:
                for _ in range(y):
                    ans += rtrun_norm(L, M, rng, eta, 1.0, 0.0, True, tr)
            if nt - y > clt:
                mean, variance = slo.trun_norm_moments(eta, 1.0, 0.0, False)
                ans += L.bo_rnorm(C.byref(rng), (nt - y) * mean, M.sqrt((nt - y) * variance))
            else:
                for _ in range(nt - y):
                    ans += rtrun_norm(L, M, rng, eta, 1.0, 0.0, False, tr)
    except Overflow:
        return Obs({}, ("overflow",), tr.margin, status="rng_branch", hulls=tr.hulls)
    return Obs(dict(z=ans), (tuple(tr.hulls), _where(rng)), tr.margin, hulls=tr.hulls)


def _ss_out(total, info):
    return dict(value=total / info, w=info, h=1.0 / info)


def logit_obs(seed, chain, sweep, i, n, eta, y, nt, clt, slot_limit=0, M=HOST, ss=False):
    """BinomialLogitCltDataImputer::impute: (z, w), or the state space family's (value, w, h)"""
    L = _lib(M)
    rng = slot_rng(seed, chain, LOGIT_STREAM, LOGIT_STRIDE, sweep * n + i, slot_limit)
    rec = slo.Record()
    with _table(M):
        total, info = slo.impute_point(L, rng, nt, y, float(eta), int(clt), rec)
    out = _ss_out(total, info) if ss else dict(z=total, w=info)
    return Obs(out, (info, rec.btpe, _where(rng)), rec.margin, btpe=rec.btpe)


def logit_binomial_facts(seed, chain, sweep, i, n, eta, y, nt, clt):
    """what the large-sample branch's binomial draws were: (inversion draws, BTPE draws, draws with
    pp > 0.5, early returns of rmultinom on an empty remainder) -- by watching ss_logit_oracle's
    rbinom and rmultinom during one more run"""
    facts = dict(inversion=0, btpe=0, pp_high=0, early=0)
    real_rbinom, real_rmultinom = slo.rbinom, slo.rmultinom

    def rbinom(L, rng, nn, pp, rec):
        p = pp if pp < 1.0 - pp else 1.0 - pp
        facts["btpe" if nn * p >= 30 else "inversion"] += 1
        facts["pp_high"] += pp > 0.5
        return real_rbinom(L, rng, nn, pp, rec)

    def rmultinom(L, rng, nn, prob, rec):
        rN = real_rmultinom(L, rng, nn, prob, rec)
        # (rN[K - 1] is set only when the loop ran to its end with something left)
        facts["early"] += nn > 0 and rN[-1] == 0 and sum(rN) == nn
        return rN
    slo.rbinom, slo.rmultinom = rbinom, rmultinom
    try:
        logit_obs(seed, chain, sweep, i, n, eta, y, nt, clt)
    finally:
        slo.rbinom, slo.rmultinom = real_rbinom, real_rmultinom
    return facts


def pg_moments(M, nt, eta):
    """the large-sample arm's mean and variance (oracle/boom_oracle.c pg_draw)"""
    az = abs(eta)
    if az < 1e-4:
        return nt * (0.25 - az * az / 48.0), nt * (1.0 / 24.0 - az * az / 120.0)
    th, ch = M.tanh(0.5 * az), M.cosh(0.5 * az)
    return nt * th / (2 * az), nt * (M.sinh(az) - az) / (4 * az * az * az * ch * ch)


PG_T, PG_PI = 0.64, 3.14159265358979323846


def _pg_a(M, n, x):
    K = (n + 0.5) * PG_PI
    if x > PG_T:
        return K * M.exp(-0.5 * K * K * x)
    return M.exp(-1.5 * (M.log(0.5 * PG_PI) + M.log(x)) + M.log(K) - 2.0 * (n + 0.5) * (n + 0.5) / x)


def _pg_rtigauss(L, M, r, z, tr):
    t = PG_T
    X = t + 1.0
    tr.arms.add("tigauss_exp" if z < 1.0 / t else "tigauss_normal")
    if z < 1.0 / t:
        alpha = 0.0
        while True:
            u = L.bo_unif(r)
            tr.see(u, alpha)
            if not u > alpha:
                break
            E1, E2 = L.bo_exp_rand(r), L.bo_exp_rand(r)
            while E1 * E1 > 2 * E2 / t:
                E1, E2 = L.bo_exp_rand(r), L.bo_exp_rand(r)
            X = 1 + E1 * t
            X = t / (X * X)
            alpha = M.exp(-0.5 * z * z * X)
    else:
        mu = 1.0 / z
        while X > t:
            Y = M.norm_rand(L.bo_norm_rand(r))
            Y *= Y
            half_mu, mu_Y = 0.5 * mu, mu * Y
            X = M.fused(M.fused(mu + half_mu * mu_Y) - half_mu * M.sqrt(M.fused(4 * mu_Y + mu_Y * mu_Y)))
            u, edge = L.bo_unif(r), mu / (mu + X)
            tr.see(u, edge)
            if u > edge:
                X = mu * mu / X
            tr.see(X, t)
    return X


def pg_draw1(L, M, r, z, tr):
    """PG(1, z) after oracle/boom_oracle.c pg_draw1 (pinned on bo_test_rpg), its functions the
    table's and its comparisons under the record"""
    z = abs(z) * 0.5
    t = PG_T
    fz = 0.125 * PG_PI * PG_PI + 0.5 * z * z
    for _tries in range(10000):
        b, a = M.sqrt(1.0 / t) * (t * z - 1), -1.0 * M.sqrt(1.0 / t) * (t * z + 1)
        x0 = M.log(fz) + fz * t
        xb = x0 - z + M.log(0.5 * M.erfc(-b / 1.4142135623730951))
        xa = x0 + z + M.log(0.5 * M.erfc(-a / 1.4142135623730951))
        qdivp = 4 / PG_PI * (M.exp(xb) + M.exp(xa))
        u, edge = L.bo_unif(r), 1.0 / (1.0 + qdivp)
        tr.see(u, edge)
        if u < edge:
            tr.arms.add("tail")
            X = M.fused(t + L.bo_exp_rand(r) / fz)
        else:
            X = _pg_rtigauss(L, M, r, z, tr)
        S = _pg_a(M, 0, X)
        Y = L.bo_unif(r) * S
        n = 0
        while True:
            n += 1
            if n & 1:
                S -= _pg_a(M, n, X)
                tr.see(Y, S)
                if Y <= S:
                    return 0.25 * X
            else:
                S += _pg_a(M, n, X)
                tr.see(Y, S)
                if Y > S:
                    break
            assert n <= 1000
    raise AssertionError("pg_draw1 gave up")


def pg_obs(seed, chain, sweep, i, n, eta, y, nt, clt, slot_limit=0, M=HOST):
    """omega ~ PG(nt, eta) and kappa = y - nt / 2: (z, w)"""
    L = _lib(M)
    nt, y, eta = int(round(nt)), int(round(y)), float(eta)
    rng = slot_rng(seed, chain, PG_STREAM, PG_STRIDE, sweep * n + i, slot_limit)
    tr = Trace()
    if nt > clt:
        mean, var = pg_moments(M, nt, eta)
        omega = L.bo_rnorm(C.byref(rng), mean, M.sqrt(var))
        tr.see(omega, 0.0)
        if not omega > 0:
            omega = mean
        arm = "series" if abs(eta) < 1e-4 else "moments"
    else:
        omega = 0.0
        for _ in range(nt):
            omega += pg_draw1(L, M, C.byref(rng), eta, tr)
        arm = "sum"
    return Obs(dict(z=float(y) - 0.5 * float(nt), w=omega), (arm, _where(rng)), tr.margin, arm=arm, arms=tr.arms)


def poisson_obs(seed, chain, sweep, i, n, eta, y, exposure, mixtures, slot_limit=0, M=HOST, ss=False):
    """PoissonDataImputer::impute: (z, w) with the internal point added first, or the state space
    family's (value, w, h) with the external point first"""
    L = _lib(M)
    rng = slot_rng(seed, chain, POISSON_STREAM, POISSON_STRIDE, sweep * n + i, slot_limit)
    with _table(M):
        if ss:
            v, q, margin = spo.impute_point(L, rng, mixtures, y, float(exposure), float(eta))
            out, info = dict(value=v, w=q, h=1.0 / q), q
        else:
            (z_ext, mu_e, sig_e), internal, margin = spo.impute_parts(L, rng, mixtures, y, float(exposure), float(eta))
            total, info = 0.0, 0.0
            if internal is not None:
                z_int, mu_i, sig_i = internal
                w = 1.0 / sig_i
                total += w * (z_int - mu_i)
                info += w
            w = 1.0 / sig_e
            # (sum + weight x residual, fusable on the device: at |eta| = 700 the two products are
            # 350 and cancel to 14, and the product's ulp is four of the sum's)
            total += M.fused(w * (z_ext - mu_e))
            info += w
            out = dict(z=total, w=info)
    return Obs(out, (info, _where(rng)), margin)


def bounded(fn, *args, **kw):
    """the observation by `fn` on the host's functions, with each output's bound (4 x the spread
    over REPLAYS replays + 8 ulp of the value) and whether every replay took the same branches:
    (Obs, {name: bound}, same)"""
    base = fn(*args, **kw)
    lo = dict(base.out)
    hi = dict(base.out)
    same = True
    first = True
    for k in range(REPLAYS):
        r = fn(*args, M=MathTable(k), **kw)
        if r.sig != base.sig or r.status != base.status:
            same = False
            continue
        for name, v in r.out.items():
            lo[name] = v if first else min(lo[name], v)
            hi[name] = v if first else max(hi[name], v)
        first = False
    bound = {name: 4.0 * (hi[name] - lo[name]) + 8.0 * float(np.spacing(abs(v))) for name, v in base.out.items()}
    return base, bound, same


def eta_of(X, gamma, beta):
    """x_i'beta over the included columns in ascending order, one rounded product and one rounded
    sum per column (the tests' X and beta make every partial sum exact)"""
    eta = np.zeros(X.shape[0])
    for j in np.flatnonzero(gamma):
        eta = eta + X[:, j] * beta[j]
    return eta


# ---- the cases of tests/test_imputer_kernels_gpu.py ---------------------------------------------
# A case is a dict of what the probe takes (kind, n, p, X, gamma, beta, y, nt, ...); reference()
# gives every chain's expected outputs, bounds and status from it.  Unless a case says otherwise:
# 3 chains, chain c includes column c alone with coefficient 1 (eta = X[:, c], exact),
# chain_offset 5 (the oracle's chain is 5 + c), sweep 3.
CHAINS, CHAIN_OFFSET, SWEEP, SEED = 3, 5, 3, 20260419
OK, RNG_BRANCH, FORECAST_VARIANCE, MODEL_TOO_LARGE = 0, 4, 5, 6      # ssvs_params.h (the probe says the same)
KMAX = 1024
SIZES = (1, 255, 256, 257, 513)
KINDS = ("probit", "logit", "logit_ss", "pg", "poisson", "poisson_ss")
OUTPUTS = dict(probit=("z",), logit=("z", "w"), pg=("z", "w"), poisson=("z", "w"),
               logit_ss=("value", "w", "h"), poisson_ss=("value", "w", "h"))
MISSING_VARIANCE = dict(logit_ss=slo.MISSING_VARIANCE, poisson_ss=spo.MISSING_VARIANCE)

# (trials, successes): one trial; only successes / only failures / both below the threshold 5;
# one kind above it and the other below; both above; no trial at all
PROBIT_OBS = [(1, 1), (1, 0), (3, 3), (3, 0), (4, 2), (9, 9), (9, 0), (12, 6), (8, 2), (8, 7), (0, 0)]
PROBIT_ETA = [0.3, -0.3, 1.2, -1.2, 2.5, -2.5, 5.0, -5.0, 1e-3, -1e-3, 30.0, -30.0, 0.0]
# trials 1 .. clt with no, every and some successes; clt + 1, 60 and 1000 trials with ys = 0, nt, between
LOGIT_OBS = [(1, 0), (1, 1), (2, 0), (2, 2), (2, 1), (3, 1), (4, 4), (5, 2), (5, 0), (5, 5), (6, 0), (6, 6), (6, 3),
             (60, 0), (60, 60), (60, 25), (1000, 0), (1000, 1000), (1000, 400)]
LOGIT_ETA = [0.0, 1e-3, -1e-3, 3.0, -3.0, 20.0, -20.0]
PG_OBS = [(1, 0), (1, 1), (3, 2), (5, 5), (6, 3), (40, 11), (1000, 999)]
PG_ETA = [0.0, 1.0, -1.0, 3.125, -3.125, 3.2, -3.2, 20.0, -20.0, 5e-5, -5e-5, 2e-4, -2e-4, 3.0, -3.0]
POISSON_ETA = [0.0, 5.0, -5.0, 599.0, -599.0, 601.0, -601.0, 700.0, -700.0]
POISSON_EXPOSURE = [1.0, 0.25, 40.0]


@functools.lru_cache(maxsize=None)
def poisson_table():
    """the mixtures of the fixture tests/test_poisson_gpu.py loads, as a table that ends at its
    last count: (dict for Mixtures, counts y of the cases: 0, 1, inside, the last, one beyond)"""
    from golden_lib import _golden_mix, load
    mix = dict(_golden_mix(load("poisson_exposure")))
    last = int(mix["counts"][-1])
    mix["largest_index"] = last + 1
    return mix, [0, 1, 7, last, last + 1]


def _crossed(n, obs, etas, shift):
    """observation i: obs[i % A]; chain c's eta: etas[(i // A + i + shift c) % B] -- every pair
    of the two lists within A B observations (A + 1 and B have no common factor)"""
    A, B = len(obs), len(etas)
    assert math.gcd(A + 1, B) == 1
    idx = np.arange(n)
    eta = np.array([[etas[(i // A + i + shift * c) % B] for i in idx] for c in range(CHAINS)])
    return [obs[i % A] for i in idx], eta


def _base(kind, n, eta, y, nt, clt=5, **more):
    """the default model: column c is chain c's eta, included alone with coefficient 1"""
    case = dict(kind=kind, n=n, p=CHAINS, chains=CHAINS, chain_offset=CHAIN_OFFSET, sweep=SWEEP, seed=SEED,
                clt=clt, slot_limit=0, X=np.ascontiguousarray(np.asarray(eta, float).T),
                gamma=np.eye(CHAINS, dtype=np.uint8), beta=np.eye(CHAINS), y=np.asarray(y, float),
                nt=np.asarray(nt, float), status0=np.zeros(CHAINS, np.int32), overflow_ok=False)
    if kind.endswith("_ss"):
        rs = np.random.RandomState(n + 17)
        stride = n + 5
        case.update(observed=(np.arange(n) % 7 != 3).astype(np.uint8), offset_stride=stride,
                    offset=np.round(rs.uniform(-0.5, 0.5, (CHAINS, stride)) * 1024) / 1024)
    if kind.startswith("poisson"):
        mix, _ = poisson_table()
        M = spo.Mixtures(mix)
        case["obs_mix"] = np.array([-1 if (v <= 0 or v >= M.largest) else int(np.searchsorted(M.counts, v))
                                    for v in case["y"].astype(np.int64)], np.int32)
    case.update(more)
    return case


def table_case(kind, n, **more):
    """the family's table of edge observations, n of them"""
    fam = kind.split("_")[0]
    if fam == "probit":
        obs, eta = _crossed(n, PROBIT_OBS, PROBIT_ETA, 4)
    elif fam == "logit":
        obs, eta = _crossed(n, LOGIT_OBS, LOGIT_ETA, 2)
    elif fam == "pg":
        obs, eta = _crossed(n, PG_OBS, PG_ETA, 4)
    else:
        _, counts = poisson_table()
        pairs = [(ex, y) for y in counts for ex in POISSON_EXPOSURE]
        obs, eta = _crossed(n, pairs, POISSON_ETA, 2)
    nt, y = zip(*obs)
    if kind.endswith("_ss"):
        # (the state space families' eta is offset + x'beta: the table's eta is the sum)
        case = _base(kind, n, eta, y, nt, **more)
        case["X"] = np.ascontiguousarray((eta - case["offset"][:, :n]).T)
        return case
    return _base(kind, n, eta, y, nt, **more)


def _obs_of(case, c, i, eta, M=HOST):
    kind = case["kind"]
    args = (case["seed"], case["chain_offset"] + c, case["sweep"], i, case["n"], eta, case["y"][i], case["nt"][i])
    if kind == "probit":
        return probit_obs(*args, case["clt"], case["slot_limit"], M=M)
    if kind in ("logit", "logit_ss"):
        return logit_obs(*args, case["clt"], case["slot_limit"], M=M, ss=kind == "logit_ss")
    if kind == "pg":
        return pg_obs(*args, case["clt"], case["slot_limit"], M=M)
    return poisson_obs(*args, spo.Mixtures(poisson_table()[0]), case["slot_limit"], M=M, ss=kind == "poisson_ss")


def case_eta(case, c):
    """chain c's linear predictor as the kernel forms it"""
    eta = eta_of(case["X"], case["gamma"][c], case["beta"][c])
    if case["kind"].endswith("_ss"):
        eta = case["offset"][c, :case["n"]] + eta
    return eta


def reference(case):
    """what the kernel must leave: want[name], bound[name] (chains x n; NaN: not written), the
    written mask, status (chains), and per observation the branch facts"""
    kind, n, chains = case["kind"], case["n"], case["chains"]
    names = OUTPUTS[kind]
    want = {k: np.full((chains, n), np.nan) for k in names}
    bound = {k: np.zeros((chains, n)) for k in names}
    written = np.zeros((chains, n), bool)
    status = case["status0"].copy()
    exact = np.zeros((chains, n), bool)        # missing steps: bit for bit
    loose = np.zeros((chains, n))              # +-1: only the sign of what is written is defined
    same, margin, facts, routes = True, np.inf, [], []
    for c in range(chains):
        if status[c] != OK:
            continue
        if int(case["gamma"][c].sum()) > KMAX:
            status[c] = MODEL_TOO_LARGE
            continue
        eta = case_eta(case, c)
        for i in range(n):
            if kind.endswith("_ss") and not case["observed"][i]:
                want["value"][c, i], want["w"][c, i], want["h"][c, i] = 0.0, 0.0, MISSING_VARIANCE[kind]
                written[c, i] = exact[c, i] = True
                continue
            base, bnd, ok = bounded(lambda M=HOST: _obs_of(case, c, i, float(eta[i]), M))
            if not ok and i < case.get("unstable", 0) and base.status == 0:
                # (see probit_cases, tiny24: no value to compare with; the draw's side is defined)
                loose[c, i] = 1.0 if case["y"][i] else -1.0
                facts.append((c, i, base))
                routes.append("far")
                continue
            same, margin = same and ok, min(margin, base.margin)
            facts.append((c, i, base))
            if kind == "probit":
                routes.append(probit_route(case["seed"], case["chain_offset"] + c, case["sweep"], i, n, float(eta[i]),
                                           case["y"][i], case["nt"][i], case["clt"], case["slot_limit"]))
            if base.status == "rng_branch":
                status[c] = RNG_BRANCH
                continue                        # (the kernel writes the truncation point there: no reference)
            written[c, i] = True
            for k in names:
                want[k][c, i], bound[k][c, i] = base.out[k], bnd[k]
    return dict(want=want, bound=bound, written=written, exact=exact, loose=loose, status=status, same=same,
                margin=margin, facts=facts, routes=routes)


def _model_case(kind, included):
    """p = 1100; every chain includes `included` (ascending) with its own coefficients; X and beta
    are small multiples of 2^-8 and 2^-6, so every product and partial sum is exact in any order"""
    n, p = 40, 1100
    case = table_case(kind, n)
    rs = np.random.RandomState(len(included))
    X = rs.randint(-256, 257, (n, p)) / 256.0
    gamma = np.zeros((CHAINS, p), np.uint8)
    gamma[:, included] = 1
    beta = np.zeros((CHAINS, p))
    k = len(included)
    for c in range(CHAINS):
        # (coefficients that keep |eta| modest whatever the number of columns)
        beta[c, included] = rs.randint(-8, 9, k) / (64.0 * max(1, k // 16))
    # (a coefficient outside the model must not be read: give the excluded ones a value that would show)
    beta[gamma == 0] = 1000.0
    case.update(p=p, X=X, gamma=gamma, beta=beta)
    if kind.endswith("_ss"):
        case["offset"] = np.round(case["offset"] * 4) / 4
    return case


COLUMNS8 = [0, 63, 64, 255, 256, 511, 512, 1099]


def model_case(kind, which):
    """which = 8: the eight columns at the lanes', waves' and rounds' edges; 1024: exactly KMAX
    columns; 1025: one too many (chain 1 only: the others keep eight)"""
    if which == 8:
        return _model_case(kind, COLUMNS8)
    keep = [j for j in range(1100) if j % 15 != 7]          # 1100 - 73 = 1027 columns
    if which == 1024:
        return _model_case(kind, keep[:500] + keep[503:])
    case = _model_case(kind, COLUMNS8)
    case["gamma"][1, :] = 0
    case["gamma"][1, keep[:1025]] = 1
    case["beta"][1, keep[:1025]] = 0.015625
    return case


def crossing_case(kind):
    """sweep n + i passes 2^32 inside the case"""
    n = 513
    sweep = (1 << 32) // n
    assert sweep * n < (1 << 32) <= sweep * n + n - 1
    return table_case(kind, n, sweep=sweep)


def parked_case(kind):
    """chain 1 is not CHAIN_OK at entry: nothing of it is written, its status stays"""
    case = table_case(kind, 257)
    case["status0"][1] = FORECAST_VARIANCE
    return case


def probit_cases():
    """the probit kernel's scheduling edges: name -> case"""
    n = 256
    cases = {}
    # 256 near-side observations of several trials: wave 0 takes a second chunk
    obs = [PROBIT_OBS[2 + i % 8] for i in range(n)]
    nt, y = zip(*obs)

    def near_sign(i):
        # successes drawn one by one want eta >= 0, failures drawn one by one eta <= 0
        up, down = 0 < y[i] <= 5, 0 < nt[i] - y[i] <= 5
        return 0.0 if up and down else 1.0 if up else -1.0 if down else (1.0 if i % 2 else -1.0)
    eta = np.array([[near_sign(i) * (0.25 + 0.015625 * (i % 50)) * (c + 1) for i in range(n)] for c in range(CHAINS)])
    cases["near256"] = _base("probit", n, eta, y, nt)
    # 256 far-side observations: the queue is walked in four rounds
    y = [i % 2 for i in range(n)]
    eta = np.array([[-(0.1 + 0.02 * (i % 97) + 0.5 * c) * (1 if y[i] else -1) for i in range(n)] for c in range(CHAINS)])
    cases["far256"] = _base("probit", n, eta, y, [1] * n)
    # 24 one-trial observations a hair on the far side (hulls of 17 .. 64 points: phase (3), more
    # than 4 of them) among near-side ones
    n = 100
    y = [i % 2 for i in range(n)]
    tiny = [1e-12, 1e-13, 1e-14, 1e-15]
    eta = np.array([[(-1 if y[i] else 1) * (tiny[(i + c) % 4] if i < 24 else -(0.3 + 0.01 * i))
                     for i in range(n)] for c in range(CHAINS)])
    # The VALUES of these 24 have no reference.  Wherever a hull passes 16 points the truncation
    # point is 1e-9 or closer to the mean, the first candidates are 1 / a large, and the knots and
    # the hull's integrals are differences of numbers 1 / a^2 large: one ulp in a knot moves an
    # exponent by tens, so which segment the next uniform falls in depends on how a - b c was
    # rounded (the device fuses it, the host does not).  Under the replays' ulps 37 % of such
    # observations change their branches at a = 1e-9, 86 % at 1e-10 and all at 1e-12, whatever the
    # seed.  reference() marks those whose replays disagree `loose`: the kernel must write a
    # finite draw on the side of zero the outcome says, leave the status alone and every other
    # observation of the workgroup exact.  An EXTRA case: phase (3)'s values are compared in
    # phase3_case, at cuts where a reference exists.
    cases["tiny24"] = _base("probit", n, eta, y, [1] * n, unstable=24)
    for clt in (0, 5):
        cases["clt%d" % clt] = table_case("probit", 150, clt=clt)
    for limit in (1, 2, 6):
        cases["slot%d" % limit] = table_case("probit", 150, slot_limit=limit)
    return cases


# (chain -> {observation: a}): one-trial observations of the workgroup below whose cut is
# a = 2e-10 .. 1e-9 on the far side, whose hull needs 17 to 19 points and whose branches are the
# same in every replay with margins above 1e-9 -- found by trying a = 1e-9, 3e-10 (chain 1 also
# 5e-10, 2e-10) at every observation; about one in twenty-five qualifies, the rest change a branch
# under the replays' ulps.  tests/test_imputer_ref_cpu.py asserts all of it again.
PHASE3 = {0: {7: 1e-9, 54: 1e-9, 63: 1e-9, 87: 3e-10, 90: 3e-10, 106: 3e-10, 122: 1e-9, 127: 3e-10, 141: 1e-9,
              150: 1e-9, 174: 3e-10},
          1: {1: 1e-9, 6: 3e-10, 71: 2e-10, 80: 1e-9, 85: 5e-10, 98: 2e-10, 101: 2e-10, 103: 1e-9, 139: 5e-10,
              170: 1e-9, 181: 3e-10, 186: 3e-10},
          2: {35: 1e-9, 38: 1e-9, 54: 1e-9, 68: 1e-9, 77: 3e-10, 86: 1e-9, 110: 1e-9, 117: 1e-9, 133: 1e-9,
              168: 3e-10, 169: 1e-9, 192: 3e-10}}


def phase3_case():
    """one workgroup of 256 far-side one-trial observations: those of PHASE3 a hair on the far
    side (their hulls outgrow 16 points: redone in phase (3) with 64-point hulls, four at a time,
    in three rounds or more), the others at ordinary eta.  Every one is compared by value"""
    n = 256
    y = [i % 2 for i in range(n)]
    eta = np.array([[(-1 if y[i] else 1) * PHASE3[c].get(i, 0.1 + 0.02 * (i % 97) + 0.5 * c) for i in range(n)]
                    for c in range(CHAINS)])
    return _base("probit", n, eta, y, [1] * n)


@functools.lru_cache(maxsize=None)
def overflow_search(values=(1e-16, 1e-18, 1e-20, 1e-25, 1e-30, 1e-35), slots=8):
    """one-trial observations of chain CHAIN_OFFSET + 1, n = 64, at a = 1e-16 and below for which
    the oracle's bo_rtrun_norm reports BO_ERR_UNSUPPORTED_RNG_BRANCH -- a hull of more than 64
    points: (those that meet the conditions of a case -- the same branches in every replay --,
    those whose hull is degenerate)"""
    L = oracle().lib
    usable, degenerate = [], []
    for a in values:
        for i in range(slots):
            rng = slot_rng(SEED, CHAIN_OFFSET + 1, PROBIT_STREAM, PROBIT_STRIDE, SWEEP * 64 + i)
            st = C.c_int(0)
            L.bo_rtrun_norm(C.byref(rng), -a, 1.0, 0.0, 1, C.byref(st))
            if st.value == 0:
                continue
            try:
                base, _, same = bounded(probit_obs, SEED, CHAIN_OFFSET + 1, SWEEP, i, 64, -a, 1, 1, 5)
            except Degenerate:
                degenerate.append((a, i))
                continue
            if base.status == "rng_branch" and same:
                usable.append((a, i))
    return usable, degenerate


def overflow_case():
    """chain 1 holds ONE observation whose hull outgrows 64 points (the first the search finds
    that every replay agrees on); the rest is the table"""
    usable, _ = overflow_search()
    a, at = usable[0]
    case = table_case("probit", 64)
    case["y"], case["nt"], case["X"] = case["y"].copy(), case["nt"].copy(), case["X"].copy()
    case["y"][at], case["nt"][at] = 1.0, 1.0
    case["X"][at, 1] = -a
    return case


def case_names():
    names = []
    for kind in KINDS:
        names += ["%s-n%d" % (kind, n) for n in SIZES]
        names += ["%s-%s" % (kind, what) for what in ("crossing", "parked", "model8", "model1024", "model1025")]
    names += ["probit-%s" % what for what in ("near256", "far256", "phase3", "tiny24", "clt0", "clt5", "slot1", "slot2", "slot6",
                                              "overflow")]
    return names


@functools.lru_cache(maxsize=None)
def case_of(name):
    kind, what = name.split("-")
    if what.startswith("model"):
        return model_case(kind, int(what[5:]))
    if what[0] == "n" and what[1:].isdigit():
        return table_case(kind, int(what[1:]))
    if what == "crossing":
        return crossing_case(kind)
    if what == "parked":
        return parked_case(kind)
    if what == "overflow":
        return overflow_case()
    if what == "phase3":
        return phase3_case()
    return probit_cases()[what]


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """the case's reference, computed once and shared (nothing may change it)"""
    return reference(case_of(name))
