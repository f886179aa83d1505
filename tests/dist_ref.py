"""References of the scalar samplers of boom_amd/csrc/device_rng.h and ar_trunc_device.h, for
tests/test_dist_ref_cpu.py (which pins them on the oracle, here, without a GPU) and
tests/test_dist_samplers_gpu.py (which compares the device's draws with them, one by one).

Python restatements over the oracle's bo_unif / bo_exp_rand / bo_norm_rand on a Philox bo_rng of
  rgamma_scale      Bmath/rgamma.cpp (the small-shape sampler, GS, GD)
  rtrun_exp         distributions/trun_exp.cpp (imputer_ref's restatement, not a second one)
  ars_gamma_tail    BoundedAdaptiveRejectionSampler on a gamma's tail
  rtg_slice x 5, rtrun_gamma, and the variance draw around them (sigma_max = 0, infinite, finite)
  tn2_draw / rtrun_norm_2   Tn2Sampler and rtrun_norm_2_mt
Every math function and every expression a + b c that a compiler may fuse goes through
imputer_ref.MathTable, so imputer_ref.bounded() gives each draw its bound: 4 x the spread of the
restatement over 8 replays + 8 ulp of the value.  With replay = None a restatement is the oracle's
own function, bit for bit, with the same stream position and status (test_dist_ref_cpu.py).

Each run returns an imputer_ref.Obs: out = {"x": value}; sig = (the PATH -- algorithm, the arm of
every branch and one entry per round of every loop, hull sizes, the segment drawn from and the
insertion position of every hull round --, (stream id, position) at the end); margin = the
smallest relative gap of a comparison; status = 0, or what the device's *bad says there (1: the
small-shape sampler's 1000 rejections, or the two-sided hull gave up; 2: the gamma tail's hull
gave up -- the cut at the mode, or 64 points); facts: arms (the set of path entries) and where.

A draw whose 8 replays do not all carry the un-nudged run's signature sits on a comparison that
rounding alone decides: it has no reference value and is SET ASIDE (support and status only)."""
import ctypes as C
import functools
import math

import numpy as np

import imputer_ref as ir
import philox_ref as pr
from imputer_ref import HOST, REPLAYS, MathTable, bounded

STREAM, STRIDE = 21, 4096          # a stream id no kernel of the product uses
SEEDS = (20260419, 0x5DEECE66D1234567)
CHAINS = (5, 0xFFFFFFFF)
BAD_SMALL, BAD_TN2, BAD_ARS = 1, 1, 2
ARS_CAP = 64
TN2_CAP_DEVICE = 63                # the device keeps the last knot in lane n: one point fewer
SET_ASIDE_CAP = 0.005
MIN_COMPARED = 16
EXPM1_ULPS = 2


class Bad(Exception):
    def __init__(self, code):
        Exception.__init__(self)
        self.code = code


class Tr(ir.Trace):
    def __init__(self):
        ir.Trace.__init__(self)
        self.path = []

    def arm(self, name):
        self.path.append(name)


def _div(a, b):
    """a / b as C gives it where b is zero (two equal points of a hull)"""
    if b != 0.0:
        return a / b
    if a == 0.0 or a != a:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _expm1(M, x):
    return M.nudge("expm1", math.expm1(x), EXPM1_ULPS)


# ---- Rmath::rgamma_mt(rng, a, scale), after oracle/boom_oracle.c rgamma_scale ------------------
def rgamma_scale(L, M, rng, tr, a, scale):
    R, F = C.byref(rng), M.fused
    q1, q2, q3, q4, q5, q6, q7 = 0.04166669, 0.02083148, 0.00801191, 0.00144121, -7.388e-5, 2.4511e-4, 2.424e-4
    a1, a2, a3, a4, a5, a6, a7 = 0.3333333, -0.250003, 0.2000062, -0.1662921, 0.1423657, -0.1367177, 0.1233795
    if a < .3:
        ee = 2.718281828459045
        w0 = a / (ee * (1 - a))
        r0 = 1.0 / (1 + w0)
        lam = (1.0 / a) - 1.0
        log_w, log_lambda = M.log(w0), M.log(lam)
        for _ in range(1000):
            u0 = L.bo_unif(R)
            tr.see(u0, r0)
            if u0 <= r0:
                tr.arm("small_exp")
                z = -M.log(u0 / r0)
            else:
                tr.arm("small_pow")
                z = M.log(L.bo_unif(R)) / lam
            log_h = -z - M.exp(-z / a)
            log_eta = -z if z >= 0 else F(log_w + log_lambda + lam * z)
            rhs = M.log(L.bo_unif(R)) + log_eta
            tr.see(log_h, rhs)
            if log_h >= rhs:
                return M.exp(-z / a + M.log(scale))
            tr.arm("small_reject")
        raise Bad(BAD_SMALL)
    if a < 1.:                                           # GS
        e = F(1.0 + 0.36787944117144232159 * a)
        while True:
            while True:
                p = e * L.bo_unif(R)
                tr.see(p, 1.0)
                if p >= 1.0:
                    tr.arm("gs_high")
                    x = -M.log((e - p) / a)
                    ex, rhs = L.bo_exp_rand(R), (1.0 - a) * M.log(x)
                else:
                    tr.arm("gs_low")
                    x = M.exp(M.log(p) / a)
                    ex, rhs = L.bo_exp_rand(R), x
                tr.see(ex, rhs)
                if ex >= rhs:
                    break
                tr.arm("gs_reject")
            if x > 0:
                return scale * x
            tr.arm("gs_zero")
    s2 = a - 0.5                                         # GD
    s = M.sqrt(s2)
    d = F(5.656854 - s * 12.0)
    t = M.norm_rand(L.bo_norm_rand(R))
    x = F(s + 0.5 * t)
    ret = x * x
    tr.see(t, 0.0)
    if t >= 0.0:
        tr.arm("gd_immediate")
        return scale * ret
    u = L.bo_unif(R)
    tr.see(d * u, t * t * t)
    if d * u <= t * t * t:
        tr.arm("gd_squeeze")
        return scale * ret
    r = 1.0 / a
    q0 = F(F(F(F(F(F(q7 * r + q6) * r + q5) * r + q4) * r + q3) * r + q2) * r + q1) * r
    if a <= 3.686:
        tr.arm("coef_low")
        b = F(0.463 + s + 0.178 * s2)
        si = 1.235
        c = F(0.195 / s - 0.079 + 0.16 * s)
    elif a <= 13.022:
        tr.arm("coef_mid")
        b = F(1.654 + 0.0076 * s2)
        si = 1.68 / s + 0.275
        c = 0.062 / s + 0.024
    else:
        tr.arm("coef_high")
        b, si, c = 1.77, 0.75, 0.1515 / s

    def q_of(t, where, log1p):
        v = t / (s + s)
        tr.see(abs(v), 0.25)
        if abs(v) <= 0.25:
            tr.arm(where + "_v_small")
            poly = F(F(F(F(F(F(a7 * v + a6) * v + a5) * v + a4) * v + a3) * v + a2) * v + a1)
            return F(q0 + 0.5 * t * t * poly * v)
        tr.arm(where + "_v_large")
        lg = M.log1p(v) if log1p else M.log(1.0 + v)
        return F(F(F(q0 - s * t) + 0.25 * t * t) + (s2 + s2) * lg)
    if x > 0.0:
        q = q_of(t, "quotient", True)
        lhs = M.log(1.0 - u)
        tr.see(lhs, q)
        if lhs <= q:
            tr.arm("gd_quotient")
            return scale * ret
    rounds = 0
    while True:
        rounds += 1
        tr.arm("loop_round")
        e = L.bo_exp_rand(R)
        u = L.bo_unif(R)
        u = u + u - 1.0
        t = F(b - si * e) if u < 0.0 else F(b + si * e)
        tr.see(t, -0.71874483771719)
        if t >= -0.71874483771719:
            q = q_of(t, "loop", False)
            tr.see(q, 0.0)
            if q > 0.0:
                w = _expm1(M, q)
                lhs, rhs = c * abs(u), w * M.exp(F(e - 0.5 * t * t))
                tr.see(lhs, rhs)
                if lhs <= rhs:
                    break
        else:
            tr.arm("loop_retry")
    tr.arm("loop_once" if rounds == 1 else "loop_twice" if rounds == 2 else "loop_three_or_more")
    x = F(s + 0.5 * t)
    return scale * x * x


# ---- rtrun_gamma_mt beyond the mode ------------------------------------------------------------
def _dtl(M, x, a, b, cut):
    """dtrun_gamma(x, a, b, cut, log = true, normalize = false)"""
    if a < 0 or b < 0 or cut < 0 or x < cut:
        return -math.inf
    return M.fused((a - 1) * M.log(x) - b * x)


def ars_gamma_tail(L, M, rng, tr, a, b, cut):
    """BoundedAdaptiveRejectionSampler on [cut, inf), after oracle/boom_oracle.c ars_draw"""
    R, F = C.byref(rng), M.fused
    xs, ys, ds, kn = [cut], [_dtl(M, cut, a, b, cut)], [(a - 1) / cut - b], [cut]
    if ds[0] >= 0:
        tr.arm("ars_at_mode")
        raise Bad(BAD_ARS)
    for _level in range(1002):
        n = len(xs)
        cdf, last, y0 = [], 0.0, ys[0]
        Fi = ir._at(M, "integral")
        for k in range(n):                                  # update_cdf
            d, y, z = ds[k], ys[k] - y0, xs[k]
            dinv = 1.0 / d
            base = F(Fi.fma(-d, z, y))
            inc1 = 0 if k == n - 1 else dinv * M.exp(F(Fi.fma(d, kn[k + 1], base)))
            inc2 = dinv * M.exp(F(Fi.fma(d, kn[k], base)))
            last = last + inc1 - inc2
            cdf.append(last)
        u = L.bo_runif(R, 0.0, cdf[n - 1])
        k = ir._lower_bound(cdf, n, u, tr)
        if k + 1 >= n:
            k = n - 1
            tr.arm(("ars_tail", n))
            cand = F(ir._at(M, "candidate").fma(1.0 / (-1 * ds[k]), L.bo_exp_rand(R), kn[k]))
        else:
            tr.arm(("ars_inner", n, k))
            cand = ir._rtrun_exp(L, M, rng, -1 * ds[k], kn[k], kn[k + 1], tr)
        target = _dtl(M, cand, a, b, cut)
        hull = F(ir._at(M, "hull").fma(ds[k], cand - xs[k], ys[k]))
        logu = hull - (1.0 / 1.0) * L.bo_exp_rand(R)
        tr.see(logu, target)
        if logu <= target:
            tr.hulls.append(n)
            tr.arm("ars_one_point" if n == 1 else "ars_grown")
            return cand
        if n >= ARS_CAP:
            tr.arm("ars_cap")
            raise Bad(BAD_ARS)
        pos = ir._lower_bound(kn, n, cand, tr)
        tr.arm(("ars_insert", pos))
        xs.insert(pos, cand)
        ys.insert(pos, target)
        ds.insert(pos, (a - 1) / cand - b)
        kn.append(0.0)
        kn[0] = xs[0]                                       # refresh_knots
        Fk = ir._at(M, "knot")
        for j in range(1, n + 1):
            if ds[j] == ds[j - 1]:
                kn[j] = xs[j - 1]
            else:
                kn[j] = (F(Fk.fma(-ds[j - 1], xs[j - 1], ys[j - 1])) - F(Fk.fma(-ds[j], xs[j], ys[j]))) / (ds[j] - ds[j - 1])
    raise Bad(BAD_ARS)


def slice_gamma_tail(L, M, rng, tr, a, b, cut):
    """rtg_slice x 5 with its rtg_init (trun_gamma.cpp:110-148): shape <= 1"""
    R = C.byref(rng)
    x = cut
    for _ in range(5):
        logpstar = _dtl(M, x, a, b, cut) - (1.0 / 1.0) * L.bo_exp_rand(R)
        lo, hi = cut, x
        f = _dtl(M, hi, a, b, cut) - logpstar
        fprime = ((a - 1) / hi) - b
        attempts = 0
        root_eps = math.sqrt(2.220446049250313e-16)
        tr.see(f, root_eps)
        while f > root_eps:
            tr.arm("slice_newton")
            hi -= f / fprime
            f = _dtl(M, hi, a, b, cut) - logpstar
            fprime = ((a - 1) / cut) - b
            attempts += 1
            if attempts > 1000:
                tr.arm("slice_newton_gave_up")
                break
            tr.see(f, root_eps)
        x = L.bo_runif(R, lo, hi)
        trials, gave_up = 0, False
        while True:
            fx = _dtl(M, x, a, b, cut)
            tr.see(fx, logpstar)
            if not fx < logpstar:
                break
            tr.arm("slice_shrink")
            hi = x
            x = L.bo_runif(R, lo, hi)
            trials += 1
            if trials > 1000:
                gave_up = True
                break
        if gave_up:
            tr.arm("slice_gave_up")
            x = cut
        elif trials == 0:
            tr.arm("slice_first_point")
    return x


def rtrun_gamma(L, M, rng, tr, a, b, cut):
    """rtrun_gamma_mt(rng, a, b, cut, nslice = 5), trun_gamma.cpp:73-106"""
    mode = (a - 1) / b
    if cut < mode:
        tr.arm("below_mode")
        while True:
            x = rgamma_scale(L, M, rng, tr, a, 1.0 / b)
            tr.see(x, cut)
            if not x < cut:
                return x
            tr.arm("below_mode_reject")
    if a > 1:
        return ars_gamma_tail(L, M, rng, tr, a, b, cut)
    tr.arm("slice")
    return slice_gamma_tail(L, M, rng, tr, a, b, cut)


def draw_variance(L, M, rng, tr, DF, SS, sigma_max):
    """GenericGaussianVarianceSampler::draw"""
    if sigma_max == 0.0:
        tr.arm("sigma_max_zero")
        return 0.0
    a, b = DF / 2, SS / 2
    if math.isinf(sigma_max):
        tr.arm("sigma_max_infinite")
        return _div(1.0, rgamma_scale(L, M, rng, tr, a, 1.0 / b))
    return _div(1.0, rtrun_gamma(L, M, rng, tr, a, b, 1.0 / (sigma_max * sigma_max)))


# ---- Tn2Sampler and rtrun_norm_2_mt, after oracle/boom_oracle.c tn2_draw / bo_rtrun_norm_2 -------
def tn2_draw(L, M, rng, tr, lo, hi, cap=ARS_CAP):
    R, F = C.byref(rng), M.fused
    xs, ys, ds = [lo, hi], [-.5 * lo * lo, -.5 * hi * hi], [-lo, -hi]
    for _level in range(1002):
        n = len(xs)
        kn = [0.0] * (n + 1)
        kn[0], kn[n] = xs[0], xs[n - 1]
        Fk = ir._at(M, "knot")
        for k in range(1, n):
            ans = F(Fk.fma(-ds[k - 1], xs[k - 1], ys[k - 1])) - F(Fk.fma(-ds[k], xs[k], ys[k]))
            kn[k] = _div(ans, ds[k] - ds[k - 1])
        cdf, y0 = [], ys[0]
        Fi = ir._at(M, "integral")
        for k in range(n):
            d = ds[k]
            y = F(Fi.fma(d, kn[k] - xs[k], ys[k]))
            if abs(d) < .00000000001:
                inc = M.exp(y - y0) * (kn[k + 1] - kn[k])
            else:
                inc = (M.exp(y - y0) / d) * _expm1(M, F(Fi.fma(d, kn[k + 1], -kn[k])))
            cdf.append(inc if k == 0 else cdf[k - 1] + inc)
        u = L.bo_runif(R, 0.0, cdf[n - 1])
        k = ir._lower_bound(cdf, n, u, tr)
        if k >= n:
            tr.arm("tn2_past_cdf")
            break
        klo, khi = kn[k], kn[k + 1]
        lam = -1 * ds[k]
        tr.margin = min(tr.margin, abs(abs(khi - klo) - 1.4901161193847656e-08))
        if lam == 0 or abs(khi - klo) < 1.4901161193847656e-08:
            tr.arm(("tn2_uniform", n, k))
            cand = L.bo_runif(R, klo, khi)
        else:
            tr.arm(("tn2_exp", n, k))
            cand = ir._rtrun_exp(L, M, rng, lam, klo, khi, tr)
        target = -.5 * cand * cand
        logu = F(ir._at(M, "hull").fma(ds[k], cand - xs[k], ys[k])) - (1.0 / 1.0) * L.bo_exp_rand(R)
        tr.see(logu, target)
        if logu < target:
            tr.hulls.append(n)
            tr.arm("tn2_two_points" if n == 2 else "tn2_grown")
            return cand
        tr.see(cand, xs[n - 1])
        tr.see(cand, xs[0])
        if cand > xs[n - 1] or cand < xs[0]:
            tr.arm("tn2_left_the_hull")
            break
        if n >= cap:
            tr.arm("tn2_cap")
            break
        pos = ir._lower_bound(xs, n, cand, tr)
        tr.arm(("tn2_insert", pos))
        xs.insert(pos, cand)
        ys.insert(pos, -.5 * cand * cand)
        ds.insert(pos, -cand)
    raise Bad(BAD_TN2)


def rtrun_norm_2(L, M, rng, tr, mu, sigma, lo, hi):
    R, F = C.byref(rng), M.fused
    if lo < mu and hi > mu:
        if (hi - lo) / sigma > .5:
            tr.arm("wide")
            y = lo - 1
            while y < lo or y > hi:
                tr.arm("wide_round")
                y = L.bo_rnorm(R, mu, sigma)
                tr.see(y, lo)
                tr.see(y, hi)
            return y
        tr.arm("narrow")
        ln_sqrt_2pi = 0.918938533204672741780329736406
        phi_mu = -(ln_sqrt_2pi + 0.5 * 0.0 * 0.0 + M.log(sigma))
        phi, u, y = phi_mu, phi_mu + 1, 0
        while u > phi:
            tr.arm("narrow_round")
            y = L.bo_runif(R, lo, hi)
            x = (y - mu) / sigma
            phi = -(F(ln_sqrt_2pi + 0.5 * x * x) + M.log(sigma))
            u = phi_mu - (1.0 / 1.0) * L.bo_exp_rand(R)
            tr.see(u, phi)
        return y
    hi = (hi - mu) / sigma
    lo = (lo - mu) / sigma
    if hi < 0:
        tr.arm("tail_below")
        y = tn2_draw(L, M, rng, tr, -hi, -lo)
        return F(mu - sigma * y)
    tr.arm("tail_above")
    y = tn2_draw(L, M, rng, tr, lo, hi)
    return F(y * sigma + mu)


def _runif(L, M, rng, tr, a, b):
    if a == b:
        tr.arm("runif_point")
    return L.bo_runif(C.byref(rng), a, b)


def _rtrun_exp(L, M, rng, tr, lam, lo, hi):
    tr.arm("trun_exp_point" if abs(hi - lo) < 1e-7 else "trun_exp_draw")
    return ir._rtrun_exp(L, M, rng, lam, lo, hi, tr)


def _norm_rand(L, M, rng, tr):
    return M.norm_rand(L.bo_norm_rand(C.byref(rng)))


def _exp_rand(L, M, rng, tr):
    return L.bo_exp_rand(C.byref(rng))


FUNCS = dict(norm_rand=_norm_rand, exp_rand=_exp_rand, runif=_runif, rtrun_exp=_rtrun_exp, rgamma_scale=rgamma_scale, draw_variance=draw_variance,
             rtrun_norm_2=rtrun_norm_2)
NARGS = dict(exp_rand=0, norm_rand=0, runif=2, random_int=2, rtrun_exp=3, rgamma_scale=2, draw_variance=3,
             rtrun_norm_2=4)


def declare(L):
    L.bo_norm_rand.argtypes = [C.c_void_p]
    L.bo_exp_rand.argtypes = [C.c_void_p]
    L.bo_unif.argtypes = [C.c_void_p]
    L.bo_runif.restype = C.c_double
    L.bo_runif.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_rnorm.restype = C.c_double
    L.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.bo_random_int.restype = C.c_int
    L.bo_random_int.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.bo_rtrun_norm_2.restype = C.c_double
    L.bo_rtrun_norm_2.argtypes = [C.c_void_p] + [C.c_double] * 4 + [C.POINTER(C.c_int)]
    return L


@functools.lru_cache(maxsize=None)
def lib():
    return declare(ir.oracle().lib)


def draw(fn, args, seed, chain, index, slot_limit=0, M=HOST):
    """one draw of `fn` from slot `index` of (seed, chain, STREAM): an imputer_ref.Obs"""
    lib()
    L = ir._lib(M)
    rng = ir.slot_rng(seed, chain, STREAM, STRIDE, index, slot_limit)
    tr, status = Tr(), 0
    try:
        x = FUNCS[fn](L, M, rng, tr, *[float(v) for v in args[:NARGS[fn]]])
    except Bad as e:
        x, status = math.nan, e.code
    where = ir._where(rng)
    return ir.Obs(dict(x=x), (tuple(tr.path), where), tr.margin, status=status, arms=frozenset(tr.path),
                  where=where, path=tuple(tr.path), hull=max(tr.hulls, default=0))


def oracle_draw(fn, args, seed, chain, index, slot_limit=0):
    """the same draw by the oracle's own function: (value, (stream id, position), status != 0)"""
    L = lib()
    rng = ir.slot_rng(seed, chain, STREAM, STRIDE, index, slot_limit)
    R, st = C.byref(rng), C.c_int(0)
    a = [float(v) for v in args]
    if fn == "runif":
        x = L.bo_runif(R, a[0], a[1])
    elif fn == "rgamma_scale":
        x = L.bo_rgamma(R, a[0], 1.0 / a[1], C.byref(st))
    elif fn == "draw_variance":
        DF, SS, sigma_max = a[:3]
        if sigma_max == 0.0:
            x = 0.0
        elif math.isinf(sigma_max):
            x = 1.0 / L.bo_rgamma(R, DF / 2, SS / 2, C.byref(st))
        else:
            x = 1.0 / L.bo_rtrun_gamma(R, DF / 2, SS / 2, 1.0 / (sigma_max * sigma_max), C.byref(st))
    elif fn == "rtrun_norm_2":
        x = L.bo_rtrun_norm_2(R, a[0], a[1], a[2], a[3], C.byref(st))
    elif fn == "random_int":
        x = L.bo_random_int(R, int(a[0]), int(a[1]))
    elif fn == "exp_rand":
        x = L.bo_exp_rand(R)
    elif fn == "norm_rand":
        x = L.bo_norm_rand(R)
    else:
        raise KeyError(fn)
    return x, ir._where(rng), st.value != 0


# ---- the cases -------------------------------------------------------------------------------------
def _below(x):
    return math.nextafter(x, -math.inf)


def _above(x):
    return math.nextafter(x, math.inf)


SHAPES = [0.05, _below(0.3), 0.3, 0.575, 0.999, _below(1.0), 1.0, 1.0000001, 2.0, 3.686, _above(3.686), 5.0,
          13.022, _above(13.022), 25.5, 200.0, 5000.5, 1e6]
# (scale = 1 / b as the oracle's bo_rgamma forms it from the rate b)
SCALES = [1.0 / 1.0, 1.0 / 1e8, 1.0 / 1e-8]


def _case(fn, rows, n, which=0, index0=3, slot_limit=0, listed=(), loose=False):
    """draw i takes rows[i % len(rows)]"""
    args = [tuple(rows[i % len(rows)]) for i in range(n)]
    return dict(fn=fn, args=args, n=n, seed=SEEDS[which % 2], chain=CHAINS[(which // 2) % 2], index0=index0,
                slot_limit=slot_limit, listed=tuple(listed), loose=loose)


def _variance_rows(a, factors, rates=(1e-3, 1e3)):
    """(DF, SS, sigma_max) with the cut at factor x the mode (a - 1) / b"""
    rows = []
    for b in rates:
        for f in factors:
            cut = (a - 1) / b * f
            rows.append((2 * a, 2 * b, 1.0 / math.sqrt(cut)))
    return rows


def _window_rows(width, offsets=(0.1, 3.0, 8.0, 30.0), mu=0.3, sigma=0.75):
    """(mu, sigma, lo, hi): the mean below lo and above hi by the offsets (in sigma), a window `width` sigma wide"""
    rows = []
    for k in offsets:
        rows.append((mu, sigma, mu + k * sigma, mu + (k + width) * sigma))
        rows.append((mu, sigma, mu - (k + width) * sigma, mu - k * sigma))
    return rows


SMALL = ("small_exp", "small_pow", "small_reject")
GS = ("gs_high", "gs_low", "gs_reject")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  `listed`: the path entries the case must reach in at least MIN_COMPARED draws
    that are compared by value (asserted, from the reference alone, by test_dist_ref_cpu.py)"""
    cs = {}
    for j, a in enumerate(SHAPES):
        if a < .3:
            listed = SMALL
        elif a < 1:
            listed = GS
        else:
            listed = ("gd_immediate", "gd_squeeze") + GD_LISTED[a]
        cs["rgamma-%s" % repr(a)] = _case("rgamma_scale", [(a, s) for s in SCALES], 2048, which=j, listed=listed)
    # (the spill stream: three numbers per slot, so every GD draw past the squeeze and every GS draw goes on there)
    cs["rgamma-spill"] = _case("rgamma_scale", [(a, 1.0) for a in (0.05, 0.575, 2.0, 25.5)], 512, which=1, slot_limit=3,
                               listed=("small_exp", "gs_low", "gs_reject", "gd_immediate", "gd_squeeze"))
    # (neighbouring draws -- neighbouring lanes of the per-lane convention -- with different shapes and scales)
    mixed = [(a, SCALES[(j + k) % 3]) for k in range(3) for j, a in enumerate(SHAPES) if a >= .3]
    cs["rgamma-mixed"] = _case("rgamma_scale", mixed, 1000, which=3, listed=("gs_low", "gd_immediate", "loop_round"))
    cs["rgamma-mixed-spill"] = _case("rgamma_scale", mixed, 300, which=2, slot_limit=3, listed=("gs_low", "gd_squeeze"))
    # ---- the variance draw
    cs["variance-zero"] = _case("draw_variance", [(7.0, 3.0, 0.0)], 64, listed=("sigma_max_zero",))
    cs["variance-infinite"] = _case("draw_variance", [(400.0, 37.0, math.inf), (2.0000002, 1e-3, math.inf), (51.0, 4e6, math.inf),
                                                      (1.15, 2.0, math.inf), (0.1, 0.3, math.inf)], 640, which=1,
                                    listed=("sigma_max_infinite", "gd_immediate", "gs_low", "small_exp"))
    cs["variance-below"] = _case("draw_variance", _variance_rows(200.0, (0.5, 0.999)) + _variance_rows(25.5, (0.5, 0.999)), 1024,
                                 which=2, listed=("below_mode", "below_mode_reject"))
    above = (1.0 + 1e-6, 1.01, 2.0, 10.0, 1e3)
    for j, a in enumerate((200.0, 1.0000001, 25.5)):
        cs["variance-above-%s" % repr(a)] = _case("draw_variance", _variance_rows(a, above[1:]), 768, which=j,
                                                  listed=ABOVE_LISTED[a])
        # (the cut 1e-6 above the mode: every hull grows; the reference's replays agree on all of them)
        cs["variance-hair-%s" % repr(a)] = _case("draw_variance", _variance_rows(a, above[:1]), 256, which=j + 1,
                                                 listed=("ars_tail", "ars_grown"))
    # a = 3, b = 1 / 2: the mode is 4 = 1 / 0.5^2 exactly
    cs["variance-at-mode"] = _case("draw_variance", [(6.0, 1.0, 0.5)], 64, which=3, listed=("ars_at_mode",))
    # The slice sampler.  Its Newton start-up takes the slope at the CUT from the second step on: with
    # shape < 1 (log density convex) that slope is the steepest, the steps fall short, and at a small cut
    # they are so short that the 1000 attempts run out (slice_newton_gave_up) -- an exit of the loop, and
    # the reference's.  The upper end so found never lies beyond the root, and for shape 1 the first step
    # lands on it, so the first point drawn is always inside the slice: the shrinking loop and its give-up
    # are not reached by the reference at any input tried (test_dist_ref_cpu.py counts it again).
    cs["variance-slice"] = _case("draw_variance", [(2 * a, 2.0, sm) for a in (1.0, 0.5, 0.005) for sm in (30.0, 0.03)], 144,
                                 which=1, listed=("slice", "slice_newton", "slice_newton_gave_up", "slice_first_point"))
    cs["variance-spill"] = _case("draw_variance", _variance_rows(25.5, (2.0,)) + [(1.0, 2.0, 0.5), (400.0, 37.0, 0.35)], 256,
                                 which=2, slot_limit=2, listed=("ars_one_point", "slice", "below_mode"))
    # ---- the two-sided truncated normal
    cs["tn2-wide"] = _case("rtrun_norm_2", [(0.3, 0.75, -0.2, 0.4), (0.3, 0.75, 0.29, 0.3 + 0.376), (-2.0, 1.5, -30.0, 40.0)], 768,
                           listed=("wide", "wide_round"))
    cs["tn2-narrow"] = _case("rtrun_norm_2", [(0.3, 0.75, 0.2, 0.5), (0.3, 0.75, 0.3 - 1e-9, 0.3 + 1e-3), (5.0, 2.0, 4.5, 5.5)], 768,
                             which=1, listed=("narrow", "narrow_round"))
    for j, (tag, width) in enumerate((("1", 1.0), ("1e-3", 1e-3), ("1e-6", 1e-6))):
        cs["tn2-tail-%s" % tag] = _case("rtrun_norm_2", _window_rows(width), 1024, which=j, listed=TAIL_LISTED[tag])
    # A window 1e-9 sigma wide.  At 0.1 sigma from the mean the knot between the two points is nearer than
    # sqrt(epsilon) to both ends and the candidate is uniform (tn2_uniform): compared in full.  At 3 and 8
    # sigma the knot is the quotient of two differences of numbers x^2 / 2 large that agree in all but
    # their last bits -- the reference's own hull is rounding noise there, as imputer_ref's probit-tiny24:
    # the replays disagree on every such draw, half the case's (at 30 sigma they agree again).  Those are checked for support and status only
    # (loose: the set-aside cap does not apply); the rest of the case is compared in full.
    cs["tn2-tail-1e-9"] = _case("rtrun_norm_2", _window_rows(1e-9), 512, which=3, listed=("tn2_uniform", "tn2_two_points"),
                                loose=True)
    cs["tn2-spill"] = _case("rtrun_norm_2", _window_rows(1.0, (0.1, 3.0)) + [(0.3, 0.75, 0.2, 0.5)], 256, which=2, slot_limit=2,
                            listed=("tail_above", "tail_below", "narrow"))
    # ---- the smaller ones
    gap = 1e-7
    rows = [(2.0, 1.0, 1.0 + _below(gap)), (2.0, 0.0, _below(gap)), (2.0, 0.0, _above(gap)), (2.0, 1.0, 1.0 + 2 * gap)]
    rows += [(lam, 0.5, 1.5) for lam in (1e-8, 1e-4, 1.0, 30.0, 700.0)] + [(3.5, -200.0, 0.0), (1e-8 / 3e-7, 0.0, 3e-7)]
    cs["trun_exp"] = _case("rtrun_exp", rows, 1100, which=1, listed=("trun_exp_point", "trun_exp_draw"))
    # (d_rtrun_exp, d_runif and d_random_int read one number: no slot limit the oracle has sends them to the spill stream)
    cs["norm_rand-spill"] = _case("norm_rand", [()], 256, which=2, slot_limit=1)
    cs["exp_rand-spill"] = _case("exp_rand", [()], 256, which=3, slot_limit=1)
    # d_runif(a, a) reads no number.  The other rows keep both ends on one side of zero (either order): the
    # replays' model of a fused a + (b - a) u is one ulp of the RESULT, which holds where the sum does not
    # cancel; between ends of opposite sign a draw next to zero differs between the fused and the
    # twice-rounded form by an ulp of the product, however small the draw (imputer_ref says the same of its
    # logistic draw next to 1).
    cs["runif"] = _case("runif", [(0.25, 0.25), (3.0, 7.5), (-1e300, -1.5e300), (0.0, 1e-300), (-0.0, 0.0), (7.5, 3.0)], 384,
                        listed=("runif_point",))
    return cs


# What else each shape of GD reaches in at least MIN_COMPARED of its 2048 draws, from the reference's
# own counts (test_dist_ref_cpu.py asserts every entry).  The quotient test (|v| = |t| / 2 s with t a
# negative normal that failed the squeeze) meets |v| <= 0.25 in 16 draws or more only from shape 13.03
# on and |v| > 0.25 only up to there; the rejection loop takes 12 % of the draws at shape 1, 4 % at 3.686, under 2 % from 13 on
# and 13 draws of 2048 at shape 200, so its rarer arms (three rounds or more, the retry at
# t < -0.71874) are listed where the loop is common: shapes 1 to 3.686.
_LOOP = ("loop_round", "loop_v_small")
_LOW = ("coef_low", "gd_quotient", "quotient_v_large", "loop_v_large", "loop_three_or_more") + _LOOP
GD_LISTED = {1.0: _LOW + ("loop_once", "loop_retry"), 1.0000001: _LOW + ("loop_once", "loop_retry"),
             2.0: _LOW + ("loop_once", "loop_retry"), 3.686: _LOW,
             _above(3.686): ("coef_mid", "quotient_v_large", "loop_once", "loop_v_large") + _LOOP,
             5.0: ("coef_mid", "quotient_v_large", "loop_once", "loop_v_large") + _LOOP,
             13.022: ("coef_mid", "quotient_v_large", "loop_once") + _LOOP,
             _above(13.022): ("coef_high", "quotient_v_small", "quotient_v_large", "loop_once", "loop_v_large") + _LOOP,
             25.5: ("coef_high", "quotient_v_small", "loop_once") + _LOOP,
             200.0: (), 5000.5: (), 1e6: ()}
ABOVE_LISTED = {200.0: ("ars_tail", "ars_inner", "ars_grown", "ars_one_point"),
                1.0000001: ("ars_tail", "ars_one_point"),
                25.5: ("ars_tail", "ars_inner", "ars_grown", "ars_one_point")}
TAIL_LISTED = {"1": ("tail_above", "tail_below", "tn2_exp", "tn2_grown", "tn2_two_points"),
               "1e-3": ("tail_above", "tail_below", "tn2_exp", "tn2_two_points"),
               "1e-6": ("tail_above", "tail_below", "tn2_two_points")}

INT_ROWS = [(0, 0), (7, 7), (0, 1), (0, 2 ** 30), (-5, -5), (-9, -2), (-(2 ** 31), -(2 ** 31) + 3), (-3, 4), (2 ** 31 - 5, 2 ** 31 - 2)]
CHAINED_N = 2 ** 18
CHAINED = dict(norm_rand=(SEEDS[0], CHAINS[1], 12345), exp_rand=(SEEDS[1], CHAINS[0], 2 ** 33 + 1))   # (seed, chain, first position)


def arm_names(path):
    """the names a path reaches: plain entries, and the first word of the tuples (hull rounds)"""
    return {p if isinstance(p, str) else p[0] for p in path}


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """the case's reference, computed once and shared (nothing may change it): per draw the value,
    its bound, whether it is compared by value, the status, (stream id, position), the set of
    names its path reaches and the smallest margin"""
    case = cases()[name]
    n = case["n"]
    want, bound = np.full(n, np.nan), np.zeros(n)
    same, status = np.zeros(n, bool), np.zeros(n, np.int64)
    stream, pos, arms, margin = np.zeros(n, np.uint64), np.zeros(n, np.uint64), [], np.full(n, np.inf)
    hull = np.zeros(n, np.int64)
    for i in range(n):
        base, bnd, ok = bounded(draw, case["fn"], case["args"][i], case["seed"], case["chain"], case["index0"] + i,
                                case["slot_limit"])
        want[i], bound[i], same[i], status[i] = base.out["x"], bnd["x"], ok, base.status
        stream[i], pos[i] = base.facts["where"]
        arms.append(arm_names(base.facts["path"]))
        margin[i], hull[i] = base.margin, base.facts["hull"]
    return dict(want=want, bound=bound, same=same, status=status, stream=stream, pos=pos, arms=arms, margin=margin,
                hull=hull)


def reached(name):
    """{path entry: the number of draws compared by value that reach it}"""
    ref = ref_of(name)
    counts = {}
    for i, names in enumerate(ref["arms"]):
        if ref["same"][i] and ref["status"][i] == 0 or names & {"ars_at_mode", "ars_cap"}:
            for a in names:
                counts[a] = counts.get(a, 0) + 1
    return counts


def serve_of(case):
    s = case["slot_limit"]
    return s if 0 < s < STRIDE else STRIDE


# ---- chained draws: 2^18 consecutive draws of one stream (d_norm_rand, d_exp_rand) --------------
@functools.lru_cache(maxsize=None)
def chained_ref(fn):
    """(values, the position after every draw) of CHAINED_N consecutive draws by the oracle"""
    L = lib()
    seed, chain, pos0 = CHAINED[fn]
    rng = ir.BoRng()
    L.bo_rng_seed_philox(C.byref(rng), int(seed), int(chain), STREAM, int(pos0))
    f = L.bo_norm_rand if fn == "norm_rand" else L.bo_exp_rand
    R = C.byref(rng)
    x, pos = np.zeros(CHAINED_N), np.zeros(CHAINED_N, np.uint64)
    for i in range(CHAINED_N):
        x[i] = f(R)
        pos[i] = rng.pos
    return x, pos


def chained_first_uniforms(fn):
    """the first uniform of every chained draw, and how many numbers the draw consumed"""
    seed, chain, pos0 = CHAINED[fn]
    _, pos = chained_ref(fn)
    start = np.concatenate([[np.uint64(pos0)], pos[:-1]])
    return pr.uniforms(seed, chain, STREAM, start), (pos - start).astype(np.int64)


def norm_rand_branches():
    """{branch of d_norm_rand: draws}, from the first uniform and the numbers consumed"""
    u1, used = chained_first_uniforms("norm_rand")
    first = u1 < 0.884070402298758
    tail = u1 >= 0.973310954173898
    r3 = ~tail & (u1 >= 0.958720824790463)
    r2 = ~tail & ~r3 & (u1 >= 0.911312780288703)
    r1 = ~first & ~tail & ~r3 & ~r2
    out = {"first": int(first.sum())}
    for name, m in (("tail", tail), ("region 3", r3), ("region 2", r2), ("region 1", r1)):
        out[name] = int(m.sum())
        out[name + ", a second round"] = int((m & (used > 3)).sum())
    out["tail, positive"] = int((tail & (u1 < 0.986655477086949)).sum())
    out["tail, negative"] = int((tail & (u1 >= 0.986655477086949)).sum())
    return out


def exp_rand_branches():
    u1, used = chained_first_uniforms("exp_rand")
    return {"at once": int((used == 1).sum()), "minimum of uniforms": int((used >= 3).sum()),
            "four numbers or more": int((used >= 4).sum()), "doubled": int((u1 <= 0.5).sum()),
            "doubled ten times": int((u1 <= 2.0 ** -10).sum())}


@functools.lru_cache(maxsize=None)
def norm_rand_bound():
    """the bound of every chained normal: 4 x the spread of MathTable.norm_rand over the replays +
    8 ulp (the normal is evaluated inside the oracle; imputer_ref says what a replay does to it)"""
    x, _ = chained_ref("norm_rand")
    lo, hi = x.copy(), x.copy()
    for k in range(REPLAYS):
        M = MathTable(k)
        r = np.array([M.norm_rand(float(v)) for v in x])
        lo, hi = (r, r.copy()) if k == 0 else (np.minimum(lo, r), np.maximum(hi, r))
    return 4.0 * (hi - lo) + 8.0 * np.spacing(np.abs(x))
