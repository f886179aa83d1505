"""Restatement of the observation families' forecasts (ba_ss_student_forecast, ba_ss_poisson_forecast,
ba_ss_logit_forecast) in plain Python over the oracle's primitives (bo_unif, bo_norm_rand / bo_rnorm,
bo_rgamma on rng_philox(seed, chain, 5)):

  advance     one forecast step of the state for static intercept, local level, local linear trend
              and seasonal blocks (bo_ssm_forecast_model's step: ssm_state_error, ssm_T, the sum)
  forecast    the horizon's loop with the family's observation draw
  rstudent    rstudent_mt: w = rgamma(nu / 2, rate nu / 2), then rnorm(mu, sigma / sqrt(w))
  rpois, rbinom   the exact count samplers AS THE DEVICE HAS THEM (boom_amd/csrc/device_rng_counts.h:
              inversion by sequential search below a mean of 10, Hoermann's PTRS / BTRS above), the same
              operations in the same order

A count draw also reports how close its decisions were: Draw.margin is the smallest |lhs - rhs| over the
comparisons that decided it -- u against the accumulated probabilities, the squeeze and range tests, the
log acceptance test, and the distance of a floor's argument from the nearest integer -- and Draw.term
the largest |term| that entered those comparisons.  A draw is CLOSE when margin < max(1e-9, 1e-12 term):
the device forms the same quantities with its own exp / log / lgamma and fused multiply-adds, a few ulps
from these, so only a close draw may come out differently there.
"""
import ctypes as C
import math

import numpy as np

KIND_LOCAL_LEVEL, KIND_LOCAL_LINEAR_TREND, KIND_SEASONAL, KIND_STATIC_INTERCEPT = 1, 2, 3, 5
SEARCH_CAP, REJECT_CAP = 128, 256    # RCOUNT_SEARCH_CAP, RCOUNT_REJECT_CAP
INF = float("inf")


class Stream:
    """a Philox stream of the oracle, read through its primitives"""

    def __init__(self, oracle, seed, chain, stream=5, pos=0):
        self.lib = oracle.lib
        self.lib.bo_rnorm.restype = C.c_double
        self.lib.bo_rnorm.argtypes = [C.c_void_p, C.c_double, C.c_double]
        self.rng = oracle.rng_philox(seed, chain, stream, pos)
        self.ref = C.byref(self.rng)

    @property
    def pos(self):
        return int(self.rng.pos)

    def unif(self):
        return self.lib.bo_unif(self.ref)

    def norm_rand(self):
        return self.lib.bo_norm_rand(self.ref)

    def rnorm(self, mu, sigma):
        return self.lib.bo_rnorm(self.ref, mu, sigma)

    def rgamma(self, a, rate):
        st = C.c_int(0)
        x = self.lib.bo_rgamma(self.ref, a, rate, C.byref(st))
        assert st.value == 0
        return x


class Draw:
    __slots__ = ("value", "margin", "term", "branch")

    def __init__(self, value, margin=INF, term=0.0, branch="edge"):
        self.value, self.margin, self.term, self.branch = value, margin, term, branch

    @property
    def close(self):
        return self.margin < max(1e-9, 1e-12 * self.term)


def rstudent(s, mu, sigma, nu):
    w = s.rgamma(nu / 2.0, nu / 2.0)
    return s.rnorm(mu, sigma / math.sqrt(w))


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def plogis(eta):
    """1 / (1 + exp(-eta)): exactly 0 or 1 at large |eta|, NaN only for NaN"""
    return 1.0 / (1.0 + _exp(-eta))


def rpois(s, lam):
    if not (lam >= 0.0) or math.isinf(lam):
        return Draw(math.nan)
    if lam == 0.0:
        return Draw(0.0)
    if lam < 10.0:
        u = s.unif()
        pk = math.exp(-lam)
        cdf = pk
        k = 0
        margin = abs(u - cdf)
        while u > cdf and k < SEARCH_CAP:
            k += 1
            pk *= lam / k
            nxt = cdf + pk
            if nxt == cdf:
                break
            cdf = nxt
            d = abs(u - cdf)
            if d < margin:
                margin = d
        return Draw(float(k), margin, 1.0, "inversion")
    slam, loglam = math.sqrt(lam), math.log(lam)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    inv_alpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    margin, term = INF, 1.0
    for _ in range(REJECT_CAP):
        u = s.unif() - 0.5
        v = s.unif()
        us = 0.5 - abs(u)
        if us == 0.0:
            continue    # (the device: k = floor(-inf) < 0)
        arg = (2.0 * a / us + b) * u + lam + 0.43
        k = math.floor(arg)
        margin = min(margin, arg - k, k + 1.0 - arg, abs(us - 0.07))
        term = max(term, abs(arg))
        if us >= 0.07:
            margin = min(margin, abs(v - vr))
            if v <= vr:
                return Draw(float(k), margin, term, "ptrs")
        margin = min(margin, abs(us - 0.013))
        if us < 0.013:
            margin = min(margin, abs(v - us))
        if k < 0 or (us < 0.013 and v > us):
            continue
        t1, t2, t3 = k * loglam, math.lgamma(k + 1.0), math.log(a / (us * us) + b)
        lhs = (math.log(v) if v > 0.0 else -INF) + math.log(inv_alpha) - t3
        rhs = -lam + t1 - t2
        margin = min(margin, abs(lhs - rhs))
        term = max(term, abs(t1), abs(t2), lam, abs(t3), abs(lhs))
        if lhs <= rhs:
            return Draw(float(k), margin, term, "ptrs")
    return Draw(math.nan, margin, term, "ptrs")


def rbinom(s, n, p):
    n = float(n)
    if not (0.0 <= p <= 1.0) or not (n >= 0.0) or math.isinf(n):
        return Draw(math.nan)
    if n == 0.0 or p == 0.0:
        return Draw(0.0)
    if p == 1.0:
        return Draw(n)
    mirror = p > 0.5
    q = 1.0 - p if mirror else p
    tag = "+mirror" if mirror else ""
    margin, term = INF, 1.0
    if n * q < 10.0:
        u = s.unif()
        odds = q / (1.0 - q)
        pk = math.exp(n * math.log1p(-q))
        cdf = pk
        k = 0.0
        margin = abs(u - cdf)
        while u > cdf and k < n:
            pk *= odds * ((n - k) / (k + 1.0))
            k += 1.0
            nxt = cdf + pk
            if nxt == cdf:
                break
            cdf = nxt
            d = abs(u - cdf)
            if d < margin:
                margin = d
        branch = "inversion"
    else:
        spq = math.sqrt(n * q * (1.0 - q))
        b = 1.15 + 2.53 * spq
        a = -0.0873 + 0.0248 * b + 0.01 * q
        c = n * q + 0.5
        vr = 0.92 - 4.2 / b
        alpha = (2.83 + 5.1 / b) * spq
        m = math.floor((n + 1.0) * q)
        lodds = math.log(q / (1.0 - q))
        h = math.lgamma(m + 1.0) + math.lgamma(n - m + 1.0)
        branch, k = "btrs", None
        for _ in range(REJECT_CAP):
            u = s.unif() - 0.5
            v = s.unif()
            us = 0.5 - abs(u)
            if us == 0.0:
                continue
            arg = (2.0 * a / us + b) * u + c
            kk = float(math.floor(arg))
            margin = min(margin, arg - kk, kk + 1.0 - arg)
            term = max(term, abs(arg))
            if kk < 0.0 or kk > n:
                continue
            margin = min(margin, abs(us - 0.07))
            if us >= 0.07:
                margin = min(margin, abs(v - vr))
                if v <= vr:
                    k = kk
                    break
            t1, t2, t3 = math.lgamma(kk + 1.0), math.lgamma(n - kk + 1.0), (kk - m) * lodds
            lhs = math.log(v * alpha / (a / (us * us) + b)) if v > 0.0 else -INF
            rhs = (h - t1 - t2) + t3
            margin = min(margin, abs(lhs - rhs))
            term = max(term, abs(h), abs(t1), abs(t2), abs(t3), abs(lhs))
            if lhs <= rhs:
                k = kk
                break
        if k is None:
            return Draw(math.nan, margin, term, branch + tag)
    return Draw(n - k if mirror else k, margin, term, branch + tag)


# ---- the state ---------------------------------------------------------------------------------------
def _new_season(blk, t):
    t -= blk["t0"]
    if t < 0:
        t -= blk["duration"] * t
    return t % blk["duration"] == 0


def layout(blocks):
    """first state component of every block, the state dimension"""
    first, m = [], 0
    for b in blocks:
        first.append(m)
        m += b["dim"]
    return first, m


def advance(s, blocks, sigsq, state, tm):
    """state <- T_tm state + the state errors of time tm (every model's errors first, in the list's
    order, as simulate_next_state draws them); sigsq[b]: block b's variances"""
    first, m = layout(blocks)
    eta = np.zeros(m)
    for b, f in zip(range(len(blocks)), first):
        blk, kind = blocks[b], blocks[b]["kind"]
        if kind == KIND_LOCAL_LEVEL:
            eta[f] = s.rnorm(0.0, math.sqrt(sigsq[b][0]))
        elif kind == KIND_LOCAL_LINEAR_TREND:
            z0, z1 = s.rnorm(0.0, 1.0), s.rnorm(0.0, 1.0)
            eta[f] = math.sqrt(sigsq[b][0]) * z0 + 0.0
            eta[f + 1] = math.sqrt(sigsq[b][1]) * z1 + 0.0
        elif kind == KIND_SEASONAL:
            if _new_season(blk, tm + 1):
                eta[f] = s.rnorm(0.0, math.sqrt(sigsq[b][0]))
        elif kind != KIND_STATIC_INTERCEPT:
            raise ValueError("the restatement has no state model of kind %d" % kind)
    st = np.array(state, float)
    for b, f in zip(range(len(blocks)), first):
        blk, kind = blocks[b], blocks[b]["kind"]
        if kind == KIND_LOCAL_LINEAR_TREND:
            st[f] = st[f] + st[f + 1]
        elif kind == KIND_SEASONAL and _new_season(blk, tm + 1):
            n = blk["dim"]
            head = 0.0
            for i in range(n):
                head -= st[f + i]
            st[f + 1:f + n] = st[f:f + n - 1].copy()
            st[f] = head
    return st + eta


def zdot(blocks, state):
    first, _ = layout(blocks)
    ans = state[first[0]]
    for f in first[1:]:
        ans += state[f]
    return ans


def forecast(s, family, T, newX, beta, blocks, sigsq, final_state, sigsq_obs=1.0, nu=None, scale=None):
    """one call of the family's forecast on the stream s (which goes on from call to call).
    family: "gaussian" (the observation line of ba_ss_forecast), "student", "poisson" (scale = exposure),
    "logit" (scale = trials).  Returns the horizon's values and, for the count families, the Draws."""
    h, p = newX.shape
    st = np.array(final_state, float)
    out, draws = np.zeros(h), []
    for i in range(h):
        st = advance(s, blocks, sigsq, st, T - 2 + i)
        zs = zdot(blocks, st)
        pred = 0.0
        for j in range(p):
            pred += newX[i, j] * beta[j]
        if family == "gaussian":
            out[i] = s.rnorm(zs, math.sqrt(sigsq_obs)) + pred
            continue
        eta = zs + pred
        if family == "student":
            out[i] = rstudent(s, eta, math.sqrt(sigsq_obs), nu)
            continue
        if family == "poisson":
            d = rpois(s, (1.0 if scale is None else scale[i]) * _exp(eta))
        else:
            d = rbinom(s, 1.0 if scale is None else float(round_half_away(scale[i])), plogis(eta))
        draws.append(d)
        out[i] = d.value
    return (out, draws) if family in ("poisson", "logit") else out


def round_half_away(x):
    """lround"""
    return math.floor(abs(x) + 0.5) * (1 if x >= 0 else -1)
