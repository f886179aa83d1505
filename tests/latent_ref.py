"""Per-observation references of the Student, quantile and multinomial logit latent-data kernels
(boom_amd/csrc/student_kernel.hip, quantile_kernel.hip, mlogit_kernel.hip), for
tests/test_latent_ref_cpu.py (which pins them, here, without a GPU) and
tests/test_latent_kernels_gpu.py (which compares the kernels' output with them).  The machinery is
tests/imputer_ref.py's -- MathTable, Fused, the replay library, bounded(), slot_rng --, imported.

One function per kernel gives what it writes for ONE observation, or for one chain in the case of
student_sigma_nu_kernel and the weighted sum of squares:

  student_obs     delta = (y - eta) / sigma, w ~ Gamma((nu + 1) / 2, rate (nu + delta^2) / 2) by
                  dist_ref.rgamma_scale (the oracle's bo_rgamma bit for bit on the host's functions,
                  tests/test_dist_ref_cpu.py) from the observation's slot, as
                  student_oracle.StudentOracle.impute and ss_student_oracle do; z = w y, or the state
                  space family's H_t;
  quantile_obs    quantile_oracle.impute_point, passed an inverse-Gaussian draw on the table (the
                  oracle's own root, the same arithmetic) so that the root's functions are the table's
                  and its comparison is under the record; then the kernel's rule for a draw that is
                  not a positive finite number (QUANTILE_WEIGHT_ERROR, w = z = 0);
  mlogit_obs      mlogit_oracle.impute_point (not restated; it takes the table as its math functions);
  sigma_nu_chain  wsse, dist_ref.draw_variance, u and student_oracle.slice_draw_nu on a log density
                  whose functions are the table's (pinned on student_oracle.nu_log_post).

Bound per value: as in imputer_ref, 4 x the spread over 8 replays + 8 ulp.  The replays move math
functions by imputer_ref.ULPS and the fusable expressions by one ulp; the sites new here are
nu + delta * delta, 1 + t + sqrt(t (2 + t)), w * yi - shift, the unmix exponent, every step of
eta's running sum after the first, the slice sampler's candidate lo + (hi - lo) u, and the two
multiply-adds of the slice target.  Two things have no entry in imputer_ref.ULPS:
  * lgamma: LGAMMA_ULPS ulp (the figure imputer_ref gives erfc, its other special function) of
    max(|value|, 1) -- lgamma crosses zero at 1 and 2, where a library's error is an ulp of the
    terms it adds, not of their sum;
  * a sum over the observations (wsse, the slice target's sum of log1p): the workgroup adds in its
    own order, the reference with np.sum.  A replay moves the sum by up to (n + 2 t) u Sum|term| in
    either direction, u = 2^-53: the bound of any summation order, and t ulp for what a term itself
    may differ by (LOG1P_TERM_ULPS, WSSE_TERM_ULPS below, derived where they stand).

Every run returns a signature -- the gamma sampler's path / the branch of rig's root test / every
unmix component / the slice sampler's doublings and shrinks, and the final stream position -- and
its smallest comparison margin.  An observation whose replays do not all carry the signature of
the un-nudged run has no reference value: it is LOOSE (finiteness, sign and status only)."""
import ctypes as C
import functools
import math
import struct
import zlib

import numpy as np

import dist_ref as dr
import imputer_ref as ir
import mlogit_oracle as mo
import quantile_oracle as qo
import student_oracle as so
from imputer_ref import HOST, MathTable, Obs, bounded, slot_rng

STUDENT_STREAM, STUDENT_STRIDE = so.IMPUTE_STREAM, so.IMPUTE_STRIDE
SN_STREAM, SN_STRIDE = so.SN_STREAM, so.SN_STRIDE
QUANTILE_STREAM, QUANTILE_STRIDE = qo.IMPUTE_STREAM, qo.IMPUTE_STRIDE
MLOGIT_STREAM, MLOGIT_STRIDE = mo.IMPUTE_STREAM, mo.IMPUTE_STRIDE
OK, RNG_BRANCH, FORECAST_VARIANCE, MODEL_TOO_LARGE = ir.OK, ir.RNG_BRANCH, ir.FORECAST_VARIANCE, ir.MODEL_TOO_LARGE
SLICE_ERROR, QUANTILE_WEIGHT_ERROR, MLOGIT_IMPUTE_ERROR, BAD_WEIGHT = 9, 10, 11, 13   # (the probe says the same)
STATUS = dict(rng_branch=RNG_BRANCH, slice_error=SLICE_ERROR, weight_error=QUANTILE_WEIGHT_ERROR,
              impute_error=MLOGIT_IMPUTE_ERROR, bad_weight=BAD_WEIGHT)
KMAX, MAX_CHOICES = 1024, 16
ACC_COUNT, ACC_SIGSQ, ACC_SIGSQ2 = 16, 1, 2
LGAMMA_ULPS = ir.ULPS["erfc"]       # (imputer_ref's figure for its other special function; the docstring)
UNIT = 2.0 ** -53
# what a term of a sum may differ by between the kernel and the reference, in ulp of the term:
#   log1p(u / nu): the function itself by imputer_ref.ULPS["log1p"]; its argument by 2 -- the kernel
#     rounds 1 / nu and the product (half an ulp each), the reference the quotient (half an ulp), and
#     log1p's relative sensitivity to its argument is at most 1;
#   w (r r): the same two rounded products on both sides unless the kernel's last one is fused into
#     the running sum, which takes one rounding (half an ulp) away: 1;
#   w (u u) of the weighted sum of squares: two rounded products in the kernel, (w u) u -- two
#     others -- in the reference's numpy: half an ulp each, 2.
LOG1P_TERM_ULPS = ir.ULPS["log1p"] + 2
WSSE_TERM_ULPS = 1
WSS_TERM_ULPS = 2
LOOSE_CAP = 0.01
SEED, CHAIN_OFFSET, SWEEP = ir.SEED, ir.CHAIN_OFFSET, ir.SWEEP
SIZES = (1, 255, 256, 257, 513)


def _L(M):
    dr.lib()                                   # (declares the primitives' argument types)
    return ir._lib(M)


def _lgamma(M, x):
    v = math.lgamma(x)
    scale = max(abs(v), 1.0)
    return v + (M.nudge("lgamma", scale, LGAMMA_ULPS) - scale)


def moved_sum(M, name, terms, term_ulps=0):
    """np.sum(terms); a replay moves it by -1, -1/2, 0, 1/2 or 1 times (n + 2 term_ulps) u Sum|term|
    (an ulp is 2 u)"""
    terms = np.asarray(terms, float)
    s = float(np.sum(terms))
    if M.rnd is None or not math.isfinite(s):
        return s
    k = zlib.crc32(struct.pack("<dI", s, M.rnd) + name.encode()) % 5 - 2
    return s + 0.5 * k * (terms.size + 2 * term_ulps) * UNIT * float(np.sum(np.abs(terms)))


def eta_rows(case, c, M=HOST):
    """chain c's linear predictor for every row of X as the kernel forms it: a running sum over the
    included columns in ascending order; a replay moves every step after the first (a fused
    multiply-add on the device) by an ulp, unless the case's products and sums are exact"""
    X, b = case["X"], case["beta"][c]
    eta = np.zeros(X.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for k, j in enumerate(np.flatnonzero(case["gamma"][c])):
            eta = eta + X[:, j] * b[j]
            if k and M.rnd is not None and not case.get("exact_eta"):
                eta = np.array([M.fused(float(v)) for v in eta])
    return eta


# ---- Student ---------------------------------------------------------------------------------------
def h_of(w, sigsq, nu):
    """the state space family's H_t and which of the rule's three exits gave it"""
    if w > 0.0:
        return sigsq / w, "weight"
    if nu > 2:
        return sigsq * nu / (nu - 2), "marginal"
    return sigsq * 1e8, "floor"


def student_obs(seed, chain, sweep, i, n, eta, y, sigsq, nu, slot_limit=0, M=HOST, ss=False, offset=0.0,
                observed=True):
    """TDataImputer::impute: (w, z), or the state space family's (w, h); a missing step of the
    latter reads no number"""
    if ss and not observed:
        h, exit_ = h_of(0.0, sigsq, nu)
        return Obs({("w", 0): 0.0, ("h", 0): h}, ("missing", exit_), math.inf, exact=True, exit=exit_, where=None)
    L = _L(M)
    yi = y - offset if ss else y
    delta = (yi - eta) / M.sqrt(sigsq)
    rate2 = M.fused(nu + delta * delta)
    rng = slot_rng(seed, chain, STUDENT_STREAM, STUDENT_STRIDE, sweep * n + i, slot_limit)
    tr = dr.Tr()
    try:
        w = dr.rgamma_scale(L, M, rng, tr, 0.5 * (nu + 1), 1.0 / (0.5 * rate2))
    except dr.Bad:
        return Obs({}, ("bad",), tr.margin, status="rng_branch", exact=False, exit=None, where=ir._where(rng))
    where = ir._where(rng)
    if not ss:
        return Obs({("w", 0): w, ("z", 0): w * yi}, (tuple(tr.path), where), tr.margin, exact=False, exit=None,
                   where=where, rate=0.5 * rate2)
    h, exit_ = h_of(w, sigsq, nu)
    status = 0 if (w >= 0.0 and math.isfinite(w)) else "bad_weight"
    return Obs({("w", 0): w, ("h", 0): h}, (tuple(tr.path), exit_, where), tr.margin, status=status, exact=False,
               exit=exit_, where=where, rate=0.5 * rate2)


# ---- quantile -------------------------------------------------------------------------------------
def quantile_obs(seed, chain, sweep, i, n, eta, y, shift, slot_limit=0, M=HOST):
    """QuantileRegressionImputeWorker::impute_latent_data_point: (w, z)"""
    L = _L(M)
    rng = slot_rng(seed, chain, QUANTILE_STREAM, QUANTILE_STRIDE, sweep * n + i, slot_limit)
    rec = dict(branch="none", margin=math.inf, t=0.0)

    def rig(mu, lam, zn, u, root=None):
        """quantile_oracle.rig with smaller_root, on the table's functions"""
        with np.errstate(all="ignore"):
            t = float(mu) * (zn * zn) / (2 * lam)
            x = float(mu) / M.fused(1 + t + M.sqrt(t * (2 + t)))
            edge = float(mu) / (float(mu) + x)
            rec.update(margin=ir._gap(u, edge), t=t, branch="larger" if u > edge else "smaller")
            if u > edge:
                x = np.float64(mu) * np.float64(mu) / np.float64(x)
        return x
    w, _, _ = qo.impute_point(y, eta, shift, lambda: M.norm_rand(L.bo_norm_rand(C.byref(rng))),
                              lambda: L.bo_unif(C.byref(rng)), rig=rig)
    where = ir._where(rng)
    if rec["branch"] == "none":
        return Obs({("w", 0): 0.0, ("z", 0): 0.0}, ("none", where), math.inf, exact=True, branch="none", where=where)
    if not (w > 0.0 and math.isfinite(w)):
        # (the kernel's rule: a draw that is no positive finite number is an error, w = z = 0)
        return Obs({("w", 0): 0.0, ("z", 0): 0.0}, (rec["branch"], "error", where), rec["margin"], status="weight_error",
                   exact=True, branch=rec["branch"], where=where, t=rec["t"])
    return Obs({("w", 0): w, ("z", 0): M.fused(w * y - shift)}, (rec["branch"], where), rec["margin"], exact=False,
               branch=rec["branch"], where=where, t=rec["t"])


# ---- multinomial logit ----------------------------------------------------------------------------
def mlogit_obs(seed, chain, sweep, i, n, eta, y, slot_limit=0, M=HOST):
    """MlvsDataImputer::impute_latent_data_point: (u, w, z = w u) of the observation's M rows"""
    L = ir.oracle().lib
    rng = slot_rng(seed, chain, MLOGIT_STREAM, MLOGIT_STRIDE, sweep * n + i, slot_limit)
    nch = len(eta)
    comps = []
    stats = {"retries": 0, "unmix_margin": math.inf, "comps": comps}
    try:
        u, w = mo.impute_point([float(e) for e in eta], int(y), lambda: L.bo_unif(C.byref(rng)), stats, M=M)
    except RuntimeError:
        # (the kernel: a non-finite linear predictor is an error, u = w = z = 0 and no number read)
        out = {(k, m): 0.0 for k in "uwz" for m in range(nch)}
        return Obs(out, ("error",), math.inf, status="impute_error", exact=True, comps=(), where=ir._where(rng))
    out = {}
    for m in range(nch):
        out[("u", m)], out[("w", m)], out[("z", m)] = u[m], w[m], w[m] * u[m]
    where = ir._where(rng)
    return Obs(out, (tuple(comps), stats["retries"], where), stats["unmix_margin"], exact=False, comps=tuple(comps),
               where=where)


def wss_tree(w, u, n, nch, fma):
    """the kernel's fixed tree over one chain's rows, in numpy: (the blocks' shares, their sum).
    A lane adds its observation's rows in order, lanes past n add 0, a wave's 64 lanes fold in
    halves, the four waves are added in order, the blocks in order.  fma: each step of a lane's
    `wss += w * (u * u)` is one rounding (a fused multiply-add) instead of two.  The source does not
    say which: the compiler's contraction decides, so a caller that compares bits accepts either"""
    from fractions import Fraction
    w, u = np.asarray(w, float).reshape(n, nch), np.asarray(u, float).reshape(n, nch)
    nblocks = (n + 255) // 256
    lane = np.zeros(nblocks * 256)
    for i in range(n):
        a = 0.0
        for m in range(nch):
            sq = u[i, m] * u[i, m]
            a = float(Fraction(w[i, m]) * Fraction(sq) + Fraction(a)) if fma else a + w[i, m] * sq
        lane[i] = a
    v = lane.reshape(nblocks, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v[:, :, :off] + v[:, :, off:2 * off]
    s = v[:, :, 0]
    part = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]
    total = 0.0
    for b in range(nblocks):
        total = total + part[b]
    return part, total


# ---- sigma^2 and nu --------------------------------------------------------------------------------
def nu_logf(M, prior, nobs, n_log_sigma, u):
    """the slice sampler's target as student_sigma_nu_kernel's StuSlice::logf writes it, on the
    table's functions (HOST: student_oracle.nu_log_post to rounding)"""
    kind, a, b = prior

    def logf(nu):
        if kind == 0:
            lp = -math.inf if (nu > b or nu < a) else M.log(1.0 / (b - a))
        elif not nu > 0:
            lp = -math.inf
        else:
            lp = M.fused(M.fused(a * M.log(b) - _lgamma(M, a) + (a - 1) * M.log(nu)) - b * nu)
        if lp == -math.inf:
            return lp
        with np.errstate(over="ignore"):
            s = moved_sum(M, "log1p", np.log1p(u / nu), LOG1P_TERM_ULPS)
        c = _lgamma(M, 0.5 * (nu + 1)) - _lgamma(M, 0.5 * nu) - 0.5 * M.log(nu * 3.141592653589793)
        return M.fused((lp + M.fused(nobs * c - n_log_sigma)) - 0.5 * (nu + 1) * s)
    return logf


def sigma_nu_chain(case, c, M=HOST):
    """what student_sigma_nu_kernel<SS> writes for chain c: sigsq, nu, dx, margin, u, the two sigma^2
    moments of acc and the trace row, keyed (name, index)"""
    L = _L(M)
    n, ss = case["n"], case["kind"].endswith("_ss")
    eta = eta_rows(case, c, M)
    obs = case["observed"].astype(bool) if ss else np.ones(n, bool)
    yi = case["y"] - case["offset"][c, :n] if ss else case["y"]
    r = np.where(obs, yi - eta, 0.0)
    wsse = moved_sum(M, "wsse", np.where(obs, case["w_in"][c] * (r * r), 0.0), WSSE_TERM_ULPS)
    nobs = float(obs.sum()) if ss else float(n)
    rng = slot_rng(case["seed"], case["chain_offset"] + c, SN_STREAM, SN_STRIDE, case["sweep"], case["slot_limit"])
    tr = dr.Tr()
    try:
        sigsq = dr.draw_variance(L, M, rng, tr, nobs + case["prior_df"], wsse + case["prior_ss"], case["sigma_max"])
    except dr.Bad:
        return Obs({}, ("bad",), tr.margin, status="rng_branch", wsse=wsse, nobs=nobs)
    sigma = M.sqrt(sigsq)
    t = r / sigma
    u = np.where(obs, t * t, 0.0)
    x, dx = float(case["nu"][c]), float(case["dx"][c])
    stats, status = {}, 0
    try:
        nu, dx_out, mg = so.slice_draw_nu(lambda: L.bo_unif(C.byref(rng)), lambda: 1.0 * L.bo_exp_rand(C.byref(rng)),
                                          nu_logf(M, case["nu_prior"], nobs, nobs * M.log(sigma), u), x, dx, stats,
                                          fused=M.fused)
    except so.SliceError:
        status, nu, dx_out, mg = "slice_error", x, dx, stats["margin"]
    out = {("sigsq", 0): sigsq, ("nu", 0): nu, ("dx", 0): dx_out}
    if math.isfinite(mg):
        out[("margin", 0)] = mg
    for i in range(n):
        out[("u", i)] = float(u[i])
    if case.get("acc") is not None:
        a, s_in = case["acc"][c], float(case["sigsq"][c])
        out[("acc", ACC_SIGSQ)] = (a[ACC_SIGSQ] - s_in) + sigsq
        out[("acc", ACC_SIGSQ2)] = M.fused(M.fused(a[ACC_SIGSQ2] - s_in * s_in) + sigsq * sigsq)
    sig = (tuple(tr.path), stats["doublings"], stats["shrinks"], ir._where(rng))
    return Obs(out, sig, min(tr.margin, mg), status=status, wsse=wsse, nobs=nobs, doublings=stats["doublings"],
               shrinks=stats["shrinks"], path=tuple(tr.path), slice_margin=mg)


# ---- the cases -------------------------------------------------------------------------------------
# A case is a dict of what the probe takes.  Unless it says otherwise: 3 chains, chain 0 includes
# two columns (its own and the last, a column of small dyadic numbers that is 0 in every even
# row), chain 1 none (an empty model), chain 2 its own alone with coefficient 1; chain_offset 5,
# sweep 3.  Column c of X is set so that chain c's linear predictor is the table's.
OUTPUTS = dict(student=("w", "z"), student_ss=("w", "h"), quantile=("w", "z"), mlogit=("u", "w", "z"))
KINDS = tuple(OUTPUTS)
SECOND, SECOND_EXACT = 0.3, 0.375
NUS = (0.11, 1.0, 2.0, 2.0000001, 5.0, 99.0)
# one nu and one sigma^2 per chain.  Chain 1 is the empty model (eta = 0: it sees only delta = y /
# sigma), so it REPEATS a nu; each of the six has a chain with a model, which meets every delta
CHAIN_NUS = (0.11, 5.0, 1.0, 2.0, 2.0000001, 5.0, 99.0)
CHAIN_SIGSQS = (1.0, 4.0, 0.25, 2.0, 1.0, 9.0, 0.0625)
DELTAS = (0.0, 1e-8, -1e-8, 1.0, -1.0, 30.0, -30.0, 1e4, -1e4)
STUDENT_Y = (0.0, 1.5, -2.25)
MISSING = (0, 63, 64, 255, 256)
QUANTILE_Y = (0.0, 1.25, -1.25)
RESIDUALS = (0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e-12, -1e-12, 1e-6, -1e-6, 1.0, -1.0, 1e6, -1e6)
QUANTILES = {1: 0.05, 255: 0.5, 256: 0.95, 257: 0.05, 513: 0.95}
CHOICES = {1: 3, 255: 2, 256: 16, 257: 3, 513: 16}


def _frame(kind, n, target, rows=1, chains=3, **more):
    """the default models around `target` (chains x n rows: the linear predictors wanted)"""
    N, p = n * rows, chains + 1
    X = np.zeros((N, p))
    second = np.where(np.arange(N) % 2 == 0, 0.0, ((np.arange(N) * 7) % 11 - 5) / 4.0)
    # (quantile: a dyadic coefficient, so the product is exact and the sum rounds once, fused or not
    # -- its residuals of 0 and 5e-324 must be those; elsewhere a coefficient whose products round)
    coef = SECOND_EXACT if kind == "quantile" else SECOND
    X[:, p - 1] = second
    gamma, beta = np.zeros((chains, p), np.uint8), np.full((chains, p), 1000.0)   # (excluded: must not be read)
    with np.errstate(over="ignore"):
        for c in range(chains):
            if c == 1:
                continue
            gamma[c, c], beta[c, c] = 1, 1.0
            X[:, c] = target[c]
            if c == 0:
                gamma[c, p - 1], beta[c, p - 1] = 1, coef
                X[:, 0] = target[0] - coef * second
    case = dict(kind=kind, n=n, p=p, chains=chains, chain_offset=CHAIN_OFFSET, sweep=SWEEP, seed=SEED, slot_limit=0,
                X=X, gamma=gamma, beta=beta, status0=np.zeros(chains, np.int32), exact_eta=kind == "quantile")
    case.update(more)
    return case


def _cross(n, chains, A, B, shift):
    """index into a list of B values for observation i of chain c, every pair with i mod A within
    A B observations (A + 1 and B without a common factor)"""
    assert math.gcd(A + 1, B) == 1
    i = np.arange(n)
    return np.array([(i // A + i + shift * c) % B for c in range(chains)])


def student_table(kind, n, chains=7, **more):
    """delta crossed with nu (CHAIN_NUS: one nu, one sigma^2 per chain; chains = 3 still has nu = 0.11
    and 1 on chains with a model) and three responses; for the state space
    family missing steps at the waves' and rounds' edges and an offset with offset_stride > n"""
    ss = kind == "student_ss"
    nu, sigsq = np.array(CHAIN_NUS[:chains]), np.array(CHAIN_SIGSQS[:chains])
    y = np.array([STUDENT_Y[i % 3] for i in range(n)])
    delta = np.array(DELTAS)[_cross(n, chains, 3, len(DELTAS), 2)]
    extra = {}
    base = np.tile(y, (chains, 1))
    if ss:
        stride = n + 5
        offset = np.round(np.random.RandomState(n + 17).uniform(-0.5, 0.5, (chains, stride)) * 1024) / 1024
        observed = np.ones(n, np.uint8)
        observed[[i for i in MISSING + (n - 1,) if i < n]] = 0
        extra = dict(observed=observed, offset=offset, offset_stride=stride)
        base = base - offset[:, :n]
    target = base - delta * np.sqrt(sigsq)[:, None]
    return _frame(kind, n, target, chains=chains, y=y, nu=nu, sigsq=sigsq, **extra, **more)


def quantile_table(n, q=None, special=None, **more):
    """the residuals crossed with three responses; special = (chain, residual): that chain's table
    also holds +-residual"""
    chains = 3
    y = np.array([QUANTILE_Y[i % 3] for i in range(n)])
    idx = _cross(n, chains, 3, len(RESIDUALS), 5)
    d = np.array(RESIDUALS)[idx]
    if special is not None:
        c, r = special
        d[c, idx[c] == 9] = r
        d[c, idx[c] == 10] = -r
    q = QUANTILES.get(n, 0.05) if q is None else q
    return _frame("quantile", n, y - d, y=y, shift=1.0 - 2.0 * q, q=q, **more)


def mlogit_eta(n, nch, chains=3):
    """the four kinds of rows: all 0, one at +700, one at -700, spread 0 .. 40"""
    eta = np.zeros((chains, n, nch))
    for c in range(chains):
        for i in range(n):
            kind, at = (i + c) % 4, (i // 4) % nch
            if kind == 1:
                eta[c, i, at] = 700.0
            elif kind == 2:
                eta[c, i, at] = -700.0
            elif kind == 3:
                eta[c, i] = np.roll(np.round(np.linspace(0.0, 40.0, nch) * 8) / 8, i)
    return eta.reshape(chains, n * nch)


def mlogit_table(n, nch=None, **more):
    nch = CHOICES.get(n, 3) if nch is None else nch
    y = (np.arange(n) % nch).astype(np.int32)
    return _frame("mlogit", n, mlogit_eta(n, nch), rows=nch, y=y, M=nch, **more)


def table_case(kind, n, **more):
    if kind.startswith("student"):
        return student_table(kind, n, **more)
    return quantile_table(n, **more) if kind == "quantile" else mlogit_table(n, **more)


COLUMNS8 = ir.COLUMNS8


def model_case(kind, which):
    """p = 1100 at n = 257: exactly KMAX columns in every chain, or (1025) one too many in chain 1
    and eight elsewhere.  X and beta are small dyadic numbers: every product and partial sum of a
    linear predictor is exact in any order and with any fusion"""
    n, p = 257, 1100
    case = table_case(kind, n, **(dict(chains=3) if kind.startswith("student") else dict(nch=2) if kind == "mlogit" else {}))
    rows = case.get("M", 1)
    keep = [j for j in range(p) if j % 15 != 7]
    included = keep[:500] + keep[503:] if which == 1024 else COLUMNS8
    assert which != 1024 or len(included) == KMAX
    rs = np.random.RandomState(which)
    X = rs.randint(-256, 257, (n * rows, p)) / 256.0
    gamma, beta = np.zeros((3, p), np.uint8), np.full((3, p), 1000.0)
    k = len(included)
    for c in range(3):
        gamma[c, included] = 1
        beta[c, included] = rs.randint(-8, 9, k) / (64.0 * max(1, k // 16))
    if which == 1025:
        gamma[1, :], beta[1, :] = 0, 1000.0
        gamma[1, keep[:1025]], beta[1, keep[:1025]] = 1, 0.015625
    case.update(p=p, X=X, gamma=gamma, beta=beta, exact_eta=True)
    if kind == "student_ss":
        case["offset"] = np.round(case["offset"] * 4) / 4
    return case


def special_case(kind, what):
    if what == "crossing":
        n = 513
        sweep = (1 << 32) // n
        assert sweep * n < (1 << 32) <= sweep * n + n - 1
        return table_case(kind, n, sweep=sweep, **(dict(chains=3) if kind.startswith("student") else {}))
    small = dict(chains=3) if kind.startswith("student") else {}
    if what == "offset7":
        return table_case(kind, 257, chain_offset=7, **small)
    if what == "parked":
        case = table_case(kind, 257, **small)
        case["status0"][1] = FORECAST_VARIANCE
        return case
    if what == "slot1":
        # (a slot that serves one uniform: the draw goes on in the slot's spill stream)
        return table_case(kind, 257, slot_limit=1, **small)
    if what == "tiny160":
        return quantile_table(257, special=(2, 1e-160))
    if what == "huge300":
        return quantile_table(257, special=(0, 1e300))
    if what == "infbeta":
        case = mlogit_table(257)
        case["beta"][2, 2] = np.inf
        return case
    raise KeyError(what)


def case_names():
    names = []
    for kind in KINDS:
        names += ["%s-n%d" % (kind, n) for n in SIZES]
        names += ["%s-%s" % (kind, what) for what in ("crossing", "offset7", "parked", "model1024", "model1025", "slot1")]
    return names + ["quantile-tiny160", "quantile-huge300", "mlogit-infbeta"]


@functools.lru_cache(maxsize=None)
def case_of(name):
    kind, what = name.split("-")
    if what.startswith("model"):
        return model_case(kind, int(what[5:]))
    if what[0] == "n" and what[1:].isdigit():
        return table_case(kind, int(what[1:]))
    return special_case(kind, what)


def _obs_of(case, c, i, eta, M):
    kind, n = case["kind"], case["n"]
    args = (case["seed"], case["chain_offset"] + c, case["sweep"], i, n)
    if kind == "quantile":
        return quantile_obs(*args, float(eta[i]), float(case["y"][i]), case["shift"], case["slot_limit"], M=M)
    if kind == "mlogit":
        nch = case["M"]
        return mlogit_obs(*args, eta[i * nch:(i + 1) * nch], case["y"][i], case["slot_limit"], M=M)
    ss = kind == "student_ss"
    return student_obs(*args, float(eta[i]), float(case["y"][i]), float(case["sigsq"][c]), float(case["nu"][c]),
                       case["slot_limit"], M=M, ss=ss, offset=float(case["offset"][c, i]) if ss else 0.0,
                       observed=bool(case["observed"][i]) if ss else True)


def reference(case):
    """what an imputation kernel must leave: want[name], bound[name] (chains x rows), the written,
    exact and loose masks, status (chains) and per observation the branch facts"""
    kind, n, chains, rows = case["kind"], case["n"], case["chains"], case.get("M", 1)
    names = OUTPUTS[kind]
    want = {k: np.full((chains, n * rows), np.nan) for k in names}
    bound = {k: np.zeros((chains, n * rows)) for k in names}
    written, exact, loose = (np.zeros((chains, n * rows), bool) for _ in range(3))
    status = case["status0"].copy()
    margin, facts = np.inf, []
    for c in range(chains):
        if status[c] != OK:
            continue
        if int(case["gamma"][c].sum()) > KMAX:
            status[c] = MODEL_TOO_LARGE
            continue
        etas = {None: eta_rows(case, c)}
        if not case.get("exact_eta") and int(case["gamma"][c].sum()) > 1:
            for k in range(ir.REPLAYS):
                etas[k] = eta_rows(case, c, MathTable(k))
        for i in range(n):
            base, bnd, ok = bounded(lambda M=HOST: _obs_of(case, c, i, etas.get(M.rnd, etas[None]), M))
            facts.append((c, i, base))
            margin = min(margin, base.margin)
            assert base.status != "rng_branch"          # (no case is built there)
            if base.status:
                assert status[c] in (OK, STATUS[base.status]), "two error codes on one chain"
                status[c] = STATUS[base.status]
            sl = slice(i * rows, (i + 1) * rows)
            written[c, sl] = True
            if not ok:
                loose[c, sl] = True
                continue
            exact[c, sl] = base.facts["exact"]
            for (k, m), v in base.out.items():
                want[k][c, i * rows + m], bound[k][c, i * rows + m] = v, bnd[(k, m)]
    return dict(want=want, bound=bound, written=written, exact=exact, loose=loose, status=status, margin=margin,
                facts=facts)


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """the case's reference, computed once and shared (nothing may change it)"""
    return reference(case_of(name))


def wss_reference(case, ref):
    """per chain (wss, bound) from the reference's u and w: the sum of w u^2, each term's bound
    2 w |u| bound(u) + WSS_TERM_ULPS ulp, plus the summation bound N u Sum|term|"""
    out = []
    for c in range(case["chains"]):
        w, u, bu = ref["want"]["w"][c], ref["want"]["u"][c], ref["bound"]["u"][c]
        terms = w * u * u
        bound = float(np.sum(2 * w * np.abs(u) * bu + WSS_TERM_ULPS * np.spacing(np.abs(terms)))) + terms.size * UNIT * float(np.sum(np.abs(terms)))
        out.append((math.fsum(terms), bound))
    return out


# ---- the cases of student_sigma_nu_kernel ------------------------------------------------------------
PRIOR_UNIFORM, PRIOR_GAMMA = (0, 0.1, 100.0), (1, 2.0, 0.1)
ACC_IN = (10.5, 300.25)


def sigma_nu_case(ss, n, prior=PRIOR_UNIFORM, sigma_max=np.inf, nu=(0.5, 3.0, 60.0), dx=(1.0, 1e-3, 1.0), acc=True,
                  trace_stride=0, trace_idx=(0, 0, 0), margin=(np.inf, np.inf, 1e-300), seed=SEED, sweep=SWEEP, **more):
    """Student-t noise about the default models' predictors, weights from a gamma law; for the state
    space family missing steps at the edges; chain c enters with nu[c], dx[c] and margin[c]"""
    kind = "sn_ss" if ss else "sn"
    rs = np.random.RandomState(1000 * n + 7 * len(more) + (3 if ss else 0))
    chains = 3
    y = np.round(rs.standard_t(4, n) * 2.0 * 256) / 256
    target = np.round(rs.normal(0.0, 0.5, (chains, n)) * 256) / 256
    extra = {}
    if ss:
        stride = n + 5
        observed = np.ones(n, np.uint8)
        observed[[i for i in MISSING + (n - 1,) if 0 < i < n]] = 0      # (step 0 stays: n = 1 has an observation)
        if n > 300:
            observed[0] = 0
        extra = dict(observed=observed, offset_stride=stride,
                     offset=np.round(rs.uniform(-0.5, 0.5, (chains, stride)) * 1024) / 1024)
    case = _frame(kind, n, target, y=y, nu=np.array(nu, float), dx=np.array(dx, float), sigsq=np.array((1.0, 4.0, 0.25)),
                  margin=np.array(margin, float), w_in=rs.gamma(2.0, 0.5, (chains, n)), prior_df=1.0, prior_ss=1.0,
                  sigma_max=float(sigma_max), nu_prior=prior, trace_stride=trace_stride,
                  trace_idx=np.array(trace_idx, np.int32), seed=seed, sweep=sweep, **extra)
    case["acc"] = None
    if acc:
        case["acc"] = np.round(rs.uniform(1.0, 2.0, (chains, ACC_COUNT)) * 64) / 64
        case["acc"][:, ACC_SIGSQ], case["acc"][:, ACC_SIGSQ2] = ACC_IN
    case.update(more)
    return case


def sigma_nu_cases():
    cases = {}
    for ss in (False, True):
        tag = "sn_ss" if ss else "sn"
        for k, n in enumerate((1, 255, 256, 257, 1000)):
            cases["%s-n%d" % (tag, n)] = sigma_nu_case(ss, n, prior=(PRIOR_UNIFORM, PRIOR_GAMMA)[k % 2], acc=k % 2 == 0,
                                                       seed=SEED + k)
        cases[tag + "-gamma"] = sigma_nu_case(ss, 257, prior=PRIOR_GAMMA, seed=SEED + 5)
        cases[tag + "-sigmamax"] = sigma_nu_case(ss, 257, sigma_max=0.5, seed=SEED + 6)
        cases[tag + "-trace0"] = sigma_nu_case(ss, 64, trace_stride=4, trace_idx=(0, 1, 4), seed=SEED + 7)
        cases[tag + "-trace5"] = sigma_nu_case(ss, 64, trace_stride=4, trace_idx=(5, 4, 1), acc=False, seed=SEED + 8)
        # nu enters outside the uniform prior's support: the target is -inf there (SliceError)
        cases[tag + "-sliceerror"] = sigma_nu_case(ss, 257, prior=(0, 1.0, 100.0), trace_stride=4, trace_idx=(2, 2, 2),
                                                   seed=SEED + 9)
        cases[tag + "-parked"] = sigma_nu_case(ss, 257, seed=SEED + 10)
        cases[tag + "-parked"]["status0"][1] = FORECAST_VARIANCE
        cases[tag + "-offset7"] = sigma_nu_case(ss, 257, chain_offset=7, seed=SEED + 11)
        # sweep 2^32 + 1: the slot's index is a 64-bit number
        cases[tag + "-sweep64"] = sigma_nu_case(ss, 64, sweep=(1 << 32) + 1, seed=SEED + 12)
    cases["sn-model1024"] = _sn_model(1024)
    cases["sn-model1025"] = _sn_model(1025)
    return cases


def _sn_model(which):
    case = sigma_nu_case(False, 257)
    m = model_case("student", which)
    case.update(p=m["p"], X=m["X"], gamma=m["gamma"], beta=m["beta"], exact_eta=True)
    return case


@functools.lru_cache(maxsize=None)
def sigma_nu_ref(name):
    """per chain (Obs, bounds, same) or None where the chain is parked / its model too large, and the
    status words"""
    case = sigma_nu_cases()[name]
    status, chains_ = case["status0"].copy(), []
    for c in range(case["chains"]):
        if status[c] != OK:
            chains_.append(None)
            continue
        if int(case["gamma"][c].sum()) > KMAX:
            status[c] = MODEL_TOO_LARGE
            chains_.append(None)
            continue
        base, bnd, same = bounded(lambda M=HOST: sigma_nu_chain(case, c, M))
        if base.status:
            status[c] = STATUS[base.status]
        chains_.append((base, bnd, same))
    return dict(chains=chains_, status=status)


EXPAND_SHAPES = ((1, 2, 1, 0), (5, 3, 0, 2), (257, 16, 3, 1), (300, 4, 2, 2))


def expand_case(n, nch, psub, pch):
    rs = np.random.RandomState(n + nch)
    Xs = rs.normal(size=(n, psub)) if psub else None
    Xc = rs.normal(size=(n * nch, pch)) if pch else None
    return Xs, Xc, mo.expand_design(Xs, Xc, n, nch)
