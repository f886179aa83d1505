"""Cases, references and bounds for the large-model kernel's pieces (boom_amd/csrc/
ssvs_big_kernel.hip: chol_tile, chol_tile_regs, big_solve, big_build_body, big_eval), on top of
fill_ref's matrices, index lists, block layout and long-double forward substitution.

A build case is one chain's model at p = P_BIG: the shared SPD matrices V and A, the sorted
index list g of k included variables, the scales sv, sa, sx (none of them 1), an xty vector
(a combination of V's columns plus noise, so that Q stays of the order of the data), a prior
mean with three non-zero entries among the included variables (the first, the middle and the
LAST one: the last panel of every case has one) and the log prior terms.

All references are numpy.longdouble; all bounds are the textbook ones with the constant
gamma_n = n u / (1 - n u), u = 2^-53, n the number of rounded operations the code performs on
the quantity (counted at each bound below).  No constant is tuned on the device.
check_build / check_eval return the largest error / bound per quantity; the callers assert
that none exceeds 1.  numpy_build / numpy_eval are the same computations in plain f64 numpy
(numpy.linalg.cholesky, f64 forward substitution, the formulas in f64): test_big_ref_cpu.py
shows them inside every bound."""
import functools

import numpy as np

import fill_ref as F

U, LD = F.U, F.LD
P_BIG = 1100
SX = 0.61
PI = 0.3
DF = 1500.0 + 1.0
KINDS = F.KINDS
INF = float("inf")

BUILD_CASES = ([(128, k) for k in (1, 63, 64, 65, 127, 128)] + [(256, k) for k in (129, 191, 192, 193, 256)] +
               [(512, k) for k in (257, 449, 512)] + [(1024, 1024)])
MODE1_CASES = [(256, 129), (512, 449)]
SOLVE_CASES = [(128, 65), (128, 128), (256, 129), (256, 193), (512, 449), (1024, 1024)]
TILE_KK = (1, 2, 7, 8, 9, 63, 64)
# (kcap, k) of the proposal windows: the matrix-core path up to 128, big_solve above; 136 is the one
# size here with k % 8 == 0 and k % 64 != 0, where the gather's row k is a row big_solve reads
EVAL_CASES = [(128, 64), (128, 65), (128, 128), (256, 129), (256, 136), (256, 192), (256, 193), (512, 449),
              (1024, 1024)]
EVAL_WINDOWS = (0, 512, 1088)


def gamma_n(n):
    return n * U / (1.0 - n * U)


def kcap_of(k):
    return 128 if k <= 128 else 256 if k <= 256 else 512 if k <= 512 else 1024


# ---- block-packed factors ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tril_index(n):
    """(rows, cols, offsets) of the lower triangle of an n x n factor in block-packed order"""
    m, c = np.tril_indices(n)
    I, J = m >> 3, c >> 3
    return m, c, ((I * (I + 1)) // 2 + J) * 64 + (m & 7) * 8 + (c & 7)


def unpack(packed, n):
    """dense n x n lower triangle of a block-packed factor"""
    m, c, o = _tril_index(n)
    L = np.zeros((n, n))
    L[m, c] = packed[o]
    return L


def pack_into(dst, L):
    m, c, o = _tril_index(L.shape[0])
    dst[o] = L[m, c]


def block(c, kcap, hostile=True):
    """F.block for any capacity (vectorised): the model of case c as the product leaves it, w and b_g
    zero behind k (the large-model build zeroes them up to the capacity), NaN where nothing is written"""
    S, k = F.layout(kcap), c["k"]
    kpad8 = (k + 7) & ~7
    b = np.full(S["total"], np.nan if hostile else 0.0)
    for name, L in (("Lv", c["Lv"]), ("La", c["La"])):
        Lp = np.zeros((kpad8, kpad8))
        Lp[:k, :k] = L
        pack_into(b[S[name]:], Lp)
        rd = S["rd" + name[1]]
        b[rd:rd + k] = 1.0 / np.diag(L)
        b[rd + k:rd + kpad8] = 0.0
    b[S["w"]:S["w"] + kcap] = 0.0
    b[S["bg"]:S["bg"] + kcap] = 0.0
    b[S["w"]:S["w"] + k] = c["w"]
    b[S["bg"]:S["bg"] + k] = c["bg"]
    return b


def big_lds_layout(p, kcap):
    """ssvs_big_lds_layout (ssvs_params.h), byte offsets; the GPU test checks it against the product's"""
    pv = (((p + 1) * 2) + 15) & ~15
    pg = (p + 15) & ~15
    kg = ((kcap * 2) + 15) & ~15
    o, L = 0, {}
    for name, size in (("tile", 36 * 64 * 8), ("rdt", 64 * 8), ("w", kcap * 8), ("y", kcap * 8), ("rd", kcap * 8),
                       ("bst", kcap * 8), ("ctrl", 512), ("g", kg), ("gst", kg), ("perm0", pv), ("perm1", pv),
                       ("oth", pv), ("last", 2 * pv), ("pred", pv), ("gam", pg), ("gam0", pg), ("nbr", pg)):
        L[name] = o
        o += size
    L["total"] = o
    return L


# ---- exact products ---------------------------------------------------------------------------
def gram_exact(L):
    """(L L' in long double, a bound on what it leaves out).  L is cut into three fixed-point pieces
    of 21 bits; a product of two pieces has 42 bits and a sum of up to 1024 of them 52, so every f64
    matrix product below is exact and only the nine partial results are added in long double."""
    n = L.shape[0]
    assert n <= 1024
    s = 2.0 ** np.ceil(np.log2(np.abs(L).max()))
    R = L / s
    pieces = []
    for _ in range(3):
        q = np.trunc(R * 2.0 ** 21)
        pieces.append(q)
        R = R * 2.0 ** 21 - q
    out = np.zeros((n, n), LD)
    for a in (2, 1, 0):
        for b in (2, 1, 0):
            out += (pieces[a] @ pieces[b].T).astype(LD) * LD(2.0) ** (-21 * (a + b + 2))
    left = 2.0 * n * 2.0 ** -63 * s * s      # |L| <= s; the part of each entry below 2^-63 s
    return out * LD(s) * LD(s), left


# ---- cases ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def xty_vector(kind):
    V, _ = F.matrices(P_BIG, kind)
    rng = np.random.Generator(np.random.PCG64(4242 + (kind == "ill")))
    beta = rng.standard_normal(P_BIG) * (rng.uniform(size=P_BIG) < 0.2)
    x = (F.SV * V) @ beta / SX + 1e-3 * rng.standard_normal(P_BIG)
    x.setflags(write=False)
    return x


def prior_mean(g):
    """three non-zero entries (fewer where the model has fewer variables): the first, the middle and
    the last included variable"""
    b = np.zeros(P_BIG)
    for pos, val in ((0, 0.7), (len(g) // 2, -1.3), (len(g) - 1, 0.4)):
        b[g[pos]] = val
    return b


@functools.lru_cache(maxsize=None)
def build_case(k, kind, mode=0):
    V, A = F.matrices(P_BIG, kind)
    g = F.index_list(P_BIG, k)
    gam = np.zeros(P_BIG, np.uint8)
    gam[g] = 1
    b = prior_mean(g)
    c = dict(p=P_BIG, k=k, kind=kind, mode=mode, V=V, A=A, g=g, gamma=gam, b=b, xty=xty_vector(kind),
             l1=np.full(P_BIG, np.log(PI)), l0=np.full(P_BIG, np.log1p(-PI)), sv=F.SV, sa=F.SA, sx=SX, DF=DF,
             max_model_size=-1)
    c["Mv"] = V[np.ix_(g, g)] * F.SV                    # f64 products, one rounding each: what the kernel factors
    c["Ma"] = A[np.ix_(g, g)] * F.SA
    # ss0q: above the Q an f64 solve gives, so that SS > 0 with room
    r = c["Ma"] @ b[g] + c["xty"][g] * SX
    w = np.linalg.solve(np.linalg.cholesky(c["Mv"]), r)
    c["ss0q"] = float(np.round(1.5 * (w @ w) + 100.0))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def cholesky_ld(M):
    """long-double Cholesky of the f64 matrix M, column by column"""
    n = M.shape[0]
    L = np.zeros((n, n), LD)
    A = M.astype(LD)
    for j in range(n):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        d = np.sqrt(col[0])
        L[j:, j] = col / d
        L[j, j] = d
    return L


@functools.lru_cache(maxsize=None)
def build_reference(k, kind, mode=0):
    """end to end in long double from the f64 products M_g: ldv, lda, w, Q, c, SS, logp, lp"""
    c = build_case(k, kind, mode)
    g = c["g"]
    Lv, La = cholesky_ld(c["Mv"]), cholesky_ld(c["Ma"])
    bg = c["b"][g].astype(LD)
    ab = c["Ma"].astype(LD) @ bg
    r = ab + c["xty"][g].astype(LD) * LD(SX)
    w = F.forward(Lv, r)
    Q, cc = w @ w, bg @ ab
    ldv, lda = 2 * np.log(np.diag(Lv)).sum(), 2 * np.log(np.diag(La)).sum()
    lp = (c["l1"][g].astype(LD)).sum() + (c["l0"][c["gamma"] == 0].astype(LD)).sum()
    SS = LD(c["ss0q"]) + cc - Q
    return dict(ldv=ldv, lda=lda, w=w, Q=Q, c=cc, SS=SS, lp=lp, logp=_logp(c, lp, ldv, lda, Q, cc, SS))


def _logp(c, lp, ldv, lda, Q, cc, SS):
    if c["mode"]:
        return lp + (lda - ldv) / 2 - (cc - Q) / 2
    return lp + (lda - ldv) / 2 - (LD(c["DF"]) / 2 - 1) * np.log(SS)


def numpy_build(c):
    """the build in plain f64 numpy: the same fields check_build takes from the device"""
    g, k = c["g"], c["k"]
    Lv, La = np.linalg.cholesky(c["Mv"]), np.linalg.cholesky(c["Ma"])
    bg = c["b"][g]
    ab = c["Ma"] @ bg
    r = ab + c["xty"][g] * c["sx"]
    w = np.zeros(k)
    for i in range(k):
        w[i] = (r[i] - Lv[i, :i] @ w[:i]) / Lv[i, i]
    Q, cc = float(w @ w), float(bg @ ab)
    ldv, lda = 2.0 * np.log(np.diag(Lv)).sum(), 2.0 * np.log(np.diag(La)).sum()
    lp = float(np.where(c["gamma"] != 0, c["l1"], c["l0"]).sum())
    SS = c["ss0q"] + cc - Q
    if c["mode"]:
        logp = lp + 0.5 * (lda - ldv) - 0.5 * (cc - Q)
    else:
        logp = lp + 0.5 * (lda - ldv) - (0.5 * c["DF"] - 1.0) * np.log(SS)
    return dict(Lv=Lv, La=La, rdv=1.0 / np.diag(Lv), rda=1.0 / np.diag(La), w=w, Q=Q, c=cc, ldv=float(ldv),
                lda=float(lda), lp=lp, SS=float(SS), logp=float(logp))


def _ratio(err, bound):
    """largest err / bound; an entry with no room at all has to be exact"""
    err, bound = np.asarray(err, LD), np.asarray(bound, LD)
    assert np.all(np.isfinite(err.astype(np.float64))), "not finite"
    tight = bound <= 0
    if np.any(tight):
        assert np.all(err[tight] == 0), "an error where the bound leaves none"
    return float((err[~tight] / bound[~tight]).max()) if np.any(~tight) else 0.0


def factor_ratio(M, L):
    """Higham, Thm 10.3: |M - L L'| <= gamma_{k+1} |L| |L|' componentwise (lower triangle: M is read
    there).  k + 1: the k - 1 fused multiply-subtracts of an entry, the division (or the square root)
    and one to spare, as the theorem has it."""
    k = L.shape[0]
    G, left = gram_exact(L)
    bound = gamma_n(k + 1) * (np.abs(L) @ np.abs(L).T) + left
    i = np.tril_indices(k)
    return _ratio(np.abs(M.astype(LD) - G)[i], bound[i])


def rd_ratio(L, rd):
    """rd_j = fl(1 / l_jj): |rd_j l_jj - 1| <= u to first order, 2 u allowed"""
    return _ratio(np.abs(rd.astype(LD) * np.diag(L).astype(LD) - 1), np.full(L.shape[0], 2 * U))


def logdet_ratio(L, ld):
    """2 sum log l_jj of the device's own factor.  Per tile the logarithms (one ulp each: factor
    1 + 2 u with the library's slack) are added one after the other (at most 63 additions), the tiles'
    sums one after the other (npan), the doubling is exact: gamma_{2 + 63 + npan} sum |log l_jj|"""
    k = L.shape[0]
    lg = np.log(np.diag(L).astype(LD))
    npan = (k + 63) // 64
    return _ratio(abs(LD(ld) - 2 * lg.sum()), 2 * gamma_n(65 + npan) * np.abs(lg).sum() + 4 * U * abs(float(2 * lg.sum())))


def check_build(c, out, end_to_end=True, a_ok=True):
    """out: Lv, La (dense k x k f64), rdv, rda, w (k), and the scalars logp, lp, ldv, lda, Q, c, SS.
    Returns {quantity: largest error / bound}.  a_ok=False: A_g has no factor (lda and logp are -inf):
    everything that does not depend on it."""
    g, k, p = c["g"], c["k"], c["p"]
    npan = (k + 63) // 64
    Lv, La, w = out["Lv"], out["La"], out["w"]
    R = {}
    R["Lv"], R["rdv"], R["ldv"] = factor_ratio(c["Mv"], Lv), rd_ratio(Lv, out["rdv"]), logdet_ratio(Lv, out["ldv"])
    if a_ok:
        R["La"], R["rda"], R["lda"] = factor_ratio(c["Ma"], La), rd_ratio(La, out["rda"]), logdet_ratio(La, out["lda"])
    # lp: per lane ceil(p / 64) additions, six more across the wave
    terms = np.where(c["gamma"] != 0, c["l1"], c["l0"]).astype(LD)
    R["lp"] = _ratio(abs(LD(out["lp"]) - terms.sum()), gamma_n((p + 63) // 64 + 6) * np.abs(terms).sum())
    # r = A_g b_g + sx xty_g: nb terms of two roundings each and their sum, the product sx xty, the
    # last addition: gamma_{nb + 3} of the terms' magnitudes
    bg = c["b"][g].astype(LD)
    nb = int(np.count_nonzero(c["b"][g]))
    Ma = c["Ma"].astype(LD)
    ab = Ma @ bg
    ab_abs = np.abs(Ma) @ np.abs(bg)
    xs = c["xty"][g].astype(LD) * LD(c["sx"])
    r = ab + xs
    r_err = gamma_n(nb + 3) * (ab_abs + np.abs(xs))
    # w (Higham, Thm 8.5): |L w - r| <= gamma_k |L| |w|; the kernel multiplies by the rounded
    # reciprocal of the diagonal instead of dividing: two roundings more
    res = np.abs(Lv.astype(LD) @ w.astype(LD) - r)
    R["w"] = _ratio(res, gamma_n(k + 2) * (np.abs(Lv) @ np.abs(w)).astype(LD) + r_err)
    # Q = sum w^2: a product, npan additions in the lane, six across the wave
    wl = w.astype(LD)
    R["Q"] = _ratio(abs(LD(out["Q"]) - wl @ wl), gamma_n(npan + 7) * (wl @ wl))
    # c = sum b_m (A b)_m: the rounded (A b)_m (gamma_{nb + 2}), a product, the same sums
    R["c"] = _ratio(abs(LD(out["c"]) - bg @ ab), gamma_n(npan + 7 + nb + 2) * (np.abs(bg) @ ab_abs))
    # SS = fl(fl(ss0q + c) - Q) on the device's own c and Q: two roundings
    dQ, dc, ss0 = LD(out["Q"]), LD(out["c"]), LD(c["ss0q"])
    SS = ss0 + dc - dQ
    ss_err = 2 * U * (abs(ss0) + abs(dc) + abs(dQ))
    R["SS"] = _ratio(abs(LD(out["SS"]) - SS), ss_err)
    if not a_ok:
        return R
    # logp by the kernel's formula on the device's own lp, ldv, lda, Q, c.  Rounded operations:
    # lda - ldv, lp + that, the logarithm (two ulps allowed), its product with DF / 2 - 1, the last
    # subtraction (mode 1: c - Q, the subtraction): 6 u of the terms' magnitudes, plus SS's rounding
    lp, ldv, lda = LD(out["lp"]), LD(out["ldv"]), LD(out["lda"])
    want = _logp(c, lp, ldv, lda, dQ, dc, SS)
    h = LD(c["DF"]) / 2 - 1
    if c["mode"]:
        mag = abs(lp) + abs(lda) + abs(ldv) + abs(dc) + abs(dQ)
        extra = 0
    else:
        mag = abs(lp) + abs(lda) + abs(ldv) + h * abs(np.log(SS))
        extra = h * ss_err / SS
    R["logp"] = _ratio(abs(LD(out["logp"]) - want), 6 * U * mag + extra)
    if end_to_end:
        ref = build_reference(k, c["kind"], c["mode"])
        # the tolerance the project uses for this call (tests/test_drop_in_gpu.py)
        R["logp_end_to_end"] = _ratio(abs(LD(out["logp"]) - ref["logp"]), 1e-9 * max(1.0, abs(float(ref["logp"]))))
    return R


# ---- the per-lane solve -------------------------------------------------------------------------
def solve_bounds(L, X):
    """fill_ref.tolerances' forward-error bound of substitution, gamma_k cond(L) |x| per column,
    without the block-inverse variant's factor 8"""
    k = L.shape[0]
    return k * U * float(np.linalg.cond(L)) * np.linalg.norm(X.astype(np.float64), axis=0)


def solve_residual_ratio(L, B, X):
    """Higham, Thm 8.5, componentwise: |L x - b| <= gamma_{k+1} |L| |x|.  Row i of big_solve is i - 1
    fused multiply-subtracts and the product with the rounded reciprocal of the diagonal (two
    roundings where the theorem's division has one).  The forward bound above is cond(L) times
    this and sees little; this one is the sharp check."""
    k = L.shape[0]
    res = np.abs(L.astype(LD) @ X.astype(LD) - B.astype(LD))
    return _ratio(res, gamma_n(k + 1) * (np.abs(L) @ np.abs(X)).astype(LD))


# ---- proposals ------------------------------------------------------------------------------------
def eval_windows(k):
    """the windows a model of k variables is evaluated at (k = 1024: also the one with 53 drops)"""
    return EVAL_WINDOWS + ((1024,) if k == 1024 else ())


@functools.lru_cache(maxsize=None)
def eval_case(k, kind="ill"):
    """fill_ref's case at P_BIG with what big_eval needs besides: gamma, the vectors of the prior, a
    model's scalars consistent with the block's factors and w.  The prior mean is non-zero exactly
    where fill_ref.flags calls a lane not fast, so those lanes are the slow ones."""
    c = dict(F.case(P_BIG, k, kind))
    g = c["g"]
    gam = np.zeros(P_BIG, np.uint8)
    gam[g] = 1
    b = np.zeros(P_BIG)
    for j in range(P_BIG):
        if j % 9 == 4 and j != g[0]:
            b[j] = 0.5
    Q = float(c["w"] @ c["w"])
    cc = 3.25
    # ss0q: above every Q' the windows' fast lanes reach (the weights are fill_ref's random ones,
    # not a regression's: an add's w_n^2 = (r_j - dv)^2 / d2 is large where d2 is small)
    qmax = Q
    for jbase in eval_windows(k):
        ref = F.reference(P_BIG, k, kind, jbase)
        nv, dv, na, ab = [np.asarray(s, np.float64) for s in ref["sums"]]
        for lane in np.nonzero(ref["flags"] & F.FAST)[0]:
            j = jbase + lane
            if ref["flags"][lane] & F.ADD:
                qmax = max(qmax, Q + (xty_vector(kind)[j] * SX + ab[lane] - dv[lane]) ** 2 /
                           (c["V"][j, j] * c["sv"] - nv[lane]))
    c.update(gamma=gam, b=b, xty=xty_vector(kind), l1=np.full(P_BIG, np.log(PI)), l0=np.full(P_BIG, np.log1p(-PI)),
             sx=SX, DF=DF, mode=0, max_model_size=-1, ss0q=float(np.round(1.5 * qmax + 100.0)),
             model=np.array([-123.5, float(k * np.log(PI) + (P_BIG - k) * np.log1p(-PI)),
                             float(2 * np.log(np.diag(c["Lv"]).astype(LD)).sum()),
                             float(2 * np.log(np.diag(c["La"]).astype(LD)).sum()), Q, cc]))
    return c


def eval_reference(c, jbase, sums=None, V=None):
    """per lane: (logp in long double by the kernel's formula from the four sums, its bound, kind) with
    kind 'add', 'drop' (fast lanes), 'slow', 'empty' (k = 1's drop), 'bad' (SS' < 0 in long double; the
    bound is then that of SS' itself) or 'none' (past p).  sums: the four
    sums to put through the formula (default: fill_ref.reference's, long double)"""
    p, k, g = c["p"], c["k"], c["g"]
    ref = F.reference(p, k, c["kind"], jbase)
    tol = F.tolerances(c, ref)
    nv, dv, na, ab = [np.asarray(s, LD) for s in (sums if sums is not None else ref["sums"])]
    _, lp, ldv, lda, Q, cc = [LD(x) for x in c["model"]]
    V = c["V"] if V is None else V
    h = LD(c["DF"]) / 2 - 1
    ss0 = LD(c["ss0q"])
    logp, bound, kind = np.full(64, -INF, LD), np.zeros(64, LD), []
    for lane in range(64):
        j = jbase + lane
        if j >= p:
            kind.append("none")
            continue
        add = not c["gamma"][j]
        l1, l0 = LD(c["l1"][j]), LD(c["l0"][j])
        lpn = lp + (l1 - l0) if add else lp + (l0 - l1)
        if c["b"][j] != 0.0 and not (not add and k == 1):
            kind.append("slow")
            continue
        if not add and k == 1:
            kind.append("empty")
            logp[lane] = lpn - h * np.log(ss0)
            # (within 2 u of the two terms' magnitudes, not to the bit: the formula rounds five times)
            bound[lane] = 2 * U * (abs(lpn) + h * abs(np.log(ss0)))
            continue
        t = [LD(x[lane]) for x in tol]
        if add:
            vjj, ajj = LD(V[j, j] * c["sv"]), LD(c["A"][j, j] * c["sa"])
            d2, da2 = vjj - nv[lane], ajj - na[lane]
            rj = LD(c["xty"][j] * c["sx"]) + ab[lane]
            wn = (rj - dv[lane]) / np.sqrt(d2)
            Qn, ldvn, ldan = Q + wn * wn, ldv + np.log(d2), lda + np.log(da2)
            SS = ss0 + cc - Qn
            dQ = h / abs(SS)
            # the roundings of d2, da2 and rj count as errors of nv, na and ab
            t[0] += U * (abs(vjj) + abs(nv[lane]))
            t[2] += U * (abs(ajj) + abs(na[lane]))
            t[3] += U * (abs(rj) + abs(ab[lane]))
            deriv = (0.5 / d2 + dQ * wn * wn / d2, dQ * 2 * abs(wn) / np.sqrt(d2), 0.5 / da2,
                     dQ * 2 * abs(wn) / np.sqrt(d2))
        else:
            Qn = Q - dv[lane] * dv[lane] / nv[lane]
            ldvn, ldan = ldv + np.log(nv[lane]), lda + np.log(na[lane])
            SS = ss0 + cc - Qn
            dQ = h / abs(SS)
            deriv = (0.5 / nv[lane] + dQ * dv[lane] ** 2 / nv[lane] ** 2, dQ * 2 * abs(dv[lane]) / nv[lane],
                     0.5 / na[lane], LD(0))
        if SS < 0:
            kind.append("bad")
            bound[lane] = (sum(abs(d) * x for d, x in zip(deriv, t)) / dQ + 4 * U * (abs(ss0) + abs(cc) + abs(Qn)))
            logp[lane] = SS      # (not a log probability: the caller checks |SS'| against the bound)
            continue
        kind.append("add" if add else "drop")
        logp[lane] = lpn + (ldan - ldvn) / 2 - h * np.log(SS)
        # first-order propagation of the sums' bounds, then the formula's own roundings: about a
        # dozen operations on terms no larger than these (8 u of each), and SS's two additions
        bound[lane] = (sum(abs(d) * x for d, x in zip(deriv, t)) +
                       8 * U * (abs(lpn) + abs(lda) + abs(ldv) + h * abs(np.log(SS))) +
                       dQ * 4 * U * (abs(ss0) + abs(cc) + abs(Qn)))
    return logp, bound, kind


def copy_lane_verdict(c, lane, pos, jbase=0):
    """The add of variable jbase + lane when its row and column of V are exact copies of the included
    variable g[pos]'s (the diagonal too): in exact arithmetic d2 = 0.  From the long-double solve of
    the copied column and fill_ref.tolerances' bounds on nv, dv and ab, which of the two ends every
    admissible device value has:
      'notpd'  d2 + its bound <= 0: the lane is not positive definite, logp = -inf, no flag;
      'dead'   d2 may come out positive, but then no larger than d2 + bound, and w_n^2 =
               (r_j - dv)^2 / d2 is so large that SS' < 0 for every such d2: logp = -inf, by
               either verdict (not positive definite, or bad_ss);
      None     neither can be shown: the case is no use for the test."""
    k, g, j = c["k"], c["g"], jbase + lane
    col = c["V"][g, g[pos]] * c["sv"]                       # f64 products, as the kernel gathers them
    x = F.forward(c["Lv"], col[:, None])[:, 0]
    nv, dv = x @ x, x @ c["w"].astype(LD)
    t_nv = 8 * k * U * c["kv"] * float(nv)
    t_dv = 8 * k * U * c["kv"] * float(np.sqrt(nv)) * float(np.linalg.norm(c["w"]))
    vjj = LD(c["V"][g[pos], g[pos]] * c["sv"])
    d2_hi = vjj - nv + t_nv + U * (abs(vjj) + nv)
    if d2_hi <= 0:
        return "notpd"
    ref = F.reference(c["p"], k, c["kind"], jbase)          # A's column is the lane's own
    ab, t_ab = LD(ref["sums"][3][lane]), F.tolerances(c, ref)[3][lane]
    rj = LD(c["xty"][j] * c["sx"]) + ab
    num = abs(rj - dv) - t_dv - t_ab - U * (abs(rj) + abs(ab))
    _, _, _, _, Q, cc = [LD(v) for v in c["model"]]
    if num > 0 and LD(c["ss0q"]) + cc - Q - num * num / d2_hi < -1e-6 * (c["ss0q"] + abs(cc) + abs(Q)):
        return "dead"
    return None


def numpy_eval_sums(c, jbase):
    """the four sums in plain f64 numpy (f64 forward substitution on the f64 factor)"""
    ref = F.reference(c["p"], c["k"], c["kind"], jbase)
    xv, xa = F.forward(c["Lv"], ref["bv"], np.float64), F.forward(c["La"], ref["ba"], np.float64)
    return F.sums(xv, xa, ref["ba"], c["w"], c["bg"])


def numpy_eval(c, jbase):
    """big_eval's formula in f64 on numpy_eval_sums: logp per lane (-inf where no fast lane)"""
    nv, dv, na, ab = numpy_eval_sums(c, jbase)
    _, lp, ldv, lda, Q, cc = c["model"]
    h = 0.5 * c["DF"] - 1.0
    out = np.full(64, -INF)
    for lane in range(64):
        j = jbase + lane
        if j >= c["p"] or c["b"][j] != 0.0:
            continue
        if c["gamma"][j]:
            if c["k"] == 1:
                out[lane] = (lp + (c["l0"][j] - c["l1"][j])) - h * np.log(c["ss0q"])
                continue
            lpn = lp + (c["l0"][j] - c["l1"][j])
            Qn = Q - dv[lane] * dv[lane] / nv[lane]
            ldvn, ldan = ldv + np.log(nv[lane]), lda + np.log(na[lane])
        else:
            lpn = lp + (c["l1"][j] - c["l0"][j])
            d2 = c["V"][j, j] * c["sv"] - nv[lane]
            da2 = c["A"][j, j] * c["sa"] - na[lane]
            wn = ((c["xty"][j] * c["sx"] + ab[lane]) - dv[lane]) / np.sqrt(d2)
            Qn, ldvn, ldan = Q + wn * wn, ldv + np.log(d2), lda + np.log(da2)
        out[lane] = lpn + 0.5 * (ldan - ldvn) - h * np.log(c["ss0q"] + cc - Qn)
    return out


# ---- tiles --------------------------------------------------------------------------------------
def tile_input(kk, kind):
    """a 64 x 64 SPD tile: the leading principal block of the case's sv V_g (k = 64)"""
    return np.ascontiguousarray(build_case(64, kind)["Mv"])
