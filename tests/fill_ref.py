"""Cases, model blocks and the high-precision reference for the table fill's triangular solves
(boom_amd/csrc/ssvs_fill_mfma.h: diag_inverses, mf_proposal_sums; ssvs_device.h: solve_blocks).

A case is what one chain's model looks like to a fill: the shared SPD matrices V and A (p x p),
the sorted index list g of the k included variables (spread evenly over 0 .. p - 1, so that
every 64-proposal window holds adds and -- from k = 3 on -- drops), the chain's scales sv, sa
(not 1), the f64 Cholesky factors of sv V_g and sa A_g, and the weights w and b_g.

block() lays that model out as the product's model block (ssvs_scalar_layout), holding what
the product leaves there and NaN wherever the fill's header says a thing "is not there":
  * factor rows k .. kpad8 - 1: ZEROS in their lower triangle and rd = 0 -- the rebuild gathers
    the padding rows as zeros (refactor: `if (m < k) ... else v = 0`, and again after one flip),
    the factorisation's column loop never touches a row >= k, and the large-model build stores
    `valid ? ... : 0.0` for row < kpad8; publish_model copies the whole blocks of kpad8 rows;
  * factor rows >= kpad8 and the upper triangles of the diagonal 8 x 8 blocks: never written: NaN;
  * rd at >= kpad8: NaN;
  * w and b_g at EVERY index >= k: NaN.  The product writes zeros at k .. kpad8 - 1 (and up to
    the capacity in the large-model build), but the fill masks its weights at k itself, so it
    may not depend on them: the block is hostile where it may be.  (zero_pad=True gives the
    product's zeros: the per-lane route's caller multiplies its zero solution by them.)
  * the scalars, the block's copy of g, S.iv / S.ia: NaN (the fill takes g from LDS).

The reference is forward substitution in numpy.longdouble on the same f64 factor."""
import functools

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
P_FULL, P_ODD = 192, 150          # a window at jbase = 128 overruns P_ODD
SV, SA = 0.37, 1.9
MF_ROWS = 16
FAST, ADD = 1, 2

# (instance MAXNI, capacity, k): every edge of mf_block_rows and of kpad8
SUMS_CASES = ([(3, 48, k) for k in (1, 7, 8, 9, 16, 17, 32, 33, 40, 41, 48)] +
              [(4, 64, k) for k in (17, 49, 56, 57, 64)] +
              [(8, 128, k) for k in (65, 80, 81, 96, 97, 112, 113, 128)])
# (p, jbase) of the windows every case is run at
WINDOWS = ((P_FULL, 0), (P_FULL, 64), (P_FULL, 128), (P_ODD, 128))
KINDS = ("well", "ill")


def bidx(m, n):
    """offset of element (m, n), n <= m, in the block-packed factor (ssvs_device.h)"""
    I, J = m >> 3, n >> 3
    return ((I * (I + 1)) // 2 + J) * 64 + (m & 7) * 8 + (n & 7)


def block_rows(k):
    """mf_block_rows"""
    return 2 if k <= 32 else 3 if k <= 48 else 4 if k <= 64 else 5 if k <= 80 else 6 if k <= 96 else 8


def layout(kcap):
    """ssvs_scalar_layout (ssvs_params.h), offsets in doubles; the GPU test checks it against
    the product's"""
    nb = kcap // 8
    fac = nb * (nb + 1) // 2 * 64
    o, S = 0, {}
    for name, size in (("Lv", fac), ("La", fac), ("rdv", kcap), ("rda", kcap), ("w", kcap), ("bg", kcap),
                       ("g", kcap // 2), ("scal", 8), ("iv", kcap * 16), ("ia", kcap * 16)):
        S[name] = o
        o += size
    S["total"] = (o + 7) & ~7
    return S


@functools.lru_cache(maxsize=None)
def matrices(p, kind):
    """(V, A): SPD p x p.  well: sample covariances of 4 p independent rows plus the identity;
    ill: equicorrelated columns (rho = 1 - delta) plus the ridge delta on the diagonal, rows and
    columns scaled by factors in [0.5, 2] -- kappa_2 of a k x k principal block ~ k / delta"""
    rng = np.random.Generator(np.random.PCG64(1000 * p + (kind == "ill")))
    out = []
    for delta in (1e-4, 3e-4):
        if kind == "well":
            X = rng.standard_normal((4 * p, p))
            M = X.T @ X / (4 * p) + np.eye(p)
        else:
            d = np.exp(rng.uniform(np.log(0.5), np.log(2.0), p))
            M = ((1.0 - delta) * np.ones((p, p)) + delta * np.eye(p)) * np.outer(d, d)
        out.append(np.ascontiguousarray(0.5 * (M + M.T)))
    return tuple(out)


def index_list(p, k):
    g = np.array([int((i + 0.5) * p / k) for i in range(k)], np.int32)
    assert np.all(np.diff(g) > 0) and g[-1] < p
    return g


@functools.lru_cache(maxsize=None)
def case(p, k, kind):
    V, A = matrices(p, kind)
    g = index_list(p, k)
    rng = np.random.Generator(np.random.PCG64(7 * p + 131 * k + (kind == "ill")))
    Lv = np.linalg.cholesky(SV * V[np.ix_(g, g)])
    La = np.linalg.cholesky(SA * A[np.ix_(g, g)])
    c = dict(p=p, k=k, kind=kind, V=V, A=A, g=g, sv=SV, sa=SA, Lv=Lv, La=La,
             w=rng.standard_normal(k), bg=rng.standard_normal(k),
             kv=float(np.linalg.cond(Lv)), ka=float(np.linalg.cond(La)))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def flags(c, jbase):
    """one wavefront's flags: lanes past p are nothing (0, as the product's `valid` makes them);
    every ninth variable is not fast (its add bit as the product computes it, whatever `fast`
    says) -- never g[0], whose drop the padded rows' gathers aim at; the rest are adds (j not
    in g) and drops (j in g)"""
    p, g = c["p"], c["g"]
    f = np.zeros(64, np.int32)
    for lane in range(64):
        j = jbase + lane
        if j >= p:
            continue
        add = j not in g
        fast = not (j % 9 == 4 and j != g[0])
        f[lane] = (FAST if fast else 0) | (ADD if add else 0)
    return f


def rhs(c, jbase, fl):
    """(B_V, B_A): k x 64 right-hand sides of the fast lanes (f64, exact: one product each);
    columns of other lanes are zero"""
    g, k = c["g"], c["k"]
    bv, ba = np.zeros((k, 64)), np.zeros((k, 64))
    for lane in range(64):
        if not fl[lane] & FAST:
            continue
        j = jbase + lane
        if fl[lane] & ADD:
            bv[:, lane] = c["V"][g, j] * c["sv"]
            ba[:, lane] = c["A"][g, j] * c["sa"]
        else:
            e = (g == j).astype(np.float64)
            bv[:, lane] = e
            ba[:, lane] = e
    return bv, ba


def forward(L, B, dtype=LD):
    """L^{-1} B by forward substitution in `dtype`"""
    L = L.astype(dtype)
    X = np.array(B, dtype=dtype)
    for i in range(L.shape[0]):
        if i:
            X[i] -= L[i, :i] @ X[:i]
        X[i] /= L[i, i]
    return X


def diag_inverse_blocks(L, k, nI, dtype=np.float64):
    """what diag_inverses computes, in its own order: column c of inv(L_II) by substitution with
    the reciprocal diagonal; rows and columns >= k zero.  nI x 16 x 16"""
    Lp = np.zeros((nI * MF_ROWS, nI * MF_ROWS), dtype)
    Lp[:k, :k] = L.astype(dtype)
    rd = np.zeros(nI * MF_ROWS, dtype)
    rd[:k] = dtype(1.0) / np.diag(L).astype(dtype)
    out = np.zeros((nI, MF_ROWS, MF_ROWS), dtype)
    for I in range(nI):
        o = MF_ROWS * I
        for c in range(MF_ROWS):
            x = np.zeros(MF_ROWS, dtype)
            for r in range(c, MF_ROWS):
                if r == c:
                    x[r] = rd[o + r]
                else:
                    acc = dtype(0.0)
                    for s in range(r):
                        acc += Lp[o + r, o + s] * x[s]
                    x[r] = -acc * rd[o + r]
            out[I, :, c] = x
    return out


def blocked(L, B, k):
    """f64 emulation of the blocked order: X_I = inv(L_II) (B_I - sum_{J < I} L_IJ X_J) with
    the inverse diagonal blocks of diag_inverse_blocks (rows padded to whole blocks of 16)"""
    nI = block_rows(k)
    n = nI * MF_ROWS
    inv = diag_inverse_blocks(L, k, nI)
    Lp = np.zeros((n, n))
    Lp[:k, :k] = L
    X = np.zeros((n, B.shape[1]))
    X[:k] = B
    for I in range(nI):
        r = slice(MF_ROWS * I, MF_ROWS * (I + 1))
        acc = X[r].copy()
        for J in range(I):
            cj = slice(MF_ROWS * J, MF_ROWS * (J + 1))
            acc -= Lp[r, cj] @ X[cj]
        X[r] = inv[I] @ acc
    return X[:k]


def sums(xv, xa, ba, w, bg):
    """(nv, dv, na, ab) per column, in the dtype of the solutions"""
    t = xv.dtype.type
    return ((xv * xv).sum(0), (xv * w.astype(t)[:, None]).sum(0), (xa * xa).sum(0),
            (ba.astype(t) * bg.astype(t)[:, None]).sum(0))


@functools.lru_cache(maxsize=None)
def reference(p, k, kind, jbase):
    """longdouble reference of one window: dict(flags, bv, ba, xv, xa, sums=(nv, dv, na, ab))"""
    c = case(p, k, kind)
    fl = flags(c, jbase)
    bv, ba = rhs(c, jbase, fl)
    xv, xa = forward(c["Lv"], bv), forward(c["La"], ba)
    return dict(flags=fl, bv=bv, ba=ba, xv=xv, xa=xa, sums=sums(xv, xa, ba, c["w"], c["bg"]))


def tolerances(c, ref):
    """per column: the bounds on |nv - ref|, |dv - ref|, |na - ref|, |ab - ref| -- the forward
    error of substitution, gamma_k cond, with the factor 8 for the block-inverse variant and
    the squared norm; ab involves no solve"""
    k = c["k"]
    nv, _, na, _ = [np.asarray(s, np.float64) for s in ref["sums"]]
    nxv = np.sqrt(nv)
    nba = np.linalg.norm(ref["ba"], axis=0)
    return (8 * k * U * c["kv"] * nv, 8 * k * U * c["kv"] * nxv * np.linalg.norm(c["w"]),
            8 * k * U * c["ka"] * na, 8 * k * U * nba * np.linalg.norm(c["bg"]))


def exact_inverse_blocks(L, k):
    """exact (longdouble) inverse of each 16 x 16 diagonal block, rows and columns >= k zero"""
    nI = block_rows(k)
    out = np.zeros((nI, MF_ROWS, MF_ROWS), LD)
    for I in range(nI):
        o = MF_ROWS * I
        kk = min(max(k - o, 0), MF_ROWS)
        if kk:
            out[I, :kk, :kk] = forward(L[o:o + kk, o:o + kk], np.eye(kk))
    return out


def block(c, kcap, zero_pad=False):
    """the model block of capacity kcap as the product leaves it (see the module's docstring)"""
    S, k = layout(kcap), c["k"]
    kpad8 = (k + 7) & ~7
    assert k <= kcap
    b = np.full(S["total"], np.nan)
    for name, L in (("Lv", c["Lv"]), ("La", c["La"])):
        for m in range(kpad8):
            for n in range(m + 1):
                b[S[name] + bidx(m, n)] = L[m, n] if m < k else 0.0
    for name, L in (("rdv", c["Lv"]), ("rda", c["La"])):
        b[S[name]:S[name] + k] = 1.0 / np.diag(L)
        b[S[name] + k:S[name] + kpad8] = 0.0
    b[S["w"]:S["w"] + k] = c["w"]
    b[S["bg"]:S["bg"] + k] = c["bg"]
    if zero_pad:
        b[S["w"] + k:S["w"] + kpad8] = 0.0
        b[S["bg"] + k:S["bg"] + kpad8] = 0.0
    return b
