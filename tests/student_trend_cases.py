"""Cases of the Student local linear trend state model (kind 8, bsts AddStudentLocalLinearTrend) for
general_spec-style block lists, shared by tests/test_student_trend_cpu.py and
tests/test_student_trend_gpu.py."""
import numpy as np

from cases import general_data, general_spec

KIND_STUDENT_TREND = 8
BSTS_NU_PRIOR = (0, 1.0, 500.0)   # bsts's default: uniform(1, 500)


def student_trend_spec(y, desc, nu_priors=(BSTS_NU_PRIOR, BSTS_NU_PRIOR), initial_nu=(5.0, 5.0)):
    """general_spec with ("student_trend",) entries: the block as general_spec makes a ("trend",), with
    kind 8, the two nu priors (kind, a, b) and the initial (nu_level, nu_slope)"""
    where = [i for i, b in enumerate(desc) if b[0] == "student_trend"]
    blocks = general_spec(y, [("trend",) if b[0] == "student_trend" else b for b in desc])
    for i in where:
        blocks[i] = dict(blocks[i], kind=KIND_STUDENT_TREND, nu_priors=[tuple(nu_priors[0]), tuple(nu_priors[1])],
                         initial_nu=np.array(initial_nu, dtype=float))
    return blocks


def as_plain_trend(blocks, scale=(1.0, 1.0)):
    """the same list with the Student trend as a local linear trend (kind 2) whose initial variances are
    those of the Student trend divided by `scale` (level, slope)"""
    out = []
    for b in blocks:
        if b["kind"] == KIND_STUDENT_TREND:
            b = {k: v for k, v in b.items() if k not in ("nu_priors", "initial_nu")}
            b = dict(b, kind=2, initial_sigma=np.asarray(b["initial_sigma"], float) / np.sqrt(np.asarray(scale, float)))
        out.append(b)
    return out


def chain_parameters(p, chains, seed):
    rs = np.random.Generator(np.random.PCG64(seed))
    gam = (rs.uniform(size=(chains, p)) < 0.6).astype(np.uint8)
    gam[:, 0] = 1
    return gam, rs.standard_normal((chains, p)) * gam


# The regression-free loop: 12 x (ba_ss_trend_draw_parameters; ba_ss_impute_state) with gamma, beta and
# sigma^2 fixed.  [student trend, seasonal(4)], T = 40.  Case 0 starts on NuPosteriorFast (nu = 5) with
# finite sigma upper limits and bsts's uniform nu prior; case 1 on NuPosteriorRobust (nu = 30) with a
# gamma nu prior and no upper limit.  The loop's first parameter draw comes before any state draw, from
# the prior alone: with bsts's 0.01 prior degrees of freedom and no upper limit that sigma^2 is of the
# order 1e100 and the state draw behind it has no digits left to compare, so the case without a limit has
# a prior of 3 degrees of freedom.  The seeds are pinned by tests/test_student_trend_cpu.py: every
# slice comparison of the restatement has a relative margin above 1e-9 on the checked chains.
LOOP_CASES = [
    dict(seed=1201, data_seed=61, nu0=(5.0, 5.0), nu_priors=(BSTS_NU_PRIOR, BSTS_NU_PRIOR), upper=None),
    dict(seed=1202, data_seed=62, nu0=(30.0, 30.0), nu_priors=((1, 2.0, 0.1), (1, 2.0, 0.1)), upper=np.inf),
]
LOOP_ROUNDS, LOOP_T, LOOP_P, LOOP_CHAINS, LOOP_SIGSQ = 12, 40, 3, 4, 0.5
LOOP_CHECK = [0, LOOP_CHAINS - 1]


def loop_case(k):
    c = LOOP_CASES[k]
    T, p = LOOP_T, LOOP_P
    X, y, _, _ = general_data(T, p, 2, [(4, 1)], seed=c["data_seed"])
    rs = np.random.Generator(np.random.PCG64(c["data_seed"] + 1000))
    y = y + np.cumsum(np.where(rs.uniform(size=T) < 0.1, 4.0 * rs.standard_normal(T), 0.0))   # a few level shifts
    blocks = student_trend_spec(y, [("student_trend",), ("seasonal", 4, 1)], c["nu_priors"], c["nu0"])
    if c["upper"] is not None:
        for b in blocks:
            b["sigma_upper_limit"] = np.full(len(b["df"]), c["upper"])
            if np.isinf(c["upper"]):
                b["df"] = np.full(len(b["df"]), 3.0)
    gam, beta = chain_parameters(p, LOOP_CHAINS, c["data_seed"] + 7)
    return dict(c, T=T, p=p, X=X, y=y, obs=None, blocks=blocks, gam=gam, beta=beta, sigsq=LOOP_SIGSQ,
                chains=LOOP_CHAINS, check=LOOP_CHECK, rounds=LOOP_ROUNDS)


def loop_oracle(o, case, chain):
    """the restatement of one chain of a loop case, and its adjusted series y - X beta"""
    import ss_student_trend_oracle as sto
    inc = np.flatnonzero(case["gam"][chain])
    ystar = case["y"] - case["X"][:, inc] @ case["beta"][chain][inc]
    return sto.StudentTrendOracle(o, case["T"], case["obs"], case["blocks"], case["seed"], chain), ystar
