"""Which data an engine holds decides which sweep entry point runs: the whole matrix
(entry point x data kind) of refusals, text included, and the walk through every kind on ONE
engine -- after each data setter exactly the new kind's sweep runs.

The expected texts are the C-ABI's contract (every refusal is BA_E_STATE); an engine per kind
first, then the transitions regression -> probit -> Poisson -> logit -> Student -> state space
-> regression on one engine.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BA_E_STATE = -9
N, P, T, CHAINS = 200, 5, 50, 4

SS = "state-space data are set: use ba_ss_sweep"
S = "Student-t regression data are set: use ba_student_sweep"
B1 = ("binomial data are set: use ba_logit_sweep / ba_probit_sweep (the regression sampler has "
      "no meaning on latent data)")
B2 = ("binomial data are set: use ba_logit_sweep / ba_probit_sweep (a sweep without the "
      "imputation is not a draw of those samplers)")
PO = "Poisson data are set: use ba_poisson_sweep"
FIRST = {k: "call ba_%s_set_data first" % k for k in ("probit", "logit", "poisson", "student", "ss")}

KINDS = ("regression", "state_space", "probit", "logit", "poisson", "student")
# entry point -> the refusal per data kind, in the order of KINDS (None: it runs)
MATRIX = {
    "sweep": (None, SS, B1, B1, B1, S),
    "draw_next": (None, SS, B1, B1, B1, S),
    "adaptive_sweep": (None, SS, B1, B1, B1, S),
    "sss_sweep": (None, SS, B2, B2, B2, S),
    "probit_sweep": (FIRST["probit"],) * 2 + (None,) + (FIRST["probit"],) * 2 + (S,),
    "logit_sweep": (FIRST["logit"],) * 3 + (None, PO, S),
    "poisson_sweep": (FIRST["poisson"],) * 4 + (None, S),
    "student_sweep": (FIRST["student"], SS, "binomial data are set: use ba_probit_sweep",
                      "binomial data are set: use ba_logit_sweep", PO, None),
    "ss_sweep": (FIRST["ss"], None) + (FIRST["ss"],) * 4,
    "ss_draw_next": (FIRST["ss"], None) + (FIRST["ss"],) * 4,
}


def data():
    from cases import student_data
    X, y, _ = student_data(N, P, 2, 1)
    return X, y


def install(eng, kind, X, y):
    """the data of `kind`, then the priors and the state its sampler needs"""
    mu, prec, pi = np.zeros(P), np.eye(P), np.full(P, 0.5)
    binary = (y > 0).astype(float)
    if kind == "regression":
        eng.build_suf_from_xy(X, y)
    elif kind == "state_space":
        eng.ss_set_data(y[:T], X[:T])
        eng.ss_set_local_level(1.0, 0.5, np.inf, 0.0, 1.0, 0.5)
    elif kind == "probit":
        eng.probit_set_data(X, binary, np.ones(N))
    elif kind == "logit":
        eng.logit_set_data(X, binary, np.ones(N))
    elif kind == "poisson":
        eng.poisson_set_data(X, np.ones(N), np.ones(N),
                             dict(counts=np.array([1]), ncomp=np.array([1]), mu=np.zeros(1),
                                  sigma=np.ones(1), weight=np.ones(1), largest_index=100))
    else:
        eng.student_set_data(X, y)
    # (the latent-data samplers of the binomial and Poisson families take a fixed-precision slab)
    eng.sss_set_slab(mu, prec, scales_with_sigsq=kind not in ("probit", "logit", "poisson"))
    eng.set_spike(pi)
    eng.set_state(np.zeros(P, np.uint8))


def call(eng, entry):
    fn = getattr(eng, entry)
    if entry.endswith("draw_next"):
        fn()
        eng.sync()
    else:
        fn(1)


def check_column(eng, kind):
    import boom_amd
    col = KINDS.index(kind)
    for entry, row in MATRIX.items():
        if row[col] is None:
            call(eng, entry)
            continue
        with pytest.raises(boom_amd.BoomAmdError) as ei:
            call(eng, entry)
        print("%-14s on %-11s: %s" % (entry, kind, ei.value))
        assert str(ei.value) == row[col], (entry, kind)
        assert ei.value.code == BA_E_STATE, (entry, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_refusal_matrix_one_engine_per_kind(kind):
    import boom_amd
    X, y = data()
    eng = boom_amd.Engine(CHAINS, seed=1)
    if kind == "regression":
        # a fresh engine holds no data: the families' sweeps ask for theirs
        for entry in ("probit_sweep", "logit_sweep", "poisson_sweep", "student_sweep", "ss_sweep",
                      "ss_draw_next"):
            with pytest.raises(boom_amd.BoomAmdError) as ei:
                call(eng, entry)
            assert str(ei.value) == MATRIX[entry][0], entry
    install(eng, kind, X, y)
    check_column(eng, kind)
    eng.close()


def test_poisson_sweep_asks_for_the_mixtures():
    import boom_amd
    from boom_amd.capi import _f64, _p
    X, _ = data()
    eng = boom_amd.Engine(CHAINS, seed=1)
    Xf = np.asfortranarray(X, dtype=np.float64)
    eng._check(eng.lib.ba_poisson_set_data(eng._h, N, P, _p(Xf), _p(_f64(np.ones(N))), _p(_f64(np.ones(N)))))
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.poisson_sweep(1)
    assert str(ei.value) == "call ba_poisson_set_mixtures first" and ei.value.code == BA_E_STATE
    # ... and the data are Poisson data all the same
    with pytest.raises(boom_amd.BoomAmdError) as ei:
        eng.logit_sweep(1)
    assert str(ei.value) == PO
    eng.close()


def test_transitions_on_one_engine():
    import boom_amd
    X, y = data()
    eng = boom_amd.Engine(CHAINS, seed=1)
    for kind in ("regression", "probit", "poisson", "logit", "student", "state_space", "regression"):
        install(eng, kind, X, y)
        check_column(eng, kind)
        g, b, s = eng.get_states()
        assert np.all(np.isfinite(b)) and np.all(s > 0), kind
    eng.close()
