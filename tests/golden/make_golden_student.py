"""Generates tests/golden/student_*.npz: TRegressionSpikeSlabSampler of the COMPILED,
UNMODIFIED reference (oracle/ref_driver.cpp: ref_student_run).  Build container only (see
make_golden.py).  Each fixture holds the data, the priors, the options and the starting
state, and per sweep gamma, beta, sigma^2, nu and the complete-data suf's sum of weights,
y'Wy and X'Wy."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from cases import student_data  # noqa: E402
from make_golden import save  # noqa: E402
from oracle_lib import Ref  # noqa: E402

NSWEEPS = 60
UNIFORM, GAMMA = (0, 0.1, 100.0), (1, 2.0, 0.1)

# name: data (n, p, nsig, seed, error df), the sampler's seed and options
CASES = {
    # t_3 errors, nu ~ Uniform(0.1, 100)
    "student_base": dict(data=(300, 10, 3, 100, 3.0), seed=17),
    # nu ~ Gamma(2, 0.1), at most 6 flips a sweep
    "student_gamma_maxflips": dict(data=(400, 24, 5, 101, 3.0), seed=18, nu_prior=GAMMA,
                                   max_flips=6),
    # sigma <= 0.45, far below the posterior's scale: the truncated draw beyond the mode
    "student_sigma_limit": dict(data=(300, 12, 4, 102, 3.0), seed=19, sigma_max=0.45),
    # a slab mean away from 0 and at most 3 variables in the model
    "student_slab_mean_max_size": dict(data=(300, 14, 4, 103, 3.0), seed=20, mu=0.3,
                                       max_model_size=3),
    # allow_model_selection(false): gamma stays at its start
    "student_no_selection": dict(data=(300, 12, 4, 104, 3.0), seed=21, allow_selection=False,
                                 init=(0, 2, 5)),
    # more than 64 variables in the model
    "student_p72": dict(data=(200, 72, 70, 105, 3.0), seed=22, pi=0.97, init="all"),
    # errors heavier than Cauchy's: nu goes below 1 (the weights' shape (nu + 1) / 2 < 1)
    "student_heavy_tails": dict(data=(300, 8, 3, 106, 0.7), seed=23, init_nu=2.0),
    # Gaussian errors: nu against the Uniform prior's upper bound (log f(hi) = -inf)
    "student_gaussian": dict(data=(400, 8, 3, 107, np.inf), seed=24, init_nu=60.0),
    # a non-default starting beta, sigma^2 and nu
    "student_start": dict(data=(300, 12, 3, 108, 3.0), seed=25, init=(0, 1, 2),
                          init_beta=True, init_sigsq=1.7, init_nu=4.5),
}


def case_arrays(spec):
    """the data, priors and starting state of a case (also what the fixture stores)"""
    n, p, nsig, dseed, df = spec["data"]
    X, y, _ = student_data(n, p, nsig, dseed, df=df)
    mu = np.full(p, spec.get("mu", 0.0))
    prec = 0.1 * np.eye(p)
    pi = np.full(p, spec.get("pi", min(0.9, 5.0 / p)))
    init = spec.get("init", (0, 1))
    g0 = np.ones(p, np.uint8) if init == "all" else np.zeros(p, np.uint8)
    if init != "all":
        g0[list(init)] = 1
    b0 = np.linspace(0.5, 1.5, p) * g0 if spec.get("init_beta") else np.zeros(p)
    return dict(X=X, y=y, mu=mu, prec=prec, pi=pi, seed=spec["seed"], init_gamma=g0,
                init_beta=b0, init_sigsq=spec.get("init_sigsq", 1.0),
                init_nu=spec.get("init_nu", 30.0),
                nu_prior=np.array(spec.get("nu_prior", UNIFORM), dtype=float),
                sigma_prior=np.array([1.0, 1.0]), sigma_max=spec.get("sigma_max", np.inf),
                max_model_size=spec.get("max_model_size", -1),
                max_flips=spec.get("max_flips", -1),
                allow_selection=int(spec.get("allow_selection", True)), nsweeps=NSWEEPS)


def main():
    R = Ref()
    for name, spec in CASES.items():
        a = case_arrays(spec)
        nup = a["nu_prior"]
        o = R.student_run(a["X"], a["y"], a["mu"], a["prec"], a["pi"], a["seed"], a["init_gamma"],
                          NSWEEPS, init_beta=a["init_beta"], init_sigsq=a["init_sigsq"],
                          init_nu=a["init_nu"], nu_prior=(int(nup[0]), nup[1], nup[2]),
                          sigma_prior=tuple(a["sigma_prior"]), sigma_max=a["sigma_max"],
                          max_model_size=a["max_model_size"], max_flips=a["max_flips"],
                          allow_selection=bool(a["allow_selection"]))
        save(name, **a, **o)


if __name__ == "__main__":
    main()
