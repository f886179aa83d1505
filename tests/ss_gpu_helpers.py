"""What the GPU tests of the state models share word for word: the refusal check, and the engine and the
comparison of the random-walk holiday's and the dynamic regression's tests.  (The engines of the regression
holiday's, the autoregression's and the Student trend's tests differ and stay in their files.)"""
import numpy as np
import pytest

from cases import bsts_priors

RTOL = 1e-8


def refused(fn, text):
    """fn() raises BoomAmdError with `text` in its message"""
    import boom_amd
    with pytest.raises(boom_amd.BoomAmdError) as e:
        fn()
    assert text in str(e.value), str(e.value)


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return bool(np.all(np.abs(a - b) <= rtol * np.abs(b)))


def engine(chains, seed, y, X, obs, blocks, g0, kernel=None):
    """an engine on the data with bsts-style regression priors (expected model size 2) and the list `blocks`"""
    import boom_amd
    prior, _, sig_up = bsts_priors(X, y, 2)
    eng = boom_amd.Engine(chains, seed=seed)
    eng.ss_set_data(y, X, obs)
    eng.set_priors(prior["b"], prior["ominv"], prior["pi"], prior["df"], prior["sigma_guess"],
                   sigma_upper_limit=sig_up)
    eng.ss_set_state_models(blocks)
    if kernel is not None:
        eng.ss_set_tuning(kernel=kernel)
    eng.set_state(g0)
    return eng
