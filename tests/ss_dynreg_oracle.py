"""A restatement of the state half of StateSpacePosteriorSampler::draw() for a list of state models that
holds DynamicRegressionStateModel blocks with the independent random-walk sampler (StateModels/
DynamicRegressionStateModel.cpp, bsts AddDynamicRegression with DynamicRegressionRandomWalkOptions;
ba_ss_add_dynamic_regression), on the device's substreams, one chain: the parity yardstick of the general
structural kernel's DR instances.  The recursion is tests/ss_state_models_oracle.py's, where the dynamic
regression is the class DynamicRegression; this file states the model, builds its block and passes that
file's names on.

The dynamic regression block (d coefficients, predictors x_t for every time t):
  T_t = I;  Z_t = x_t on the block's components;  RQR_t = diag(sigma_1^2 .. sigma_d^2), every step;
  observe_state(then, now, t), t = 1 .. T - 1: (now[i] - then[i])^2 into coefficient i's sum, n = T - 1 each;
  initial state rmvn_mt(mean, diagonal variance): d standard normals, sqrt(P0) z + a0;
  one GenericGaussianVarianceSampler(ChisqModel(df_i, guess_i)) with a sigma upper limit per coefficient.

CONVENTIONS (the device's; BOOM draws the d variances from one generator): variance i of the block reads
sampler id 10 + 16 x (the dynamic coefficients ahead of it in the list); the block reads d standard normals
of stream 2 per step t >= 1, scaled by sigma_i, whatever the sigmas.

forecast(): forecast step i advances the block with d errors (rnorm(0, sigma_i), in order) and observes
the new state with row T + i of the predictors.
"""
import numpy as np

from ss_state_models_oracle import (DYNREG, Structure, block_stream_ids, f64, forecast,  # noqa: F401
                                    impute_state, simulate_forward, state_model_suf)
from ss_state_models_oracle import StateOracle as DynRegOracle  # noqa: F401


def dynreg_block(predictors, sdy, initial_sigma=None, a0=None):
    """a dynamic regression block dict with bsts-style defaults per coefficient: sd prior guess 0.01 sd(y),
    df 0.01, upper limit sd(y); initial state N(a0 or 0, sd(y)^2)"""
    x = f64(predictors)
    d = x.shape[1]
    sig = np.full(d, 0.3) if initial_sigma is None else f64(initial_sigma)
    return dict(kind=DYNREG, dim=d, predictors=x, nseasons=0, duration=1, t0=0, lags=0, df=np.full(d, 0.01),
                sigma_guess=np.full(d, 0.01 * sdy), sigma_upper_limit=np.full(d, sdy), initial_sigma=sig,
                initial_phi=np.zeros(0), a0=np.zeros(d) if a0 is None else f64(a0), P0=np.full(d, sdy * sdy))
