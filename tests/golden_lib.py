"""The fixtures under tests/golden/ as the tests read them."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def _golden_mix(g):
    return dict(counts=g["mix_counts"], ncomp=g["mix_ncomp"], mu=g["mix_mu"], sigma=g["mix_sigma"],
                weight=g["mix_weight"], largest_index=int(g["mix_largest_index"]))
