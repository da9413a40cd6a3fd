"""Stand-in for information_theory.information (un-vendored), as far as
src/VQ.py uses it.  Assumption A14 (unpinned): energy(x)
is the sum of the squared samples, accumulated in float64."""
import numpy as np


def energy(x):
    x = np.asarray(x, dtype=np.float64)
    return np.sum(x * x)
