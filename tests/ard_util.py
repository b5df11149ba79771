"""ARD kernel parameters for the tests: a different lengthscale and a different linear variance in every dimension, so
that a kernel which reads parameter k where it should read parameter col disagrees with its reference.

    ls_k = botorch_default_lengthscale(d) (0.5 + perm(k) / max(d - 1, 1))      0.5 to 1.5 of the default
    lv_k = 0.05 + 0.4 perm2(k) / max(d - 1, 1)                                  0.05 to 0.45

perm and perm2 are two permutations of range(d) drawn from default_rng(seed): the values are pairwise distinct, and at
d = 32 any two lengthscales differ by at least 1 / 31 = 3 % of the default.  tests/test_ard_host.py checks that the
oracle fits with them and that the yardsticks of the GPU tests reject two swapped entries by a wide margin.

LADDER holds, for each of the four DMAX instances (4, 8, 16, 32) of the d-dispatched kernels, its widest d and the next
instance's narrowest."""
from functools import lru_cache

import numpy as np

from bayesianoptimizer_amd import KernelParams, botorch_default_lengthscale
from oracle import gp_oracle as O
from tests.oracle_engine import to_oracle_params

LADDER = (4, 5, 8, 9, 16, 17, 32)
KINDS = ("rbf", "matern52", "scale_linear_matern52")
ACQS = {"ei": O.ACQ_EI, "logei": O.ACQ_LOGEI, "ucb": O.ACQ_UCB, "variance": O.ACQ_VARIANCE}
NOISE, BETA = 1e-4, 4.0


@lru_cache(maxsize=None)
def sweep_problem(n, d, m=5000):
    """(X, y, candidates) of the ARD sweep tests: the suite's synthetic_problem(n, d, 21) and sobol_candidates(m, d, 22),
    read-only.  best_f is y.max(), beta is BETA, the noise NOISE, the parameters ard_params(kind, d, d, noise=NOISE)."""
    X, y = O.synthetic_problem(n, d, 21)
    Xs = O.sobol_candidates(m, d, 22)
    for a in (X, y, Xs):
        a.setflags(write=False)
    return X, y, Xs


def ard_values(d, seed):
    """(lengthscales, linear variances) of the recipe above, two float64 vectors of length d."""
    rng = np.random.default_rng(seed)
    perm, perm2 = rng.permutation(d), rng.permutation(d)
    den = max(d - 1, 1)
    return botorch_default_lengthscale(d) * (0.5 + perm / den), 0.05 + 0.4 * perm2 / den


def ard_params(kind, d, seed, **kw):
    """(KernelParams, O.KernelParams) with the recipe's values: the ARD counterpart of test_gpu_parity.pair."""
    ls, lv = ard_values(d, seed)
    kp = KernelParams(kind, [float(v) for v in ls], linear_variance=[float(v) for v in lv], **kw)
    return kp, to_oracle_params(kp, d)


def swapped(kp, i, j, what="lengthscale"):
    """kp with entries i and j of its lengthscales (or linear variances) exchanged: the index mix-up the tests must see."""
    v = list(getattr(kp, what))
    v[i], v[j] = v[j], v[i]
    return kp.replace(**{what: v})


def swap_pairs(d):
    """(0, 1), (d - 2, d - 1) and, above 16 dimensions, (15, 16): the pair that straddles the two 16-dimension sweeps."""
    pairs = [(0, 1), (d - 2, d - 1)] + ([(15, 16)] if d > 16 else [])
    return sorted(set(pairs))
