"""The multi-output test problem of the pruned top-k sweep over independent outputs (gpx_acquire_topk_multi_f64), and
the CPU replay of its bound with the oracle.  Shared by tests/test_gpu_topk_multi.py and tests/test_topk_multi_host.py.

Problem: X, y0 = synthetic_problem(n, d, 21); output 0 is y0, output t >= 1 is cos(4 X a_t + t) + 0.3 y0 with a_t drawn
from default_rng(5), every column standardised by its own mean and std.  Kernels (rbf, matern52,
scale_linear_matern52) cycled over the outputs, each with its own lengthscale, outputscale, noise and constant mean.
Objective weights 1 / T, y_mean = 0.1 t, y_scale = 1 + 0.5 t, best_f the best observed objective value, beta = 4,
candidates sobol_candidates(5000, d, 22)."""
from functools import lru_cache

import numpy as np
import scipy.linalg as sla

from bayesianoptimizer_amd import KernelParams, botorch_default_lengthscale
from oracle import gp_oracle as O
from tests.ard_util import ard_values
from tests.oracle_engine import to_oracle_params

KINDS = ["rbf", "matern52", "scale_linear_matern52"]
ACQS = ["ei", "logei", "ucb", "variance"]
OACQ = {"ei": O.ACQ_EI, "logei": O.ACQ_LOGEI, "ucb": O.ACQ_UCB, "variance": O.ACQ_VARIANCE}
D, M, BETA = 4, 5000, 4.0
SEED_BLOCK, HEAD_ROWS = 1024, 128  # PRUNE_SEED, PRUNE_HEAD_ROWS of csrc/gpx_sweep_layout.h


@lru_cache(maxsize=None)
def problem(n, T=3, d=D, kinds=None, cov_fp32=(), ard=False):
    """dict(X, Y, params, w, ym, ys, best_f): never modified by its users.  kinds: a tuple of kernel kinds to cycle
    instead of KINDS; cov_fp32: the outputs built with the fp32 covariance; ard: output t takes the per-dimension
    lengthscales and linear variances of tests/ard_util.py with seed d + t (a different set per output) in place of
    the scalar ones."""
    X, y0 = O.synthetic_problem(n, d, 21)
    rng = np.random.default_rng(5)
    cols = [y0] + [np.cos(4.0 * X @ rng.random(d) + t) + 0.3 * y0 for t in range(1, T)]
    Y = np.stack([(c - c.mean()) / c.std() for c in cols], axis=1)
    kinds = kinds or tuple(KINDS)
    params = [KernelParams(kinds[t % len(kinds)], botorch_default_lengthscale(d) * (0.8 + 0.2 * t),
                           outputscale=1.0 + 0.25 * t, noise=1e-4 * (1 + t), const_mean=0.05 * t, linear_variance=0.3,
                           cov_fp32=t in cov_fp32) for t in range(T)]
    if ard:
        for t in range(T):
            ls, lv = ard_values(d, d + t)
            params[t] = params[t].replace(lengthscale=[float(v) for v in ls], linear_variance=[float(v) for v in lv])
    w = [1.0 / T] * T
    ym = [0.1 * t for t in range(T)]
    ys = [1.0 + 0.5 * t for t in range(T)]
    best_f = float(((Y * np.array(ys) + np.array(ym)) @ np.array(w)).max())
    for a in (X, Y):
        a.setflags(write=False)
    return dict(X=X, Y=Y, params=params, w=w, ym=ym, ys=ys, best_f=best_f)


@lru_cache(maxsize=None)
def candidates(m=M, d=D):
    Xs = O.sobol_candidates(m, d, 22)
    Xs.setflags(write=False)
    return Xs


@lru_cache(maxsize=None)
def _replay_moments(n, T):
    """(objective mean, exact variance, variance from the head rows of every output) of the candidates, by the oracle:
    per output the GPyTorch floor on the standardised variance, weighted by w_t^2 y_scale_t^2 and summed."""
    pr = problem(n, T)
    Xs = candidates()
    mu = np.zeros(len(Xs))
    var = np.zeros(len(Xs))
    var_ub = np.zeros(len(Xs))
    for t in range(T):
        p = to_oracle_params(pr["params"][t], D)
        st = O.fit(pr["X"], pr["Y"][:, t], p)
        Ks = O.kernel_matrix(pr["X"], Xs, p)
        V = sla.solve_triangular(st.L, Ks, lower=True, check_finite=False)
        kd = O.kernel_diag(Xs, p)
        c = (pr["w"][t] * pr["ys"][t]) ** 2
        mu += pr["w"][t] * (pr["ym"][t] + pr["ys"][t] * (p.const_mean + Ks.T @ st.alpha))
        var += c * np.maximum(kd - np.einsum("ij,ij->j", V, V), O.GPYTORCH_MIN_VAR_F64)
        var_ub += c * np.maximum(kd - np.einsum("ij,ij->j", V[:HEAD_ROWS], V[:HEAD_ROWS]), O.GPYTORCH_MIN_VAR_F64)
    return mu, var, var_ub


def oracle_survivors(n, acq, k, T=3):
    """Staged candidates (behind the seed block) whose bound, scored from the head rows' variance, still reaches the
    incumbent: the k-th best exact score of the seed block."""
    pr = problem(n, T)
    mu, var, var_ub = _replay_moments(n, T)
    floor = O.BOTORCH_MIN_VAR
    exact = O.acquisition(mu, np.maximum(var, floor), OACQ[acq], pr["best_f"], BETA)
    ub = O.acquisition(mu, np.maximum(var_ub, floor), OACQ[acq], pr["best_f"], BETA)
    tau = np.sort(exact[:SEED_BLOCK])[::-1][k - 1]
    return int((ub[SEED_BLOCK:] >= tau).sum())
