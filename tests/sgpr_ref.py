"""NumPy restatement of the closed-form SVGP variational posterior (gpx_svgp_fit_collapsed_f64), project-first:
Phi = L_Z^{-1} K(Z, X) by a triangular solve, then B = I + Phi Phi^T / s2 and b = Phi r / s2.  Kernel, Cholesky and the
SVGP predictive come from oracle.gp_oracle.  Also the shapes and hyperparameters the host and GPU tests share."""
from dataclasses import dataclass

import numpy as np
import scipy.linalg as sla

from bayesianoptimizer_amd import KernelParams
from oracle import gp_oracle as O

JITTER = 1e-4
# n, M, d, T, input scale s (inputs s N(0, 1)), noise of task t
SHAPES = {
    1: (520, 130, 3, 1, 0.3, lambda t: 1e-2),
    2: (700, 200, 5, 3, 0.3, lambda t: 1e-3 * (t + 1)),
    3: (400, 130, 5, 2, 0.6, lambda t: 1e-2),
    4: (300, 64, 8, 8, 0.6, lambda t: 1e-3),
}


@dataclass
class Problem:
    X: np.ndarray      # n x d
    Y: np.ndarray      # n x T
    Z: np.ndarray      # T x M x d (the same random rows of X for every task)
    kps: list          # engine KernelParams per task
    ops: list          # oracle KernelParams per task


def problem(shape: int, seed: int = 0) -> Problem:
    """Hyperparameters as tests/test_svgp.py::svgp_problem: lengthscales 0.8-1.8, per-task noise and const_mean."""
    n, M, d, T, s, noise_of = SHAPES[shape]
    rng = np.random.default_rng(1000 * shape + seed)
    X = s * rng.standard_normal((n, d))
    Z1 = X[rng.choice(n, size=M, replace=False)]
    Z = np.repeat(Z1[None], T, axis=0)
    Y = np.empty((n, T))
    kps, ops = [], []
    for t in range(T):
        ls = 0.8 + rng.random(d)
        lv = 0.05 + 0.1 * rng.random(d)
        os_, noise, c = 0.5 + rng.random(), noise_of(t), 0.1 * t - 0.2
        kps.append(KernelParams("scale_linear_matern52", list(ls), outputscale=os_, noise=noise, const_mean=c,
                                linear_variance=list(lv)))
        ops.append(O.KernelParams(O.SCALE_LINEAR_MATERN52, ls, outputscale=os_, noise=noise, const_mean=c,
                                  linear_variance=lv))
        w = rng.standard_normal(d)
        Y[:, t] = c + np.sin(X @ w) + 0.3 * (X @ rng.standard_normal(d)) + np.sqrt(noise) * rng.standard_normal(n)
    return Problem(X, Y, Z, kps, ops)


def phi_matrix(Z, X, p, jitter=JITTER):
    Kzz = O.kernel_matrix(Z, Z, p)
    Kzz[np.diag_indices_from(Kzz)] += jitter
    L = O.cholesky(Kzz)
    return sla.solve_triangular(L, O.kernel_matrix(Z, X, p), lower=True, check_finite=False)


def fit_collapsed_task(Z, X, y, p, jitter=JITTER):
    """One task: dict with m, C (lower, positive diagonal, C C^T = S), S, B, b, Phi, r, and the bound ``F`` with its five
    ``terms`` in the C ABI's order."""
    n = X.shape[0]
    s2 = p.noise
    Phi = phi_matrix(Z, X, p, jitter)
    M = Phi.shape[0]
    r = np.asarray(y, dtype=np.float64) - p.const_mean
    B = np.eye(M) + Phi @ Phi.T / s2
    b = Phi @ r / s2
    LB = O.cholesky(B)
    S = sla.cho_solve((LB, True), np.eye(M), check_finite=False)
    S = 0.5 * (S + S.T)
    m = sla.cho_solve((LB, True), b, check_finite=False)
    C = O.cholesky(S)
    u = sla.solve_triangular(LB, b, lower=True, check_finite=False)
    terms = np.array([
        -0.5 * n * np.log(2.0 * np.pi * s2),
        -np.log(np.diag(LB)).sum(),
        -0.5 * (r @ r) / s2,
        0.5 * (u @ u),
        -0.5 * (O.kernel_diag(X, p).sum() - np.einsum("ij,ij->", Phi, Phi)) / s2,
    ])
    return {"m": m, "C": C, "S": S, "B": B, "b": b, "Phi": Phi, "r": r, "F": terms.sum(), "terms": terms}


def fit_collapsed(pb: Problem, jitter=JITTER):
    """(vmean T x M, vchol T x M x M, bound T x 6) of every task."""
    T = len(pb.ops)
    res = [fit_collapsed_task(pb.Z[t], pb.X, pb.Y[:, t], pb.ops[t], jitter) for t in range(T)]
    vmean = np.stack([r["m"] for r in res])
    vchol = np.stack([r["C"] for r in res])
    bound = np.stack([np.concatenate([[r["F"]], r["terms"]]) for r in res])
    return vmean, vchol, bound


def fps_cpu(X, k, start):
    """torch stand-in for GPEngine.fps (oracle farthest point sampling)."""
    import torch

    return torch.as_tensor(O.farthest_point_sampling(np.asarray(X), int(k), int(start)), dtype=torch.int64)
