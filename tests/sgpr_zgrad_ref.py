"""Two independent CPU computations of the gradient of the collapsed SVGP bound with respect to the inducing locations
(gpx_svgp_bound_grad_z_f64), on the problems of tests/sgpr_grad_ref.py:

 (a) ``autograd_dz``: sgpr_grad_ref.autograd_task's F in torch fp64 with Z differentiated;
 (b) ``formula_dz``: the closed form in NumPy.  With G_u = dF/dK(Z, X) and G_A = dF/dK_ZZ (sgpr_grad_ref.formula_task)
     and d1 the derivative in the first argument,
        dF/dz_ak = sum_i G_u[a, i] d1 k(z_a, x_i)_k + 2 sum_b G_A[a, b] d1 k(z_a, z_b)_k
        d1 k(z, x)_k = -kfac (z_k - x_k) / l_k^2  (+ outputscale v_k x_k for the linear part).

Both return d(-F)/dZ (M x d), the sign the library writes.  (b) also returns ``scale``, the sum of the ABSOLUTE summands
of the two sums above: the entrywise yardstick |d dZ_ak| <= tau scale_ak.  (The "sum of |parts|" of sgpr_grad_ref would
have only two parts per entry here, which cancel: it is not used.)"""
import functools
import math

import numpy as np
import scipy.linalg as sla
import torch

from tests import sgpr_grad_ref as G
from tests import sgpr_ref as R

# (b) against (a), entrywise |d| / scale, largest over sgpr_grad_ref.problem's shapes (1-4, 16 and its DSHAPES), the
# three kinds and all tasks: tests/test_svgp_zgrad_host.py measures and prints it (4.76e-12, attained at shape 2, rbf,
# task 0).  The GPU tests leave the project's factor 32 for the different summation order (sgpr_grad_ref.TAU).
TAUZ0 = 4.8e-12
TAUZ = 32 * TAUZ0
SHAPES = (1, 2, 3, 4, 16) + tuple(G.DSHAPES)


def _bound_t(Zt, Xt, yt, p, kind, jitter):
    d = Xt.shape[1]
    n, M = Xt.shape[0], Zt.shape[0]
    ls = torch.tensor(p.lengthscales(d), dtype=torch.float64)
    os_ = torch.tensor(float(p.outputscale), dtype=torch.float64)
    lv = torch.tensor(p.linear_variances(d), dtype=torch.float64)
    s2, c = float(p.noise), float(p.const_mean)
    Ku = G._kernel_t(Zt, Xt, kind, ls, os_, lv)
    A = G._kernel_t(Zt, Zt, kind, ls, os_, lv) + jitter * torch.eye(M, dtype=torch.float64)
    kd = G._diag_t(Xt, kind, os_, lv)
    L = torch.linalg.cholesky(A)
    Phi = torch.linalg.solve_triangular(L, Ku, upper=False)
    r = yt - c
    B = torch.eye(M, dtype=torch.float64) + Phi @ Phi.T / s2
    LB = torch.linalg.cholesky(B)
    u = torch.linalg.solve_triangular(LB, (Phi @ r / s2)[:, None], upper=False)[:, 0]
    return (-0.5 * n * math.log(2.0 * math.pi * s2) - torch.log(torch.diagonal(LB)).sum() - 0.5 * (r @ r) / s2
            + 0.5 * (u @ u) - 0.5 * (kd.sum() - (Phi * Phi).sum()) / s2)


def autograd_dz(Z, X, y, p, jitter: float = R.JITTER) -> np.ndarray:
    """(a): d(-F)/dZ by autograd."""
    Zt = torch.tensor(np.asarray(Z, dtype=np.float64), requires_grad=True)
    Xt, yt = (torch.tensor(np.asarray(v, dtype=np.float64)) for v in (X, y))
    F = _bound_t(Zt, Xt, yt, p, G._kind(p), jitter)
    return -torch.autograd.grad(F, Zt)[0].numpy()


def bound_value(Z, X, y, p, jitter: float = R.JITTER) -> float:
    """F itself in NumPy (the finite-difference check's function)."""
    kind = G._kind(p)
    Z, X, y = (np.asarray(v, dtype=np.float64) for v in (Z, X, y))
    n, d = X.shape
    M = Z.shape[0]
    ls, lv = np.array(p.lengthscales(d)), np.array(p.linear_variances(d))
    os_, s2, c = float(p.outputscale), float(p.noise), float(p.const_mean)
    Ku = G._kernel_and_grads(Z, X, kind, ls, os_, lv)[0]
    A = G._kernel_and_grads(Z, Z, kind, ls, os_, lv)[0] + jitter * np.eye(M)
    L = np.linalg.cholesky(A)
    Phi = sla.solve_triangular(L, Ku, lower=True, check_finite=False)
    r = y - c
    LB = np.linalg.cholesky(np.eye(M) + Phi @ Phi.T / s2)
    u = sla.solve_triangular(LB, Phi @ r / s2, lower=True, check_finite=False)
    kdiag = os_ * (((X * X * lv).sum(1) if kind == "scale_linear_matern52" else 0.0) + np.ones(n))
    return float(-0.5 * n * math.log(2.0 * math.pi * s2) - np.log(np.diag(LB)).sum() - 0.5 * (r @ r) / s2
                 + 0.5 * (u @ u) - 0.5 * (kdiag.sum() - np.einsum("ij,ij->", Phi, Phi)) / s2)


def _d1k(A, B, kind, ls, os_, lv):
    """d1 k(a, b)_k for every pair: |A| x |B| x d."""
    diff = A[:, None, :] - B[None, :, :]
    r2 = ((diff / ls) ** 2).sum(-1)
    if kind == "rbf":
        kfac = os_ * np.exp(-0.5 * r2)
    else:
        r = np.sqrt(r2)
        kfac = os_ * (5.0 / 3.0) * (1.0 + G.SQRT5 * r) * np.exp(-G.SQRT5 * r)
    out = -kfac[:, :, None] * diff / ls ** 2
    if kind == "scale_linear_matern52":
        out = out + os_ * lv * B[None, :, :]
    return out


def formula_dz(Z, X, y, p, jitter: float = R.JITTER):
    """(b): (d(-F)/dZ, scale), both M x d."""
    kind = G._kind(p)
    Z, X, y = (np.asarray(v, dtype=np.float64) for v in (Z, X, y))
    d = X.shape[1]
    M = Z.shape[0]
    ls, lv = np.array(p.lengthscales(d)), np.array(p.linear_variances(d))
    os_, s2, c = float(p.outputscale), float(p.noise), float(p.const_mean)
    Ku = G._kernel_and_grads(Z, X, kind, ls, os_, lv)[0]
    A = G._kernel_and_grads(Z, Z, kind, ls, os_, lv)[0] + jitter * np.eye(M)
    L = np.linalg.cholesky(A)
    W = sla.solve_triangular(L, np.eye(M), lower=True, check_finite=False).T
    Phi = W.T @ Ku
    r = y - c
    B = np.eye(M) + Phi @ Phi.T / s2
    LB = np.linalg.cholesky(B)
    Wp = sla.solve_triangular(LB, np.eye(M), lower=True, check_finite=False).T
    S = Wp @ Wp.T
    m = Wp @ (Wp.T @ (Phi @ r / s2))
    cv = W @ m
    e = r - Ku.T @ cv
    Gu = (W @ (np.eye(M) - S) @ W.T @ Ku + np.outer(cv, e)) / s2
    GA = 0.5 * W @ (2.0 * np.eye(M) - S - B - np.outer(m, m)) @ W.T
    tu = Gu[:, :, None] * _d1k(Z, X, kind, ls, os_, lv)
    ta = 2.0 * GA[:, :, None] * _d1k(Z, Z, kind, ls, os_, lv)
    return -(tu.sum(1) + ta.sum(1)), np.abs(tu).sum(1) + np.abs(ta).sum(1)


def ratio(got, ref, scale) -> float:
    """max |got - ref| / scale over the entries."""
    return float(np.max(np.abs(np.asarray(got) - ref) / scale))


@functools.lru_cache(maxsize=None)
def reference(shape, kind, jitter=R.JITTER):
    """Per task of sgpr_grad_ref.problem(shape) with its kernels set to ``kind``: (a) and (b)'s scale, computed once and
    shared.  Returns (problem, parameters per task, list of (autograd dZ, scale))."""
    pb = G.problem(shape)
    kps = [G.with_kind(p, kind) for p in pb.kps]
    return pb, kps, [(autograd_dz(pb.Z[t], pb.X, pb.Y[:, t], kps[t], jitter),
                      formula_dz(pb.Z[t], pb.X, pb.Y[:, t], kps[t], jitter)[1]) for t in range(len(kps))]


def value_grad_all(X, Y, jitter: float = R.JITTER):
    """``value_grad_all(params, Z)`` for mll.fit_hyperparameters_sparse(learn_inducing=True): sgpr_grad_ref's (a) with
    (a)'s dZ as ``"inducing"``."""
    Xn, Yn = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)

    def f(params, Z):
        out = []
        for t, p in enumerate(params):
            g = G.autograd_task(Z[t], Xn, Yn[:, t], p, jitter)
            g["inducing"] = autograd_dz(Z[t], Xn, Yn[:, t], p, jitter)
            out.append(g)
        return out

    return f
