"""Two independent CPU computations of the collapsed SVGP bound F and its hyperparameter gradient
(gpx_svgp_bound_grad_f64), on the problems of tests/sgpr_ref.py:

 (a) ``autograd_task``: F restated in torch fp64 with the three kernels written out, differentiated by autograd;
 (b) ``formula_task``: the closed-form derivatives in NumPy, in the arrangement the GPU kernel uses
     (H = W (I - S) W^T, G_u = (H K_u + c_v e^T) / s2, G_A = W (2I - S - B - m m^T) W^T / 2).

Both return a dict in the layout ``mll._loss_grad`` reads, gradients of -F with respect to the NATURAL parameters:
``nll`` = -F, ``noise``, ``outputscale``, ``const_mean``, ``lengthscale`` (d), ``linear_variance`` (d), ``bound`` (F and
its five terms), and ``parts``: for every gradient entry the signed contributions whose sum it is.  For the kernel's
parameters (outputscale, lengthscales, linear variances) these are the three parts through K_u = K(Z, X), through K_ZZ
and through the diagonal k(x_i, x_i); the noise and the constant mean do not enter a covariance, their parts are the
derivatives of the bound's five terms.  ``scale`` is the sum of the parts' absolute values: the entrywise yardstick
|dg_i| <= tau scale_i of the tests (the convention of test_gpu_svgp_collapsed.py's check_bound)."""
import functools
import math

import numpy as np
import scipy.linalg as sla
import torch

from bayesianoptimizer_amd import KernelParams
from oracle import gp_oracle as O
from tests import sgpr_ref as R

# (b) against (a), entrywise |dg_i| / scale_i, largest over sgpr_ref's four shapes, the three kinds and all tasks
# (tests/test_svgp_grad_host.py measures and prints it; shape 1, rbf); the suite's tolerance leaves a factor 32 for
# the GPU's different summation order
TAU0 = 6.5e-10
TAU = 32 * TAU0
# the extra shape of the DMAX = 16 kernels (n, M, d, T, input scale, noise), beside sgpr_ref.SHAPES
SHAPE16 = (300, 64, 12, 1, 0.3, lambda t: 1e-2)
# one shape per edge of the d-dispatched instances (DMAX = 4, 8, 16, 32): d = 4, 16, 32 fill theirs (no k < d guard is ever
# false), d = 9 and 17 are the narrowest of the next (d = 17: a single real coordinate in the second 16-dimension sweep).
# M = 130: the second row tile has two rows; n = 300 with chunk = 128: three chunks, the last of 44 columns.  Seeds 1000 d.
DSHAPES = {
    104: (300, 130, 4, 1, 0.3, lambda t: 1e-2),
    109: (300, 64, 9, 1, 0.3, lambda t: 1e-2),
    116: (300, 64, 16, 2, 0.3, lambda t: 1e-2),
    117: (300, 130, 17, 1, 0.3, lambda t: 1e-2),
    132: (300, 64, 32, 2, 0.3, lambda t: 1e-3 * (t + 1)),
}

KINDS = ("rbf", "matern52", "scale_linear_matern52")
ENTRIES = ("noise", "outputscale", "const_mean", "lengthscale", "linear_variance")
SQRT5 = math.sqrt(5.0)


def with_kind(p: KernelParams, kind: str) -> KernelParams:
    return p.replace(kind=kind)


def _kind(p) -> str:
    k = p.kind
    return k.lower() if isinstance(k, str) else KINDS[int(k)]


def flat(g: dict, key: str = None) -> np.ndarray:
    """The gradient entries (or ``g[key]``'s: 'scale') as one vector in ENTRIES order."""
    src = g if key is None else g[key]
    return np.concatenate([np.atleast_1d(np.asarray(src[k], dtype=np.float64)) for k in ENTRIES])


# ---- (a) torch autograd ------------------------------------------------------------------------------
def _kernel_t(A, B, kind, ls, os_, lv):
    r2 = torch.zeros((A.shape[0], B.shape[0]), dtype=torch.float64)
    for k in range(A.shape[1]):
        diff = A[:, k:k + 1] / ls[k] - (B[:, k] / ls[k])[None, :]
        r2 = r2 + diff * diff
    if kind == "rbf":
        return os_ * torch.exp(-0.5 * r2)
    pos = r2 > 0
    r = torch.where(pos, torch.sqrt(torch.where(pos, r2, torch.ones_like(r2))), torch.zeros_like(r2))
    mat = (1.0 + SQRT5 * r + (5.0 / 3.0) * r2) * torch.exp(-SQRT5 * r)
    if kind == "matern52":
        return os_ * mat
    return os_ * ((A * lv) @ B.T + mat)


def _diag_t(X, kind, os_, lv):
    if kind != "scale_linear_matern52":
        return os_ * torch.ones(X.shape[0], dtype=torch.float64)
    return os_ * ((X * X * lv).sum(1) + 1.0)


def autograd_task(Z, X, y, p: KernelParams, jitter: float = 1e-4) -> dict:
    kind = _kind(p)
    d = X.shape[1]
    Zt, Xt, yt = (torch.tensor(np.asarray(v, dtype=np.float64)) for v in (Z, X, y))
    n, M = Xt.shape[0], Zt.shape[0]

    def copy():  # one copy of the kernel's parameters per place they enter (K_u, K_ZZ, the diagonal)
        return (torch.tensor(p.lengthscales(d), dtype=torch.float64, requires_grad=True),
                torch.tensor(float(p.outputscale), dtype=torch.float64, requires_grad=True),
                torch.tensor(p.linear_variances(d), dtype=torch.float64, requires_grad=True))

    th = [copy() for _ in range(3)]
    s2 = torch.tensor(float(p.noise), dtype=torch.float64, requires_grad=True)
    c = torch.tensor(float(p.const_mean), dtype=torch.float64, requires_grad=True)
    Ku = _kernel_t(Zt, Xt, kind, *th[0])
    A = _kernel_t(Zt, Zt, kind, *th[1]) + jitter * torch.eye(M, dtype=torch.float64)
    kd = _diag_t(Xt, kind, th[2][1], th[2][2])
    L = torch.linalg.cholesky(A)
    Phi = torch.linalg.solve_triangular(L, Ku, upper=False)
    r = yt - c
    B = torch.eye(M, dtype=torch.float64) + Phi @ Phi.T / s2
    LB = torch.linalg.cholesky(B)
    u = torch.linalg.solve_triangular(LB, (Phi @ r / s2)[:, None], upper=False)[:, 0]
    terms = [-0.5 * n * torch.log(2.0 * math.pi * s2), -torch.log(torch.diagonal(LB)).sum(), -0.5 * (r @ r) / s2,
             0.5 * (u @ u), -0.5 * (kd.sum() - (Phi * Phi).sum()) / s2]
    F = terms[0] + terms[1] + terms[2] + terms[3] + terms[4]
    flat_th = [v for cp in th for v in cp]
    gk = torch.autograd.grad(F, flat_th, retain_graph=True, allow_unused=True)
    gk = [torch.zeros_like(v) if g is None else g for v, g in zip(flat_th, gk)]
    sc = []
    for tm in terms:
        g = torch.autograd.grad(tm, [s2, c], retain_graph=True, allow_unused=True)
        sc.append([0.0 if v is None else float(v) for v in g])
    sc = -np.array(sc)  # 5 x {noise, const_mean}, of -F
    lin = kind == "scale_linear_matern52"
    parts = {
        "noise": sc[:, 0], "const_mean": sc[:, 1],
        "outputscale": -np.array([float(gk[3 * q + 1]) for q in range(3)]),
        "lengthscale": -np.stack([gk[3 * q].numpy() for q in range(3)]),
        "linear_variance": -np.stack([gk[3 * q + 2].numpy() for q in range(3)]) if lin else np.zeros((3, d)),
    }
    return _pack(float(F.detach()), [float(t.detach()) for t in terms], parts)


def _pack(F, terms, parts):
    out = {"nll": -F, "bound": np.array([F] + list(terms)), "parts": parts,
           "scale": {k: np.abs(v).sum(axis=0) for k, v in parts.items()}}
    for k, v in parts.items():
        s = v.sum(axis=0)
        out[k] = float(s) if s.ndim == 0 else s
    return out


# ---- (b) the closed-form derivatives, NumPy ---------------------------------------------------------------
def _kernel_and_grads(A, B, kind, ls, os_, lv):
    """k(A, B) and its derivatives: d/d outputscale, d/d lengthscale_k (list), d/d linear_variance_k (list)."""
    d = A.shape[1]
    q = [((A[:, k:k + 1] - B[None, :, k]) / ls[k]) ** 2 for k in range(d)]
    r2 = np.zeros((A.shape[0], B.shape[0]))
    for k in range(d):
        r2 += q[k]
    if kind == "rbf":
        base = np.exp(-0.5 * r2)
        kfac = os_ * base
    else:
        r = np.sqrt(r2)
        ex = np.exp(-SQRT5 * r)
        base = (1.0 + SQRT5 * r + (5.0 / 3.0) * r2) * ex
        kfac = os_ * (5.0 / 3.0) * (1.0 + SQRT5 * r) * ex
    dv = []
    if kind == "scale_linear_matern52":
        xx = [A[:, k:k + 1] * B[None, :, k] for k in range(d)]
        for k in range(d):
            base = base + lv[k] * xx[k]
        dv = [os_ * xx[k] for k in range(d)]
    return os_ * base, base, [kfac * q[k] / ls[k] for k in range(d)], dv


def formula_task(Z, X, y, p: KernelParams, jitter: float = 1e-4) -> dict:
    kind = _kind(p)
    Z, X, y = (np.asarray(v, dtype=np.float64) for v in (Z, X, y))
    n, d = X.shape
    M = Z.shape[0]
    ls, lv = np.array(p.lengthscales(d)), np.array(p.linear_variances(d))
    os_, s2, c = float(p.outputscale), float(p.noise), float(p.const_mean)
    lin = kind == "scale_linear_matern52"
    Ku, dKu_os, dKu_ls, dKu_lv = _kernel_and_grads(Z, X, kind, ls, os_, lv)
    A, dA_os, dA_ls, dA_lv = _kernel_and_grads(Z, Z, kind, ls, os_, lv)
    A = A + jitter * np.eye(M)
    L = np.linalg.cholesky(A)
    W = sla.solve_triangular(L, np.eye(M), lower=True, check_finite=False).T  # L^{-T}
    Phi = W.T @ Ku
    r = y - c
    B = np.eye(M) + Phi @ Phi.T / s2
    b = Phi @ r / s2
    LB = np.linalg.cholesky(B)
    Wp = sla.solve_triangular(LB, np.eye(M), lower=True, check_finite=False).T
    S = Wp @ Wp.T
    u = Wp.T @ b
    m = Wp @ u
    cv = W @ m
    e = r - Ku.T @ cv
    H = W @ (np.eye(M) - S) @ W.T
    Gu = (H @ Ku + np.outer(cv, e)) / s2
    GA = 0.5 * W @ (2.0 * np.eye(M) - S - B - np.outer(m, m)) @ W.T
    xx = (X * X * lv).sum(1) if lin else np.zeros(n)
    kdiag = os_ * (xx + 1.0)
    trPP = float(np.einsum("ij,ij->", Phi, Phi))
    terms = [-0.5 * n * math.log(2.0 * math.pi * s2), -np.log(np.diag(LB)).sum(), -0.5 * (r @ r) / s2, 0.5 * (u @ u),
             -0.5 * (kdiag.sum() - trPP) / s2]
    F = terms[0] + terms[1] + terms[2] + terms[3] + terms[4]
    # dF/ds2 = -n/(2 s2) + (M - tr S)/(2 s2) + e^T e/(2 s2^2) + (sum k(x_i, x_i) - tr Phi Phi^T)/(2 s2^2); by the bound's
    # terms: d(logdet) = (M - tr S)/(2 s2), d(quad) = r^T r/(2 s2^2), d(fit) = (e^T e - r^T r)/(2 s2^2)
    rr, ee = float(r @ r), float(e @ e)
    d_s2 = [-0.5 * n / s2, 0.5 * (M - np.trace(S)) / s2, 0.5 * rr / s2 ** 2, 0.5 * (ee - rr) / s2 ** 2,
            0.5 * (kdiag.sum() - trPP) / s2 ** 2]
    # dF/dc = sum_i e_i / s2: quad gives sum r / s2, fit gives -(sum r - sum e) / s2
    d_c = [0.0, 0.0, r.sum() / s2, (e.sum() - r.sum()) / s2, 0.0]
    con = lambda G, D: float(np.einsum("ij,ij->", G, D))
    parts = {
        "noise": -np.array(d_s2), "const_mean": -np.array(d_c),
        "outputscale": -np.array([con(Gu, dKu_os), con(GA, dA_os), -0.5 / s2 * (xx + 1.0).sum()]),
        "lengthscale": -np.stack([np.array([con(Gu, D) for D in dKu_ls]), np.array([con(GA, D) for D in dA_ls]),
                                  np.zeros(d)]),
        "linear_variance": -np.stack([np.array([con(Gu, D) for D in dKu_lv]), np.array([con(GA, D) for D in dA_lv]),
                                      -0.5 / s2 * os_ * (X * X).sum(0)]) if lin else np.zeros((3, d)),
    }
    return _pack(F, terms, parts)


def value_grad_all(pb_Z, X, Y, jitter: float = 1e-4, task=autograd_task):
    """``value_grad_all(params) -> list of dicts`` for mll.fit_hyperparameters_sparse: computation (a) per task."""
    Xn, Yn = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)

    def f(params):
        return [task(pb_Z[t], Xn, Yn[:, t], p, jitter) for t, p in enumerate(params)]

    return f


def entry_ratio(got: dict, ref: dict) -> float:
    """max_i |got_i - ref_i| / scale_i over the gradient entries (scale from ``ref``; entries whose scale is 0 must
    agree exactly and count as 0)."""
    dg, sc = np.abs(flat(got) - flat(ref)), flat(ref, "scale")
    assert np.all(dg[sc == 0.0] == 0.0), "an entry without contributions must be exactly 0"
    return float(np.max(dg[sc > 0.0] / sc[sc > 0.0])) if np.any(sc > 0.0) else 0.0


# ---- problems and cached references ------------------------------------------------------------------------
def make_problem(n, M, d, T, s, noise_of, seed) -> R.Problem:
    """sgpr_ref.problem's recipe at free sizes (engine parameters only; kind scale_linear_matern52)."""
    rng = np.random.default_rng(seed)
    X = s * rng.standard_normal((n, d))
    Z = np.repeat(X[rng.choice(n, size=M, replace=False)][None], T, axis=0)
    Y = np.empty((n, T))
    kps, ops = [], []
    for t in range(T):
        ls, lv = 0.8 + rng.random(d), 0.05 + 0.1 * rng.random(d)
        os_, noise, c = 0.5 + rng.random(), noise_of(t), 0.1 * t - 0.2
        kps.append(KernelParams("scale_linear_matern52", list(ls), outputscale=os_, noise=noise, const_mean=c,
                                linear_variance=list(lv)))
        ops.append(O.KernelParams(O.SCALE_LINEAR_MATERN52, ls, outputscale=os_, noise=noise, const_mean=c,
                                  linear_variance=lv))
        w = rng.standard_normal(d)
        Y[:, t] = c + np.sin(X @ w) + 0.3 * (X @ rng.standard_normal(d)) + np.sqrt(noise) * rng.standard_normal(n)
    return R.Problem(X, Y, Z, kps, ops)


@functools.lru_cache(maxsize=None)
def problem(shape) -> R.Problem:
    """sgpr_ref.problem(shape) for its shapes 1-4; shape 16: SHAPE16; the DSHAPES by their keys."""
    if shape in DSHAPES:
        pb = make_problem(*DSHAPES[shape], seed=1000 * DSHAPES[shape][2])
    else:
        pb = make_problem(*SHAPE16, seed=16000) if shape == 16 else R.problem(shape)
    for a in (pb.X, pb.Y, pb.Z):
        a.setflags(write=False)
    return pb


@functools.lru_cache(maxsize=None)
def reference(shape, kind, jitter=R.JITTER, tasks=None):
    """Computation (a) for every task (or the listed ones) of a problem with its kernels set to ``kind``: computed
    once and shared.  Returns (problem, parameters per task, list of (a)'s dicts)."""
    pb = problem(shape)
    kps = [with_kind(p, kind) for p in pb.kps]
    ts = range(len(kps)) if tasks is None else tasks
    return pb, kps, [autograd_task(pb.Z[t], pb.X, pb.Y[:, t], kps[t], jitter) for t in ts]


def check_grad(got: dict, ref: dict, tau: float = TAU, what: str = ""):
    """The suite's gradient check: every entry within tau of its scale, the ratio printed before it is asserted."""
    ratio = entry_ratio(got, ref)
    print(f"{what}: max |dg| / scale = {ratio:.3e} (tau = {tau:.2e})")
    assert ratio <= tau, what
