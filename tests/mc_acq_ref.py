"""Independent fp64 reference of gpx_mc_acq_f64 in torch on the CPU (include/gpx.h): the forward definitions written
from scratch, gradients by autograd through the symmetrised covariance and the Cholesky factor.  Imports nothing from
bayesianoptimizer_amd.acqf."""
import math

import torch

JITTERS = (0.0, 1e-8, 1e-7, 1e-6)
FAT_ALPHA = 2.0


def softplus(y):
    return torch.logaddexp(y, torch.zeros_like(y))  # exact: no linear branch above a threshold


def log_improvement(f, best_f, tau_relu, fat_relu):
    y = (f - best_f) / tau_relu
    if fat_relu:
        return math.log(tau_relu) + torch.log(softplus(y) + 0.1 / (1.0 + y * y))
    return math.log(tau_relu) + torch.where(y > -37.0, torch.log(softplus(torch.clamp(y, min=-37.0))), y)


def fatmax(li, tau, dim=-1):
    M = li.amax(dim=dim, keepdim=True)
    t = 1.0 + (M - li) / (FAT_ALPHA * tau)
    return M.squeeze(dim) + tau * torch.log((t ** -FAT_ALPHA).sum(dim=dim))


def smoothmax(li, tau, dim=-1):
    return tau * torch.logsumexp(li / tau, dim=dim)


def batch_jitter(cov):
    """Per q-batch: (info, jitter) of the first of A, A + 1e-8 I, A + 1e-7 I, A + 1e-6 I that factors (info -1: none)."""
    A = 0.5 * (cov + cov.transpose(1, 2))
    eye = torch.eye(A.shape[-1], dtype=A.dtype)
    info = torch.full((A.shape[0],), -1, dtype=torch.int32)
    jit = torch.zeros(A.shape[0], dtype=A.dtype)
    for b in range(A.shape[0]):
        for k, j in enumerate(JITTERS):
            L, bad = torch.linalg.cholesky_ex(A[b] + j * eye)
            if int(bad) == 0 and bool(torch.isfinite(L).all()):
                info[b], jit[b] = k, j
                break
    return info, jit


def mc_acq(mean, cov, z, kind, best_f=0.0, fat_relu=True, fat_max=False, tau_relu=1e-6, tau_max=1e-2):
    """(value (B), gmean (B, q), gcov (B, q, q), info (B)) for mean (B, q), cov (B, q, q), z (S, q)."""
    mean = mean.detach().cpu().double().clone().requires_grad_(True)
    cov = cov.detach().cpu().double().clone().requires_grad_(True)
    z = z.detach().cpu().double()
    B, q = mean.shape
    S = z.shape[0]
    info, jit = batch_jitter(cov.detach())
    ok = info >= 0
    eye = torch.eye(q, dtype=torch.float64)
    A = 0.5 * (cov + cov.transpose(1, 2)) + jit.view(B, 1, 1) * eye
    A = torch.where(ok.view(B, 1, 1), A, eye)  # placeholder for the batches that do not factor
    L = torch.linalg.cholesky(A)
    f = mean.unsqueeze(0) + torch.einsum("bij,sj->sbi", L, z)  # S x B x q
    if kind == "qlogei":
        li = log_improvement(f, best_f, tau_relu, fat_relu)
        r = fatmax(li, tau_max) if fat_max else smoothmax(li, tau_max)
        value = torch.logsumexp(r, dim=0) - math.log(S)
    elif kind == "qpsd":
        value = f.std(dim=0).sum(dim=-1)
    else:
        raise ValueError(kind)
    gmean, gcov = torch.autograd.grad(value[ok].sum(), (mean, cov), allow_unused=True)
    gmean = torch.zeros_like(mean) if gmean is None else gmean
    nan = torch.tensor(float("nan"), dtype=torch.float64)
    value = torch.where(ok, value.detach(), nan)
    gmean = torch.where(ok.view(B, 1), gmean, nan)
    gcov = torch.where(ok.view(B, 1, 1), gcov, nan)
    return value, gmean, gcov, info


def qpsd_closed_form(L, z):
    """sum_i sqrt(l_i C l_i^T) with C the unbiased sample covariance of the rows of z: the form the kernel evaluates."""
    C = torch.cov(z.T).reshape(z.shape[1], z.shape[1])
    return torch.sqrt(torch.einsum("bij,jk,bik->bi", L, C, L)).sum(dim=-1)


def synthetic_moments(B, q, seed):
    """cov = R R^T / (q + 3) * 0.3 with R of shape q x (q + 3), mean ~ 0.5 N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    R = torch.randn(B, q, q + 3, dtype=torch.float64, generator=g)
    cov = R @ R.transpose(1, 2) / (q + 3) * 0.3
    mean = 0.5 * torch.randn(B, q, dtype=torch.float64, generator=g)
    return mean, cov


def base_samples(S, q, seed):
    return torch.randn(S, q, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
