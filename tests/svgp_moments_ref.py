"""CPU references of gpx_svgp_moments_grad_f64 (include/gpx.h): the latent q-batch posterior moments of one SVGP task and
their first-argument derivatives w.r.t. the candidates.

* ``moments_grad``: NumPy fp64 by triangular solves, V = L^-1 K*, G = V - S (S^T V), H = L^-T G, alpha' = L^-T m, with
  the oracle's kernels and first-argument kernel derivatives (as ``oracle.gp_oracle.moments_grad`` uses them).  No
  inverse and no W (I - S S^T) W^T is formed, and nothing assumes S S^T <= I.
* ``torch_moments``: the same predictive written out independently in torch (kernels restated here, covariance in the
  form K** - A^T A + (S^T A)^T (S^T A)), differentiable w.r.t. the candidates.
* ``problem``: the inputs of the GPU tests, one (M, d, q, B) shape and kernel kind at a time.
* ``SvgpOracleEngine``: the oracle engine with the sparse model's calls on the CPU, for runs of the drop-in without a GPU.
"""
from functools import lru_cache

import numpy as np
import scipy.linalg as sla
import torch

from bayesianoptimizer_amd.engine import SVGPTaskState
from oracle import gp_oracle as O
from tests import sgpr_ref as R
from tests.ard_util import ard_params
from tests.mc_nei_ref import NeiOracleEngine
from tests.oracle_engine import to_oracle_params

JITTER = 1e-4


def _factor(Z, p, jitter):
    Kzz = O.kernel_matrix(Z, Z, p)
    Kzz[np.diag_indices_from(Kzz)] += jitter
    return O.cholesky(Kzz)


def moments_grad(Z, vmean, vchol, p, Xs, q, jitter=JITTER):
    """mean (m), dmean (m, d), cov (m, q), dcov (m, d, q) of one task: Z (M, d), vmean (M), vchol (M, M; lower triangle
    used), p the oracle's KernelParams, Xs (m, d) in consecutive q-batches."""
    Z, Xs = np.asarray(Z, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    m, d = Xs.shape
    L = _factor(Z, p, jitter)
    Ks = O.kernel_matrix(Z, Xs, p)  # (M, m)
    V = sla.solve_triangular(L, Ks, lower=True, check_finite=False)
    S = np.tril(np.asarray(vchol, dtype=np.float64))
    G = V - S @ (S.T @ V)
    H = sla.solve_triangular(L, G, lower=True, trans="T", check_finite=False)
    alpha = sla.solve_triangular(L, np.asarray(vmean, dtype=np.float64), lower=True, trans="T", check_finite=False)
    D = O.kernel_grad_first(Xs, Z, p)  # (m, M, d)
    mean = p.const_mean + Ks.T @ alpha
    dmean = np.einsum("aij,i->aj", D, alpha)
    cov = np.empty((m, q))
    dcov = np.empty((m, d, q))
    for a in range(m):
        b0 = (a // q) * q
        cols = slice(b0, b0 + q)
        kp = O.kernel_matrix(Xs[a:a + 1], Xs[cols], p)[0]
        gp = O.kernel_grad_first(Xs[a:a + 1], Xs[cols], p)[0]  # (q, d)
        cov[a] = kp - Ks[:, a] @ H[:, cols]
        dcov[a] = gp.T - D[a].T @ H[:, cols]
    return mean, dmean, cov, dcov


# ---- torch restatement ---------------------------------------------------------------------------------------------
def torch_kernel(A, B, p):
    """k(a, b) for all rows of A (.., na, d) and B (.., nb, d): the three kinds of the C ABI, written from their
    definitions."""
    ls = torch.tensor(np.asarray(p.lengthscale, dtype=np.float64))
    diff = (A.unsqueeze(-2) - B.unsqueeze(-3)) / ls
    r2 = (diff * diff).sum(-1)
    if p.kind == O.RBF:
        return p.outputscale * torch.exp(-0.5 * r2)
    # sqrt has no derivative at 0 (a candidate against itself): r2 + 0 there, where the Matern's own derivative is 0
    r = torch.sqrt(torch.where(r2 > 0, r2, torch.ones_like(r2))) * (r2 > 0)
    s5r = np.sqrt(5.0) * r
    mat = (1.0 + s5r + (5.0 / 3.0) * r2) * torch.exp(-s5r)
    if p.kind == O.MATERN52:
        return p.outputscale * mat
    lv = torch.tensor(np.asarray(p.linear_variance, dtype=np.float64))
    return p.outputscale * ((A * lv) @ B.transpose(-1, -2) + mat)


def torch_moments(Z, vmean, vchol, p, X, jitter=JITTER):
    """mean (B, q) and covariance (B, q, q) of the q-batches X (B, q, d), differentiable w.r.t. X."""
    Z = torch.tensor(np.array(Z, dtype=np.float64))
    mvec = torch.tensor(np.array(vmean, dtype=np.float64))
    S = torch.tril(torch.tensor(np.array(vchol, dtype=np.float64)))
    Kzz = torch_kernel(Z, Z, p) + jitter * torch.eye(Z.shape[0], dtype=torch.float64)
    L = torch.linalg.cholesky(Kzz)
    Ks = torch_kernel(Z.expand(X.shape[0], -1, -1), X, p)  # (B, M, q)
    A = torch.linalg.solve_triangular(L, Ks, upper=False)
    SA = S.T @ A
    mean = p.const_mean + (A * mvec.view(1, -1, 1)).sum(1)
    cov = torch_kernel(X, X, p) - A.transpose(1, 2) @ A + SA.transpose(1, 2) @ SA
    return mean, cov


def prior_scale(p, Xs):
    """The prior variance scale the covariance tolerance is relative to: outputscale, times 1 + sum_k v_k x_k^2 at the
    candidate where that is largest for the linear kind."""
    if p.kind != O.SCALE_LINEAR_MATERN52:
        return p.outputscale
    return p.outputscale * (1.0 + float((np.asarray(Xs) ** 2 @ np.asarray(p.linear_variance)).max()))


# ---- the GPU tests' inputs -------------------------------------------------------------------------------------------
N_FIT = 600
SHAPES = ((50, 4, 4, 2), (129, 1, 1, 5), (200, 5, 3, 3), (300, 9, 32, 5), (130, 32, 2, 2), (140, 17, 2, 2))
KINDS = ("rbf", "matern52", "scale_linear_matern52")


@lru_cache(maxsize=None)
def problem(M, d, q, B, kind):
    """(kp, op, Z (M, d), X (N_FIT, d), y (N_FIT), Xs (B q, d), vmean (M), vchol (M, M)) with ARD lengthscales (and ARD
    linear variances for the linear kind), read-only.  Inputs lie in the unit cube; Z is a stratified draw (one point per
    cell of a regular partition of the first coordinate, jittered), so that no two inducing points coincide at d = 1.
    vmean / vchol are the ARBITRARY state: random mean, random lower-triangular factor with diagonal 1.5, for which
    S S^T <= I fails (its first diagonal entry is 2.25)."""
    rng = np.random.default_rng(100000 + 1000 * M + 10 * d + q)
    kp, op = ard_params(kind, d, d, noise=1e-2, outputscale=1.3, const_mean=0.2)
    Z = rng.random((M, d))
    Z[:, 0] = (rng.permutation(M) + 0.1 + 0.8 * rng.random(M)) / M
    X = rng.random((N_FIT, d))
    w = rng.standard_normal(d) / np.sqrt(d)
    y = np.sin(3.0 * X @ w) + 0.3 * (X ** 2).sum(1) / d + 0.1 * rng.standard_normal(N_FIT)
    Xs = rng.random((B * q, d))
    vmean = rng.standard_normal(M)
    vchol = np.tril(rng.standard_normal((M, M)) / np.sqrt(M), -1) + 1.5 * np.eye(M)
    out = (kp, op, Z, X, y, Xs, vmean, vchol)
    for a in out[2:]:
        a.setflags(write=False)
    return out


# ---- the drop-in on the CPU ----------------------------------------------------------------------------------------
class SvgpOracleEngine(NeiOracleEngine):
    """The oracle engine (with the MC acquisition reference) plus the sparse model's calls restated on the CPU: the
    closed-form fit (sgpr_ref), the predictive (oracle), ``svgp_moments_grad`` (above) and the ``moments_grad``
    dispatch on an SVGPTaskState."""

    device = torch.device("cpu")

    def svgp_fit_collapsed(self, params, Z, X, Y, jitter=JITTER, chunk=None):
        Z, X, Y = (np.asarray(torch.as_tensor(v).cpu(), dtype=np.float64) for v in (Z, X, Y))
        res = [R.fit_collapsed_task(Z[t], X, Y[:, t], to_oracle_params(p, X.shape[1]), jitter)
               for t, p in enumerate(params)]
        bound = np.stack([np.concatenate([[r["F"]], r["terms"]]) for r in res])
        return (torch.tensor(np.stack([r["m"] for r in res])), torch.tensor(np.stack([r["C"] for r in res])),
                torch.tensor(bound))

    def svgp_prepare(self, params, Z, vmean, vchol, jitter=JITTER):
        Z, vmean, vchol = (torch.as_tensor(v, dtype=torch.float64) for v in (Z, vmean, vchol))
        d = Z.shape[2]
        alpha = np.stack([sla.solve_triangular(_factor(Z[t].numpy(), to_oracle_params(p, d), jitter), vmean[t].numpy(),
                                               lower=True, trans="T") for t, p in enumerate(params)])
        return {"Z": Z, "vmean": vmean, "vchol": vchol, "params": list(params), "jitter": jitter,
                "alpha": torch.tensor(alpha)}

    def svgp_predict(self, prep, Xs, min_var=1e-10, want=("mean", "var", "score")):
        d = Xs.shape[1]
        mu, var, score = O.svgp_predict(prep["Z"].numpy(), prep["vmean"].numpy(), prep["vchol"].numpy(),
                                        [to_oracle_params(p, d) for p in prep["params"]], np.asarray(Xs),
                                        jitter=prep["jitter"], min_var=min_var)
        return torch.tensor(mu), torch.tensor(var), torch.tensor(score)

    def svgp_moments_grad(self, prep, task, Xs, q=1, need_grad=True):
        self.calls.setdefault("svgp_moments_grad", []).append((int(Xs.shape[0]), int(q), bool(need_grad)))
        Xs = torch.as_tensor(Xs, dtype=torch.float64).cpu().numpy()
        p = to_oracle_params(prep["params"][task], Xs.shape[1])
        mean, dmean, cov, dcov = (torch.tensor(v) for v in moments_grad(
            prep["Z"][task].numpy(), prep["vmean"][task].numpy(), prep["vchol"][task].numpy(), p, Xs, q, prep["jitter"]))
        return (mean, dmean, cov, dcov) if need_grad else (mean, None, cov, None)

    def moments_grad(self, state, Xs, q=1, alpha=None):
        if isinstance(state, SVGPTaskState):
            if alpha is not None and alpha.data_ptr() != state.alpha.data_ptr():
                raise ValueError("an SVGP task's objective column is its own alpha'")
            return self.svgp_moments_grad(state.prep, state.task, Xs, q)
        return super().moments_grad(state, Xs, q, alpha)


def dropin_optimizer(tmp_path, acquisition, batch_size=8, engine=None):
    """The drop-in on the sparse policy above 30 points, with 40 initial points of the stub simulator."""
    from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
    from tests.stubs import BOUNDS, StubSimulator

    cfg = GPConfig(large_n_policy=True, large_n_model="sparse", num_restarts=2, acqf_raw_samples=32)
    return BayesianOptimizer(StubSimulator(), BOUNDS, str(tmp_path / acquisition), n_initial_points=40, n_batches=1,
                             batch_size=batch_size, svgp_threshold=30, target_total=40 + batch_size,
                             engine=engine if engine is not None else SvgpOracleEngine(), gp_config=cfg,
                             acquisition=acquisition, seed=4)


def dropin_round(opt, k=8):
    """Initial design, the sparse fit and one acquisition of k points: finite, in the unit cube."""
    from bayesianoptimizer_amd.models import SparseGP

    opt._initial_design()
    opt.fit_gp_model()
    assert isinstance(opt.gp_model, SparseGP)
    batch = opt.acquire(k)
    assert batch.shape == (k, 5) and bool(torch.isfinite(batch).all())
    assert float(batch.min()) >= 0.0 and float(batch.max()) <= 1.0
    return batch
