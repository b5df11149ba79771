"""CPU reference of gpx_svgp_condition_f64 (include/gpx.h): the exact Bayesian update of one task's whitened
q(u) = N(m, C C^T) by new Gaussian observations, in the basis of the current posterior.

* ``condition_task``: NumPy / SciPy fp64 by triangular solves.  U = C^T L^-1 K(Z, X_n), e = y_n - const - Phi_n^T m,
  P = I + U U^T / s2; D is the lower-triangular factor with D D^T = P^-1, obtained as the C ABI does: the Cholesky
  factor of P in REVERSED index order, its inverse transposed, reversed back.  No inverse of P or of S is formed.
* ``dense_update``: the same update written out independently from S' = (S^-1 + Phi Phi^T / s2)^-1 and
  m' = S' (S^-1 m + Phi r / s2) with dense inverses (for the check of ``condition_task`` only).
* ``SvgpConditionOracleEngine``: tests/svgp_acquire_ref.SvgpAcquireOracleEngine plus ``svgp_condition`` answered from
  ``condition_task``, for the drop-in without a GPU.
"""
import numpy as np
import scipy.linalg as sla
import torch

from oracle import gp_oracle as O
from tests import sgpr_ref as R
from tests import svgp_acquire_ref as AR
from tests import svgp_moments_ref as SR
from tests.oracle_engine import to_oracle_params


def lower_inverse_factor(P):
    """D lower triangular with positive diagonal and D D^T = P^-1 (unique): with J the index reversal, J P J = L' L'^T,
    W' = L'^-T (upper) and D = J W' J."""
    n = P.shape[0]
    Lr = O.cholesky(P[::-1, ::-1])
    Wr = sla.solve_triangular(Lr, np.eye(n), lower=True, check_finite=False).T
    return np.ascontiguousarray(Wr[::-1, ::-1])


def condition_task(Z, m, C, p, Xn, yn, jitter=R.JITTER):
    """One task: dict with the updated ``m`` and ``C`` (lower, positive diagonal), and ``U``, ``e``, ``D``, ``g``.
    Z (M, d), m (M), C (M, M; lower triangle used), p the oracle's KernelParams, Xn (k, d), yn (k)."""
    m = np.asarray(m, dtype=np.float64)
    C = np.tril(np.asarray(C, dtype=np.float64))
    s2 = p.noise
    Phi = R.phi_matrix(np.asarray(Z, dtype=np.float64), np.asarray(Xn, dtype=np.float64), p, jitter)  # (M, k)
    U = C.T @ Phi
    e = np.asarray(yn, dtype=np.float64) - p.const_mean - Phi.T @ m
    P = np.eye(C.shape[0]) + U @ U.T / s2
    D = lower_inverse_factor(P)
    g = D @ (D.T @ (U @ e)) / s2
    return {"m": m + C @ g, "C": np.tril(C @ D), "U": U, "e": e, "D": D, "g": g}


def dense_update(Z, m, C, p, Xn, yn, jitter=R.JITTER):
    """(m', S') from the information form with dense inverses."""
    m = np.asarray(m, dtype=np.float64)
    C = np.tril(np.asarray(C, dtype=np.float64))
    s2 = p.noise
    Phi = R.phi_matrix(np.asarray(Z, dtype=np.float64), np.asarray(Xn, dtype=np.float64), p, jitter)
    Sinv = np.linalg.inv(C @ C.T)
    Snew = np.linalg.inv(Sinv + Phi @ Phi.T / s2)
    Snew = 0.5 * (Snew + Snew.T)
    r = np.asarray(yn, dtype=np.float64) - p.const_mean
    return Snew @ (Sinv @ m + Phi @ r / s2), Snew


def condition(Z, vmean, vchol, ops, Xn, Yn, jitter=R.JITTER):
    """Every task: (vmean T x M, vchol T x M x M)."""
    res = [condition_task(Z[t], vmean[t], vchol[t], ops[t], Xn, Yn[:, t], jitter) for t in range(len(ops))]
    return np.stack([r["m"] for r in res]), np.stack([r["C"] for r in res])


class SvgpConditionOracleEngine(AR.SvgpAcquireOracleEngine):
    def svgp_condition(self, prep, X, Y, vmean=None, vchol=None, chunk=0):
        X = torch.as_tensor(X, dtype=torch.float64).cpu().numpy()
        Y = torch.as_tensor(Y, dtype=torch.float64).cpu().numpy()
        Y = Y[:, None] if Y.ndim == 1 else Y
        self.calls.setdefault("svgp_condition", []).append(int(X.shape[0]))
        ops = [to_oracle_params(p, X.shape[1]) for p in prep["params"]]
        vm, vc = condition(prep["Z"].numpy(), prep["vmean"].numpy(), prep["vchol"].numpy(), ops, X, Y, prep["jitter"])
        new = SR.SvgpOracleEngine.svgp_prepare(self, prep["params"], prep["Z"], vm, vc, prep["jitter"])
        if vmean is None:
            return new, None, None
        return new, new["vmean"], new["vchol"]
