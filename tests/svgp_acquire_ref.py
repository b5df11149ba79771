"""CPU reference of gpx_svgp_acquire_f64 (include/gpx.h): the analytic acquisition of a linear objective over the tasks of
a sparse model, from the LATENT predictive.

* ``latent_moments``: ``oracle.gp_oracle.svgp_predict`` with every task's likelihood noise set to 0 and GPyTorch's 1e-10
  floor: mean and latent variance per task (m x T).
* ``objective_scores``: mean sum_t w_t (y_mean_t + y_scale_t mu_t), variance max(sum_t w_t^2 y_scale_t^2 var_t, 1e-12),
  scored by ``oracle.gp_oracle.acquisition``.
* ``SvgpAcquireOracleEngine``: tests/svgp_moments_ref.SvgpOracleEngine plus ``svgp_acquire`` answered from the two above,
  for the sparse model's sweeps and the drop-in without a GPU.
"""
import dataclasses

import numpy as np
import torch

from oracle import gp_oracle as O
from tests import svgp_moments_ref as SR
from tests.oracle_engine import to_oracle_params

KINDS = {"ei": O.ACQ_EI, "logei": O.ACQ_LOGEI, "ucb": O.ACQ_UCB, "variance": O.ACQ_VARIANCE}


def latent_moments(Z, vmean, vchol, ops, Xs, jitter=SR.JITTER):
    """(mean, var), each m x T: the predictive of f, not of y."""
    latent = [dataclasses.replace(p, noise=0.0) for p in ops]
    mean, var, _ = O.svgp_predict(Z, vmean, vchol, latent, Xs, jitter=jitter, min_var=O.GPYTORCH_MIN_VAR_F64)
    return mean, var


def objective_scores(mean, var, kind, weights, y_mean=None, y_scale=None, best_f=0.0, beta=4.0):
    T = mean.shape[1]
    w = np.asarray(weights, dtype=np.float64)
    ym = np.zeros(T) if y_mean is None else np.asarray(y_mean, dtype=np.float64)
    ys = np.ones(T) if y_scale is None else np.asarray(y_scale, dtype=np.float64)
    mu = (w * (ym + ys * mean)).sum(1)
    v = np.maximum(((w * w) * (ys * ys) * var).sum(1), O.BOTORCH_MIN_VAR)
    return O.acquisition(mu, v, KINDS[kind] if isinstance(kind, str) else int(kind), best_f, beta)


class SvgpAcquireOracleEngine(SR.SvgpOracleEngine):
    def svgp_acquire(self, prep, Xs, k, kind="logei", best_f=0.0, beta=4.0, weights=None, y_mean=None, y_scale=None,
                     index_offset=0, return_scores=False):
        Xs = torch.as_tensor(Xs, dtype=torch.float64).cpu().numpy()
        T, d, m, k = prep["Z"].shape[0], Xs.shape[1], Xs.shape[0], int(k)
        if not 1 <= k <= m:
            raise ValueError("k must be in [1, m]")
        self.calls.setdefault("svgp_acquire", []).append((m, k, kind))
        mean, var = latent_moments(prep["Z"].numpy(), prep["vmean"].numpy(), prep["vchol"].numpy(),
                                   [to_oracle_params(p, d) for p in prep["params"]], Xs, prep["jitter"])
        scores = objective_scores(mean, var, kind, [1.0] * T if weights is None else weights, y_mean, y_scale, best_f,
                                  beta)
        val, idx = O.topk_desc(scores, k)
        out = (torch.tensor(val), torch.tensor(idx + int(index_offset), dtype=torch.int64))
        return out + (torch.tensor(scores),) if return_scores else out
