"""Driven variant (optimization/Bayesian7.py): serving a trained batched SVGP on the GPU engine, and the pool scan.

SURVEY §8a row a9 and §8f row 2.  ``scripts/run_optimization.py:4`` drives ``Bayesian7.BayesianOptimizer``, whose
acquisition (``optimization/Bayesian7.py:646-688``) is: LHS candidate pool -> per 2048-candidate chunk
``likelihood(model(x_std)).variance.sum(0)`` -> ``torch.topk(K_big)`` -> ``farthest_point_sampling(batch_k)``.  Here the
predictive, the top-k and the FPS all run in libgpx (``gpx_svgp_*``, ``gpx_topk_f64``, ``gpx_fps_f64``).  A model
comes from one of two places: a checkpoint the reference trained (``batch_svgp.pt``, ``:702-707``) through
``SVGPModel.from_state_dict``, or ``SVGPModel.fit_collapsed``: for given hyperparameters and inducing points the
variational distribution the reference's Adam loop on the ELBO (``:451-538``) descends towards is known in closed form
(Gaussian likelihood: Titsias' collapsed posterior), and ``gpx_svgp_fit_collapsed_f64`` computes it.
``SVGPModel.fit`` also chooses the hyperparameters, by maximising that bound over all n points
(``gpx_svgp_bound_grad_f64``) and, with ``learn_inducing_locations=True``, moves Z along with them
(``gpx_svgp_bound_grad_z_f64``), as the reference's ``learn_inducing_locations=True`` does.  Minibatch training and
non-Gaussian likelihoods stay out of scope.

All arithmetic is fp64 (the reference model is float32; its variational jitter, 1e-4, is kept as the default).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import torch

from .engine import GPEngine, KernelParams
from .transforms import LogInputStandardizer

VARIATIONAL_JITTER_F32 = 1e-4  # gpytorch settings.variational_cholesky_jitter for float32 [upstream]
NOISE_LOWER_BOUND = 1e-4       # GaussianLikelihood noise constraint GreaterThan(1e-4) [upstream]


def _softplus(x: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.softplus(x.to(torch.float64))


@dataclass
class SVGPModel:
    """Trained state of Bayesian7's BatchSVGP (``optimization/Bayesian7.py:128-178``), T tasks (outputs).

    Z: T x M x d inducing points (standardized-log input space), vmean: T x M, vchol: T x M x M
    (chol_variational_covar; its lower triangle is used), params: per task ScaleKernel(Linear + Matérn-5/2)
    hyperparameters with ConstantMean ``const_mean`` and GaussianLikelihood ``noise``."""

    Z: torch.Tensor
    vmean: torch.Tensor
    vchol: torch.Tensor
    params: List[KernelParams]
    jitter: float = VARIATIONAL_JITTER_F32
    bound: Optional[torch.Tensor] = None  # fit_collapsed: T x 6 on the host, the collapsed bound F and its five terms
    hyper_result: Optional[object] = None  # fit: the MLLFitOutputsResult of the hyperparameter search

    @property
    def num_tasks(self) -> int:
        return self.Z.shape[0]

    @classmethod
    def fit_collapsed(cls, X, Y, params: Union[KernelParams, Sequence[KernelParams]], Z,
                      jitter: float = VARIATIONAL_JITTER_F32, engine: Optional[GPEngine] = None) -> "SVGPModel":
        """The model whose variational distribution is the optimum of the full-batch ELBO for the given
        hyperparameters (one KernelParams for all tasks, or one per task) and inducing points Z (M x d shared by the
        tasks, or T x M x d): ``GPEngine.svgp_fit_collapsed``.  X: n x d input-transformed, Y: n x T.  The bound's value
        and terms are kept as ``model.bound`` (T x 6, host)."""
        eng = engine or GPEngine()
        Y = torch.as_tensor(Y)
        if Y.dim() == 1:
            Y = Y.unsqueeze(-1)
        T = Y.shape[1]
        plist = [params] * T if isinstance(params, KernelParams) else list(params)
        Z = torch.as_tensor(Z).to(device=eng.device, dtype=torch.float64)
        if Z.dim() == 2:
            Z = Z.unsqueeze(0).expand(T, -1, -1)
        Z = Z.contiguous()
        vmean, vchol, bound = eng.svgp_fit_collapsed(plist, Z, X, Y, jitter=jitter)
        return cls(Z=Z, vmean=vmean, vchol=vchol, params=plist, jitter=jitter, bound=bound.cpu())

    @classmethod
    def fit(cls, X, Y, Z, params0: Union[KernelParams, Sequence[KernelParams]], prior_set: str = "none",
            fit_mean: bool = True, options: Optional[dict] = None, jitter: float = VARIATIONAL_JITTER_F32,
            engine: Optional[GPEngine] = None, value_grad_all=None,
            learn_inducing_locations: bool = False) -> "SVGPModel":
        """Hyperparameters and variational distribution together: the hyperparameters that maximise the collapsed
        bound over all n points, starting from ``params0`` (``mll.fit_hyperparameters_sparse``: L-BFGS-B on
        ``GPEngine.svgp_bound_value_grad``), then ``fit_collapsed`` at the result: the fixed point of the reference's
        joint ELBO training (``optimization/Bayesian7.py:451-538``) for the given inducing points.  With
        ``learn_inducing_locations`` the inducing points are optimised too, every task its own copy starting from
        ``Z``, and the model stands on the fitted ones (``model.hyper_result.Z``).  The optimiser's result is kept as
        ``model.hyper_result``."""
        from .mll import default_spec, fit_hyperparameters_sparse
        import numpy as np

        eng = engine or GPEngine()
        Y = torch.as_tensor(Y)
        if Y.dim() == 1:
            Y = Y.unsqueeze(-1)
        T, d = Y.shape[1], torch.as_tensor(X).shape[1]
        plist = [params0] * T if isinstance(params0, KernelParams) else list(params0)
        kind = plist[0].kind if isinstance(plist[0].kind, str) else \
            {0: "rbf", 1: "matern52", 2: "scale_linear_matern52"}[int(plist[0].kind)]
        x0 = np.concatenate([default_spec(kind, d, prior_set, p, fit_mean).raw_from_params(p) for p in plist])
        res = fit_hyperparameters_sparse(eng, X, Y, Z, kind, prior_set, bases=plist, fit_mean=fit_mean, options=options,
                                         value_grad_all=value_grad_all, x0=x0, jitter=jitter,
                                         learn_inducing=learn_inducing_locations)
        model = cls.fit_collapsed(X, Y, res.params, Z if res.Z is None else res.Z, jitter=jitter, engine=eng)
        model.hyper_result = res
        return model

    @classmethod
    def from_state_dict(cls, model_sd: dict, likelihood_sd: Optional[dict] = None,
                        jitter: float = VARIATIONAL_JITTER_F32) -> "SVGPModel":
        """Parameters of a gpytorch BatchSVGP / GaussianLikelihood state dict (the ``{"model": ..., "likelihood":
        ...}`` checkpoint of ``optimization/Bayesian7.py:702-707``; load it with ``torch.load(path,
        weights_only=True)``).  Raw parameters go through gpytorch's default constraints [upstream]: softplus
        (Positive) for lengthscale, LinearKernel variance and outputscale; softplus + 1e-4 for the noise."""
        g = lambda k: model_sd[k].to(torch.float64)  # noqa: E731
        Z = g("variational_strategy.inducing_points")
        vmean = g("variational_strategy._variational_distribution.variational_mean")
        vchol = g("variational_strategy._variational_distribution.chol_variational_covar")
        T, M, d = Z.shape
        ls = _softplus(model_sd["covar_module.base_kernel.kernels.1.raw_lengthscale"]).reshape(T, -1)
        lv = _softplus(model_sd["covar_module.base_kernel.kernels.0.raw_variance"]).reshape(T, -1)
        os_ = _softplus(model_sd["covar_module.raw_outputscale"]).reshape(T)
        if "mean_module.raw_constant" in model_sd:
            const = g("mean_module.raw_constant").reshape(T)
        else:
            const = g("mean_module.constant").reshape(T)
        noise = torch.full((T,), NOISE_LOWER_BOUND, dtype=torch.float64)
        if likelihood_sd is not None and "noise_covar.raw_noise" in likelihood_sd:
            noise = _softplus(likelihood_sd["noise_covar.raw_noise"]).reshape(T) + NOISE_LOWER_BOUND
        params = []
        for t in range(T):
            lvt = lv[t] if lv.shape[1] == d else lv[t].expand(d)
            params.append(KernelParams("scale_linear_matern52", [float(v) for v in ls[t]], outputscale=float(os_[t]),
                                       noise=float(noise[t]), const_mean=float(const[t]),
                                       linear_variance=[float(v) for v in lvt]))
        return cls(Z=Z, vmean=vmean, vchol=vchol, params=params, jitter=jitter)


class SVGPPredictor:
    """The SVGP predictive on the engine: ``predict`` ≙ ``likelihood(model(x_std))`` mean / variance
    (``optimization/Bayesian7.py:558,668``); ``pool_scan`` ≙ the acquisition block ``:646-688``."""

    def __init__(self, model: SVGPModel, engine: Optional[GPEngine] = None,
                 input_transform: Optional[LogInputStandardizer] = None, prep: Optional[dict] = None):
        """``prep``: the prepared state of ``model`` where the caller already has it (``condition_on_observations``);
        by default it is built here (``GPEngine.svgp_prepare``)."""
        self.engine = engine or GPEngine()
        self.model = model
        self.input_transform = input_transform
        if prep is None:
            prep = self.engine.svgp_prepare(model.params, model.Z, model.vmean, model.vchol, jitter=model.jitter)
        self.prep = prep

    def condition_on_observations(self, X: torch.Tensor, Y: torch.Tensor, transformed: bool = False) -> "SVGPPredictor":
        """A new predictor whose model knows the observations (X, Y) too (X: k x d, unit cube unless ``transformed``;
        Y: k x T): the exact update of q(u) on the device (``GPEngine.svgp_condition``), without a factorisation of
        K_ZZ, a pass over the old points or an ``svgp_prepare``.  Hyperparameters, Z and the jitter are kept; the new
        model's ``bound`` is None (the bound of the enlarged data cannot be updated from q alone).  This predictor and
        its model are left as they are."""
        m = self.model
        prep, vmean, vchol = self.engine.svgp_condition(self.prep, self._std(X, transformed), Y, vmean=m.vmean,
                                                        vchol=m.vchol)
        model = SVGPModel(Z=m.Z, vmean=vmean, vchol=vchol, params=m.params, jitter=m.jitter, bound=None)
        return SVGPPredictor(model, engine=self.engine, input_transform=self.input_transform, prep=prep)

    def _std(self, X: torch.Tensor, transformed: bool) -> torch.Tensor:
        X = X.to(device=self.engine.device, dtype=torch.float64)
        if transformed or self.input_transform is None:
            return X
        return self.input_transform(X).to(torch.float64)

    def predict(self, X: torch.Tensor, transformed: bool = False):
        """(mean, variance), each m x T, of the likelihood-wrapped predictive at X (unit cube unless
        ``transformed``)."""
        mean, var, _ = self.engine.svgp_predict(self.prep, self._std(X, transformed), want=("mean", "var"))
        return mean, var

    def uncertainty(self, X: torch.Tensor, transformed: bool = False) -> torch.Tensor:
        """Sum over tasks of the predictive variance (``pred.variance.sum(dim=0)``, ``:671``)."""
        _, _, score = self.engine.svgp_predict(self.prep, self._std(X, transformed), want=("score",))
        return score

    def pool_scan(self, cand_unit: torch.Tensor, batch_k: int, k_big_cap: int = 8000,
                  generator: Optional[torch.Generator] = None, start: Optional[int] = None):
        """Bayesian7's acquisition (``:646-688``): score the pool, keep the K_big most uncertain
        (K_big = min(max(5000, 20 batch_k), k_big_cap, pool)), then farthest-point-sample ``batch_k`` of them from a
        random start (``torch.randint``, ``:93``).  Returns (selected unit points batch_k x d, their pool indices)."""
        cand_unit = cand_unit.to(device=self.engine.device, dtype=torch.float64).contiguous()
        m = cand_unit.shape[0]
        score = self.uncertainty(cand_unit)
        k_big = int(min(max(5000, 20 * batch_k), k_big_cap, m))
        _, idx_big = self.engine.topk(score, k_big)
        cand_big = cand_unit.index_select(0, idx_big)
        if batch_k >= k_big:  # farthest_point_sampling returns its input unchanged (:89-90)
            return cand_big, idx_big
        if start is None:
            start = int(torch.randint(0, k_big, (1,), generator=generator).item())
        sel = self.engine.fps(cand_big, batch_k, start)
        return cand_big.index_select(0, sel), idx_big.index_select(0, sel)


def select_inducing_points(X: torch.Tensor, m: int, subset_size: int = 10000,
                           generator: Optional[torch.Generator] = None,
                           engine: Optional[GPEngine] = None) -> torch.Tensor:
    """Inducing points as ``optimization/Bayesian7.py:109-123`` picks them: a random subsample of ``subset_size`` rows
    of X when it has more, then farthest-point sampling (``GPEngine.fps``, random start) of min(m, rows) of them.
    ``generator``: a CPU torch.Generator for the two draws."""
    n = X.shape[0]
    if n > subset_size:
        X = X[torch.randperm(n, generator=generator)[:subset_size].to(X.device)]
        n = X.shape[0]
    m = min(int(m), n)
    if m >= n:  # farthest_point_sampling returns its input unchanged (:89-90)
        return X
    eng = engine or GPEngine()
    start = int(torch.randint(0, n, (1,), generator=generator).item())
    return X[eng.fps(X, m, start).to(X.device)]
