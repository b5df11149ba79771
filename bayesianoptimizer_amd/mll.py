"""Maximum-marginal-likelihood hyperparameter fit — the ``fit_gpytorch_mll`` step of the
reference (optimization/Bayesian.py:92-93, optimization/Bayesian1.py:114-115, optimization/Bayesian6.py:480-488).

Every objective evaluation runs on the GPU through the engine: Gram + Cholesky + L^{-T} + alpha
(``gpx_fit_f64``) and the fused K^{-1}-contraction gradient kernel (``gpx_mll_grad_f64``).  The host keeps only
what BoTorch/GPyTorch keep on the host [upstream]: the parameter transforms, the priors and scipy's L-BFGS-B.

Objective (ExactMarginalLogLikelihood [upstream], negated for minimisation):
    loss(raw) = ( -log p(y | theta) - sum_priors log prior(theta) ) / n,     theta = transform(raw)

Prior/constraint sets (the SingleTaskGP defaults differ by BoTorch version; the reference pins none):
  "dim_scaled"  BoTorch >= 0.12: RBF (or Matérn-5/2) ARD kernel without ScaleKernel;
                lengthscale LogNormal(sqrt2 + log(d)/2, sqrt3), constraint l >= 0.025 (no transform),
                initialised at the prior mode; noise LogNormal(-4, 1), constraint >= 1e-4 (no transform),
                initialised at the mode exp(-5); ConstantMean initialised at 0.
  "gamma"       BoTorch < 0.12: ScaleKernel(Matérn-5/2 ARD); lengthscale Gamma(3, 6) and outputscale Gamma(2, 0.15)
                through softplus (Positive), raw 0; noise Gamma(1.1, 0.05), constraint >= 1e-4 (no transform),
                initialised at the mode 2.0.
  "none"        no priors; softplus-positive lengthscale / outputscale / linear variances, noise >= 1e-4 through
                softplus (GaussianLikelihood default) — e.g. the ScaleKernel(Linear + Matérn-5/2) of
                optimization/Bayesian6.py:471-473.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np

from ._capi import GPXError
from .engine import KernelParams

SQRT2 = math.sqrt(2.0)
SQRT3 = math.sqrt(3.0)
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


# ---- priors ----------------------------------------------------------------------------------------
@dataclass(frozen=True)
class LogNormalPrior:
    loc: float
    scale: float

    def log_prob(self, x: float) -> float:
        z = (math.log(x) - self.loc) / self.scale
        return -math.log(x) - math.log(self.scale) - LOG_SQRT_2PI - 0.5 * z * z

    def dlog_prob(self, x: float) -> float:
        return -1.0 / x - (math.log(x) - self.loc) / (self.scale * self.scale * x)

    @property
    def mode(self) -> float:
        return math.exp(self.loc - self.scale * self.scale)


@dataclass(frozen=True)
class GammaPrior:
    concentration: float
    rate: float

    def log_prob(self, x: float) -> float:
        a, b = self.concentration, self.rate
        return a * math.log(b) - math.lgamma(a) + (a - 1.0) * math.log(x) - b * x

    def dlog_prob(self, x: float) -> float:
        return (self.concentration - 1.0) / x - self.rate

    @property
    def mode(self) -> float:
        return max(self.concentration - 1.0, 0.0) / self.rate


# ---- transforms --------------------------------------------------------------------------------------
def _softplus(r: float) -> float:
    return r + math.log1p(math.exp(-r)) if r > 0 else math.log1p(math.exp(r))


def _softplus_inv(x: float) -> float:
    return x + math.log(-math.expm1(-x)) if x < 30 else x


def _sigmoid(r: float) -> float:
    return 1.0 / (1.0 + math.exp(-r)) if r >= 0 else math.exp(r) / (1.0 + math.exp(r))


@dataclass
class Hyper:
    """One scalar hyperparameter: natural value = lower + softplus(raw) (softplus) or raw (identity)."""

    name: str                    # "noise" | "const_mean" | "outputscale" | "lengthscale" | "linear_variance"
    index: Optional[int]         # dimension for ARD entries
    transform: str               # "identity" | "softplus"
    lower: Optional[float]       # constraint lower bound (natural units)
    prior: Optional[object]      # LogNormalPrior | GammaPrior | None
    init: float                  # natural initial value

    def to_natural(self, raw: float) -> float:
        if self.transform == "softplus":
            return (self.lower or 0.0) + _softplus(raw)
        return raw

    def to_raw(self, nat: float) -> float:
        if self.transform == "softplus":
            return _softplus_inv(max(nat - (self.lower or 0.0), 1e-300))
        return nat

    def dnat_draw(self, raw: float) -> float:
        return _sigmoid(raw) if self.transform == "softplus" else 1.0

    def raw_bounds(self):
        if self.transform == "identity" and self.lower is not None:
            return (self.lower, None)
        return (None, None)


@dataclass
class HyperSpec:
    kind: str
    d: int
    hypers: List[Hyper]
    base: KernelParams                       # values of the parameters that are not fitted

    def params_from_raw(self, raw: np.ndarray) -> KernelParams:
        p = self.base.replace()
        ls = list(p.lengthscales(self.d))
        lv = list(p.linear_variances(self.d))
        kw = {}
        for h, r in zip(self.hypers, raw):
            v = h.to_natural(float(r))
            if h.name == "lengthscale":
                ls[h.index] = v
            elif h.name == "linear_variance":
                lv[h.index] = v
            else:
                kw[h.name] = v
        return p.replace(lengthscale=ls, linear_variance=lv, **kw)

    def x0(self) -> np.ndarray:
        return np.array([h.to_raw(h.init) for h in self.hypers], dtype=np.float64)

    def bounds(self):
        return [h.raw_bounds() for h in self.hypers]

    def raw_from_params(self, p: KernelParams) -> np.ndarray:
        """The raw vector at which ``params_from_raw`` gives the fitted entries of ``p`` (a start from known values)."""
        ls, lv = p.lengthscales(self.d), p.linear_variances(self.d)
        nat = [ls[h.index] if h.name == "lengthscale" else lv[h.index] if h.name == "linear_variance"
               else float(getattr(p, h.name)) for h in self.hypers]
        return np.array([h.to_raw(v) for h, v in zip(self.hypers, nat)], dtype=np.float64)


def default_spec(kind: str, d: int, prior_set: str = "dim_scaled", base: Optional[KernelParams] = None,
                 fit_mean: bool = True) -> HyperSpec:
    """The SingleTaskGP hyperparameters of the chosen BoTorch generation (module docstring)."""
    kind = kind.lower()
    hs: List[Hyper] = []
    if prior_set == "dim_scaled":
        lp = LogNormalPrior(SQRT2 + 0.5 * math.log(d), SQRT3)
        npr = LogNormalPrior(-4.0, 1.0)
        hs.append(Hyper("noise", None, "identity", 1e-4, npr, npr.mode))
        if fit_mean:
            hs.append(Hyper("const_mean", None, "identity", None, None, 0.0))
        hs += [Hyper("lengthscale", k, "identity", 2.5e-2, lp, lp.mode) for k in range(d)]
        outputscale = 1.0
    elif prior_set == "gamma":
        npr, opr, lpr = GammaPrior(1.1, 0.05), GammaPrior(2.0, 0.15), GammaPrior(3.0, 6.0)
        hs.append(Hyper("noise", None, "identity", 1e-4, npr, npr.mode))
        if fit_mean:
            hs.append(Hyper("const_mean", None, "identity", None, None, 0.0))
        hs.append(Hyper("outputscale", None, "softplus", 0.0, opr, _softplus(0.0)))
        hs += [Hyper("lengthscale", k, "softplus", 0.0, lpr, _softplus(0.0)) for k in range(d)]
        outputscale = _softplus(0.0)
    elif prior_set == "none":
        hs.append(Hyper("noise", None, "softplus", 1e-4, None, 1e-4 + _softplus(0.0)))
        if fit_mean:
            hs.append(Hyper("const_mean", None, "identity", None, None, 0.0))
        hs.append(Hyper("outputscale", None, "softplus", 0.0, None, _softplus(0.0)))
        hs += [Hyper("lengthscale", k, "softplus", 0.0, None, _softplus(0.0)) for k in range(d)]
        if kind == "scale_linear_matern52":
            hs += [Hyper("linear_variance", k, "softplus", 0.0, None, _softplus(0.0)) for k in range(d)]
        outputscale = _softplus(0.0)
    else:
        raise ValueError(f"unknown prior set '{prior_set}' (dim_scaled | gamma | none)")
    if base is None:
        base = KernelParams(kind, 1.0, outputscale=outputscale)
    spec = HyperSpec(kind=kind, d=d, hypers=hs, base=base.replace(kind=kind))
    # initial values of the fitted entries also seed ``base`` (used for anything not fitted)
    spec.base = spec.params_from_raw(spec.x0())
    return spec


# ---- objective -------------------------------------------------------------------------------------
def _feasible(spec: HyperSpec, raw) -> bool:
    """A line-search trial point outside the parameter domain (a softplus underflowing to 0, an overflow) scores +inf,
    so L-BFGS-B backtracks (GPyTorch's NaN loss plays that role in fit_gpytorch_mll_scipy [upstream])."""
    nat = [h.to_natural(float(r)) for h, r in zip(spec.hypers, raw)]
    return all(np.isfinite(v) for v in nat) and not any(v <= 0.0 for h, v in zip(spec.hypers, nat)
                                                        if h.name in ("lengthscale", "outputscale", "noise"))


def _loss_grad(spec: HyperSpec, raw, g: dict, n: int):
    """(loss, dloss/draw) of one output: (-log p(y) - sum_priors log prior) / n from the natural-parameter gradient
    dict ``g`` (ExactMarginalLogLikelihood's value divided by num_data [upstream])."""
    loss = g["nll"]
    grad = np.empty(len(spec.hypers))
    for i, (h, r) in enumerate(zip(spec.hypers, raw)):
        nat = h.to_natural(float(r))
        dn = g[h.name][h.index] if h.index is not None else g[h.name]
        if h.prior is not None:
            loss -= h.prior.log_prob(nat)
            dn = dn - h.prior.dlog_prob(nat)
        grad[i] = dn * h.dnat_draw(float(r))
    return loss / n, grad / n


def objective(spec: HyperSpec, value_grad: Callable, n: int):
    """loss(raw), dloss/draw with value_grad(params) -> dict of -log p(y) and its natural-parameter gradient
    (engine.mll_value_grad or the oracle's mll_value_grad)."""

    def f(raw):
        raw = np.asarray(raw, dtype=np.float64)
        if not _feasible(spec, raw):
            return np.inf, np.zeros_like(raw)
        try:
            g = value_grad(spec.params_from_raw(raw))
        except (GPXError, np.linalg.LinAlgError):  # indefinite through the jitter ladder: +inf, L-BFGS-B backtracks
            return np.inf, np.zeros_like(raw)
        if not np.isfinite(g["nll"]):
            return np.inf, np.zeros_like(raw)
        return _loss_grad(spec, raw, g, n)

    return f


def objective_outputs(specs: Sequence[HyperSpec], value_grad_all: Callable, n: int):
    """The multi-output loss over the concatenated raw vector [raw_0, raw_1, ...]: the sum of the per-output losses
    (BoTorch's fit_gpytorch_mll on a batched model sums the batch of ExactMarginalLogLikelihood values, each with its
    own prior terms [upstream]); value_grad_all(list of params) -> list of per-output dicts (one batched evaluation)."""
    sizes = [len(sp.hypers) for sp in specs]
    offs = np.concatenate([[0], np.cumsum(sizes)])

    def f(raw):
        raw = np.asarray(raw, dtype=np.float64)
        parts = [raw[offs[t]:offs[t + 1]] for t in range(len(specs))]
        if not all(_feasible(sp, r) for sp, r in zip(specs, parts)):
            return np.inf, np.zeros_like(raw)
        try:
            gs = value_grad_all([sp.params_from_raw(r) for sp, r in zip(specs, parts)])
        except (GPXError, np.linalg.LinAlgError):
            return np.inf, np.zeros_like(raw)
        if not all(np.isfinite(g["nll"]) for g in gs):
            return np.inf, np.zeros_like(raw)
        loss = 0.0
        grad = np.empty_like(raw)
        for t, (sp, r, g) in enumerate(zip(specs, parts, gs)):
            lt, gt = _loss_grad(sp, r, g, n)
            loss += lt
            grad[offs[t]:offs[t + 1]] = gt
        return loss, grad

    return f


@dataclass
class MLLFitResult:
    params: KernelParams
    loss: float                 # final (-mll) = (nll - log priors) / n
    nll: float                  # final -log p(y)
    n_evals: int
    success: bool
    message: str
    raw: np.ndarray = field(default_factory=lambda: np.zeros(0))


def fit_hyperparameters(engine, X, y, kind: str = "rbf", prior_set: str = "dim_scaled",
                        base: Optional[KernelParams] = None, fit_mean: bool = True,
                        options: Optional[dict] = None, value_grad: Optional[Callable] = None,
                        x0: Optional[Sequence[float]] = None) -> MLLFitResult:
    """L-BFGS-B over the raw hyperparameters, like fit_gpytorch_mll -> fit_gpytorch_mll_scipy [upstream].

    ``engine`` provides ``mll_value_grad(X, y, params)`` (GPEngine: GPU; tests inject the oracle through
    ``value_grad``).  ``options`` go to scipy.optimize.minimize (scipy's L-BFGS-B defaults otherwise).
    """
    from scipy.optimize import minimize

    Xn = np.asarray(X.cpu() if hasattr(X, "cpu") else X, dtype=np.float64)
    yn = np.asarray(y.cpu() if hasattr(y, "cpu") else y, dtype=np.float64)
    yn = yn.reshape(-1, 1) if yn.ndim == 1 else yn  # T columns share the hyperparameters
    n, d = Xn.shape
    spec = default_spec(kind, d, prior_set, base, fit_mean)
    if value_grad is None:
        state = [None]

        def value_grad(p):
            res, state[0] = engine.mll_value_grad(X, y, p, state=state[0])
            return res

    f = objective(spec, value_grad, n)
    last = {}

    def fg(raw):
        v, g = f(raw)
        last["v"] = v
        return v, g

    start = spec.x0() if x0 is None else np.asarray(x0, dtype=np.float64)
    res = minimize(fg, start, jac=True, method="L-BFGS-B", bounds=spec.bounds(), options=options or {})
    p = spec.params_from_raw(res.x)
    final = value_grad(p)
    loss, _ = f(res.x)
    return MLLFitResult(params=p, loss=float(loss), nll=float(final["nll"]), n_evals=int(res.nfev),
                        success=bool(res.success), message=str(res.message), raw=res.x.copy())


@dataclass
class MLLFitOutputsResult:
    params: List[KernelParams]  # one per output
    loss: float                 # final sum over outputs of (-mll_t)
    nll: List[float]            # final -log p(y_t) per output
    n_evals: int
    success: bool
    message: str
    raw: np.ndarray = field(default_factory=lambda: np.zeros(0))
    Z: Optional[np.ndarray] = None  # fit_hyperparameters_sparse(learn_inducing=True): the fitted T x M x d locations


def fit_hyperparameters_outputs(engine, X, Y, kind: str = "rbf", prior_set: str = "dim_scaled",
                                bases: Optional[Sequence[KernelParams]] = None, fit_mean: bool = True,
                                options: Optional[dict] = None, value_grad_all: Optional[Callable] = None,
                                x0: Optional[Sequence[float]] = None) -> MLLFitOutputsResult:
    """Hyperparameters of T independent outputs on one X (Y: n x T), each output its own set — the multi-output
    SingleTaskGP's fit_gpytorch_mll (optimization/Bayesian1.py:114-115 [upstream]): ONE L-BFGS-B over the concatenated
    raw vector on the summed loss.  Every evaluation is one batched fit of all outputs and one batched gradient
    (GPEngine.mll_value_grad_outputs); tests inject the oracle through ``value_grad_all``."""
    from scipy.optimize import minimize

    Xn = np.asarray(X.cpu() if hasattr(X, "cpu") else X, dtype=np.float64)
    Yn = np.asarray(Y.cpu() if hasattr(Y, "cpu") else Y, dtype=np.float64)
    Yn = Yn.reshape(-1, 1) if Yn.ndim == 1 else Yn
    n, d = Xn.shape
    T = Yn.shape[1]
    bases = list(bases) if bases is not None else [None] * T
    if len(bases) != T:
        raise ValueError(f"expected {T} base parameter sets, got {len(bases)}")
    specs = [default_spec(kind, d, prior_set, bases[t], fit_mean) for t in range(T)]
    if value_grad_all is None:
        state = [None]

        def value_grad_all(ps):
            res, state[0] = engine.mll_value_grad_outputs(X, Y, ps, states=state[0])
            return res

    f = objective_outputs(specs, value_grad_all, n)
    start = np.concatenate([sp.x0() for sp in specs]) if x0 is None else np.asarray(x0, dtype=np.float64)
    bounds = [b for sp in specs for b in sp.bounds()]
    res = minimize(f, start, jac=True, method="L-BFGS-B", bounds=bounds, options=options or {})
    sizes = np.concatenate([[0], np.cumsum([len(sp.hypers) for sp in specs])])
    ps = [sp.params_from_raw(res.x[sizes[t]:sizes[t + 1]]) for t, sp in enumerate(specs)]
    final = value_grad_all(ps)
    loss, _ = f(res.x)
    return MLLFitOutputsResult(params=ps, loss=float(loss), nll=[float(g["nll"]) for g in final],
                               n_evals=int(res.nfev), success=bool(res.success), message=str(res.message),
                               raw=res.x.copy())


def fit_hyperparameters_sparse(engine, X, Y, Z, kind: str = "scale_linear_matern52", prior_set: str = "none",
                               bases: Optional[Sequence[KernelParams]] = None, fit_mean: bool = True,
                               options: Optional[dict] = None, value_grad_all: Optional[Callable] = None,
                               x0: Optional[Sequence[float]] = None, jitter: float = 1e-4,
                               learn_inducing: bool = False) -> MLLFitOutputsResult:
    """``fit_hyperparameters_outputs`` with the collapsed SVGP bound F in the place of the marginal likelihood: the
    hyperparameters of T sparse models on inducing points Z (M x d shared, or T x M x d) that maximise F over all n
    points.  F is the ELBO of optimization/Bayesian7.py:451-538 with q(u) already at its optimum, so its maximiser is
    the fixed point of that joint training.  ONE L-BFGS-B over the concatenated raw vectors on the summed loss
    (-F_t - log priors) / n; every evaluation is one batched GPU evaluation (GPEngine.svgp_bound_value_grad), a failed
    K_ZZ scores +inf.  ``result.nll[t]`` = -F_t.  Tests inject a CPU reference through ``value_grad_all``.

    ``learn_inducing``: Z moves too, as the reference's ``learn_inducing_locations=True`` lets it
    (optimization/Bayesian7.py:152).  The L-BFGS-B vector is the raw hyperparameters followed by the T M d entries of Z
    (unbounded; every task its own copy, also of a shared Z, as the reference's expanded parameter becomes), the Z part
    of the gradient the evaluation's ``"inducing"`` arrays / n (GPEngine.svgp_bound_value_grad(inducing_grad=True)).
    Points that collide make K_ZZ fail: +inf, like any failed K_ZZ.  The search has two legs with the same ``options``:
    the hyperparameters alone on the given Z (the ``learn_inducing=False`` search), then the joint vector from that
    point.  L-BFGS-B does not leave a point for a worse one, so the loss never ends above the fixed-Z fit's.  (A joint
    search from the raw start spends its first steps on the T M d location entries, which dominate the gradient's norm,
    and within a small iteration budget ended behind the fixed-Z fit: 520 points, M = 130, 15 iterations, F = 438.64
    against 439.36.)  ``n_evals`` counts both legs.  An injected ``value_grad_all`` is then called as
    ``value_grad_all(params, Z)`` with the current T x M x d array.  ``result.Z`` is the fitted array (None when Z is
    not learned), ``result.raw`` the hyperparameters' part of the vector."""
    from scipy.optimize import minimize

    Xn = np.asarray(X.cpu() if hasattr(X, "cpu") else X, dtype=np.float64)
    Yn = np.asarray(Y.cpu() if hasattr(Y, "cpu") else Y, dtype=np.float64)
    Yn = Yn.reshape(-1, 1) if Yn.ndim == 1 else Yn
    n, d = Xn.shape
    T = Yn.shape[1]
    bases = list(bases) if bases is not None else [None] * T
    if len(bases) != T:
        raise ValueError(f"expected {T} base parameter sets, got {len(bases)}")
    specs = [default_spec(kind, d, prior_set, bases[t], fit_mean) for t in range(T)]
    if learn_inducing:
        Zn = np.array(Z.detach().cpu().numpy() if hasattr(Z, "cpu") else Z, dtype=np.float64)
        Zn = np.repeat(Zn[None], T, axis=0) if Zn.ndim == 2 else Zn
        if Zn.ndim != 3 or Zn.shape[0] != T:
            raise ValueError(f"Z must be M x d or {T} x M x d")
        at_start = None if value_grad_all is None else (lambda ps: value_grad_all(ps, Zn))
        first = fit_hyperparameters_sparse(engine, X, Yn, Zn, kind, prior_set, bases=bases, fit_mean=fit_mean,
                                           options=options, value_grad_all=at_start, x0=x0, jitter=jitter)
        return _fit_sparse_with_inducing(engine, X, Yn, Zn, specs, n, options, value_grad_all, first, jitter)
    if value_grad_all is None:
        import torch

        Zd = torch.as_tensor(Z).to(device=engine.device, dtype=torch.float64)
        Zd = (Zd.unsqueeze(0).expand(T, -1, -1) if Zd.dim() == 2 else Zd).contiguous()
        Xd = torch.as_tensor(X).to(device=engine.device, dtype=torch.float64)
        Yd = torch.as_tensor(Yn).to(device=engine.device, dtype=torch.float64)

        def value_grad_all(ps):
            return engine.svgp_bound_value_grad(ps, Zd, Xd, Yd, jitter=jitter)

    f = objective_outputs(specs, value_grad_all, n)
    start = np.concatenate([sp.x0() for sp in specs]) if x0 is None else np.asarray(x0, dtype=np.float64)
    bounds = [b for sp in specs for b in sp.bounds()]
    res = minimize(f, start, jac=True, method="L-BFGS-B", bounds=bounds, options=options or {})
    sizes = np.concatenate([[0], np.cumsum([len(sp.hypers) for sp in specs])])
    ps = [sp.params_from_raw(res.x[sizes[t]:sizes[t + 1]]) for t, sp in enumerate(specs)]
    loss, _ = f(res.x)
    nll = [float("inf")] * T
    if np.isfinite(loss):
        nll = [float(g["nll"]) for g in value_grad_all(ps)]
    return MLLFitOutputsResult(params=ps, loss=float(loss), nll=nll, n_evals=int(res.nfev), success=bool(res.success),
                               message=str(res.message), raw=res.x.copy())


def _fit_sparse_with_inducing(engine, X, Yn, Zn, specs, n, options, value_grad_all, first,
                              jitter) -> MLLFitOutputsResult:
    """fit_hyperparameters_sparse(learn_inducing=True), second leg: the vector is [raw hyperparameters, Z.ravel()],
    started at the fixed-Z fit ``first`` on Zn (T x M x d)."""
    from scipy.optimize import minimize

    T = len(specs)
    if value_grad_all is None:
        import torch

        Xd = torch.as_tensor(X).to(device=engine.device, dtype=torch.float64)
        Yd = torch.as_tensor(Yn).to(device=engine.device, dtype=torch.float64)

        def value_grad_all(ps, Zc):
            return engine.svgp_bound_value_grad(ps, torch.as_tensor(Zc).to(engine.device), Xd, Yd, jitter=jitter,
                                                inducing_grad=True)

    sizes = np.concatenate([[0], np.cumsum([len(sp.hypers) for sp in specs])])
    nh = int(sizes[-1])

    def f(x):
        x = np.asarray(x, dtype=np.float64)
        Zc = x[nh:].reshape(Zn.shape)
        seen = {}

        def at_z(ps):
            seen["g"] = value_grad_all(ps, Zc)
            return seen["g"]

        loss, gh = objective_outputs(specs, at_z, n)(x[:nh])
        if not np.isfinite(loss):
            return np.inf, np.zeros_like(x)
        gz = np.concatenate([np.asarray(g["inducing"], dtype=np.float64).ravel() for g in seen["g"]]) / n
        return loss, np.concatenate([gh, gz])

    bounds = [b for sp in specs for b in sp.bounds()] + [(None, None)] * Zn.size
    res = minimize(f, np.concatenate([first.raw, Zn.ravel()]), jac=True, method="L-BFGS-B", bounds=bounds,
                   options=options or {})
    ps = [sp.params_from_raw(res.x[sizes[t]:sizes[t + 1]]) for t, sp in enumerate(specs)]
    Zfit = res.x[nh:].reshape(Zn.shape).copy()
    loss, _ = f(res.x)
    nll = [float("inf")] * T
    if np.isfinite(loss):
        nll = [float(g["nll"]) for g in value_grad_all(ps, Zfit)]
    return MLLFitOutputsResult(params=ps, loss=float(loss), nll=nll, n_evals=first.n_evals + int(res.nfev),
                               success=bool(res.success), message=str(res.message), raw=res.x[:nh].copy(), Z=Zfit)
