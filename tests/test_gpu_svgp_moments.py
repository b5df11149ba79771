"""GPU tests of gpx_svgp_moments_grad_f64 (GPEngine.svgp_moments_grad): the q-batch moments of one SVGP task and their
candidate derivatives against the NumPy reference by triangular solves (tests/svgp_moments_ref.py), the value-only
form, determinism, consistency with gpx_svgp_predict_f64, task selection, argument validation, and what stands on the
call: acqf's MC acquisitions and optimize_acqf on a models.SparseGP, and the drop-in's "qpsd" round.

Tolerances are the project's for gpx_moments_grad_f64 (tests/test_acqf.py): mean 1e-9 of max|mean|, cov 1e-9 of the prior
variance scale, dmean and dcov 1e-8 of the largest reference entry."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import _capi, acqf
from bayesianoptimizer_amd._capi import GPXError
from bayesianoptimizer_amd.models import SparseGP
from tests import mc_acq_ref
from tests import svgp_moments_ref as SR
from tests.ard_util import ard_params
from tests.oracle_engine import to_oracle_params

pytestmark = pytest.mark.gpu


def dev(engine, a):
    return torch.tensor(np.array(a, dtype=np.float64), device=engine.device)


def prepare(engine, kps, Z, vmean, vchol):
    """GPEngine.svgp_prepare of T tasks: Z (T, M, d), vmean (T, M), vchol (T, M, M) as NumPy arrays."""
    return engine.svgp_prepare(kps, dev(engine, Z), dev(engine, vmean), dev(engine, vchol), jitter=SR.JITTER)


@functools.lru_cache(maxsize=None)
def case(M, d, q, B, kind, model):
    """(kp, op, Z, Xs, vmean, vchol, reference moments) of one shape, kind and model, computed once; the fitted model's
    state is sgpr_ref's closed form (the GPU fit itself is tests/test_gpu_svgp_collapsed.py's subject)."""
    from tests import sgpr_ref as R

    kp, op, Z, X, y, Xs, vmean, vchol = SR.problem(M, d, q, B, kind)
    if model == "fit":
        fit = R.fit_collapsed_task(Z, X, y, op, SR.JITTER)
        vmean, vchol = fit["m"], fit["C"]
    ref = SR.moments_grad(Z, vmean, vchol, op, Xs, q)
    return kp, op, Z, Xs, vmean, vchol, ref


def check_moments(got, ref, op, Xs, what):
    mean, dmean, cov, dcov = (v.cpu().numpy() for v in got)
    rm, rdm, rc, rdc = ref
    ps = SR.prior_scale(op, Xs)
    e = (np.abs(mean - rm).max() / np.abs(rm).max(), np.abs(dmean - rdm).max() / np.abs(rdm).max(),
         np.abs(cov - rc).max() / ps, np.abs(dcov - rdc).max() / np.abs(rdc).max())
    print(f"{what}: |d mean| {e[0]:.1e}  |d dmean| {e[1]:.1e}  |d cov| / prior {e[2]:.1e}  |d dcov| {e[3]:.1e}")
    assert np.isfinite(rdm).all() and np.isfinite(rdc).all()
    assert e[0] <= 1e-9 and e[2] <= 1e-9, what
    assert e[1] <= 1e-8 and e[3] <= 1e-8, what


@pytest.mark.parametrize("model", ["fit", "arbitrary"])
@pytest.mark.parametrize("kind", SR.KINDS)
@pytest.mark.parametrize("M,d,q,B", SR.SHAPES)
def test_moments_match_reference(engine, M, d, q, B, kind, model):
    """Every shape of svgp_moments_ref.SHAPES, the three kinds with ARD parameters, the closed-form fit of 600 points
    and an arbitrary state with S S^T <= I violated.  The value-only call returns the gradient call's mean and cov bit
    for bit, and a second call repeats the first."""
    kp, op, Z, Xs, vmean, vchol, ref = case(M, d, q, B, kind, model)
    prep = prepare(engine, [kp], Z[None], vmean[None], vchol[None])
    got = engine.svgp_moments_grad(prep, 0, dev(engine, Xs), q)
    check_moments(got, ref, op, Xs, f"M={M} d={d} q={q} B={B} {kind} {model}")
    mean, dmean, cov, dcov = engine.svgp_moments_grad(prep, 0, dev(engine, Xs), q, need_grad=False)
    assert dmean is None and dcov is None
    assert torch.equal(mean, got[0]) and torch.equal(cov, got[2])
    again = engine.svgp_moments_grad(prep, 0, dev(engine, Xs), q)
    assert all(torch.equal(a, b) for a, b in zip(again, got))


@pytest.mark.parametrize("kind", SR.KINDS)
@pytest.mark.parametrize("model", ["fit", "arbitrary"])
def test_q1_is_the_predictive_without_noise_and_floor(engine, kind, model):
    kp, op, Z, Xs, vmean, vchol, _ = case(200, 5, 3, 3, kind, model)
    Xq = dev(engine, np.random.default_rng(5).random((300, 5)))
    prep = prepare(engine, [kp], Z[None], vmean[None], vchol[None])
    mu, var, _ = engine.svgp_predict(prep, Xq, min_var=1e-10, want=("mean", "var"))
    mean, _, cov, _ = engine.svgp_moments_grad(prep, 0, Xq, 1, need_grad=False)
    mu, var, mean, cov = (v.cpu().numpy().reshape(-1) for v in (mu, var, mean, cov))
    assert np.abs(mean - mu).max() <= 1e-9 * np.abs(mu).max()
    keep = var > 1e-10
    assert keep.sum() > 250
    assert np.abs(cov + op.noise - var)[keep].max() <= 1e-9 * SR.prior_scale(op, Xq.cpu().numpy())


def test_task_selection(engine):
    """T = 2 with different Z and hyperparameters: task 1 of the joint prepare is the single-task prepare of its data."""
    a = case(200, 5, 3, 3, "matern52", "fit")
    b = case(200, 5, 3, 3, "scale_linear_matern52", "arbitrary")
    both = prepare(engine, [a[0], b[0]], np.stack([a[2], b[2]]), np.stack([a[4], b[4]]), np.stack([a[5], b[5]]))
    single = prepare(engine, [b[0]], b[2][None], b[4][None], b[5][None])
    Xs = dev(engine, b[3])
    got = engine.svgp_moments_grad(both, 1, Xs, 3)
    check_moments(got, b[6], b[1], b[3], "task 1 of 2")
    assert all(torch.equal(x, y) for x, y in zip(got, engine.svgp_moments_grad(single, 0, Xs, 3)))
    with pytest.raises(ValueError):
        engine.svgp_moments_grad(both, 2, Xs, 3)


def test_invalid_arguments_launch_nothing(engine):
    kp, op, Z, Xs, vmean, vchol, ref = case(50, 4, 4, 2, "rbf", "fit")
    prep = prepare(engine, [kp], Z[None], vmean[None], vchol[None])
    M, d, m, q = 50, 4, 8, 4
    X = dev(engine, Xs)
    f64 = dict(dtype=torch.float64, device=engine.device)
    mean, dmean, cov, dcov = (torch.full(s, -7.0, **f64) for s in ((m,), (m, d), (m, q), (m, d, q)))
    nb = ctypes.c_size_t()
    assert engine.lib.gpx_svgp_moments_grad_workspace_size(M, m, ctypes.byref(nb)) == _capi.GPX_OK
    ws = torch.empty(nb.value, dtype=torch.uint8, device=engine.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
    pc = kp.to_c(d)

    def call(m=m, q=q, dmean=dmean, dcov=dcov, ws_bytes=nb.value, Zt=prep["Z"][0]):
        engine._bind_stream()
        return engine.lib.gpx_svgp_moments_grad_f64(
            engine.handle, ctypes.byref(pc), M, p(Zt), d, p(prep["W"][0]), p(prep["W2"][0]), p(prep["alpha"][0]), p(X),
            m, q, d, p(mean), p(dmean), p(cov), p(dcov), p(ws), ws_bytes)

    for bad in (dict(q=3), dict(q=_capi.GPX_MAX_Q + 1, m=2 * (_capi.GPX_MAX_Q + 1)), dict(dcov=None), dict(dmean=None),
                dict(ws_bytes=nb.value - 1), dict(Zt=None)):
        assert call(**bad) == _capi.GPX_INVALID_ARG, bad
        assert engine.lib.gpx_last_error(engine.handle)
    torch.cuda.synchronize()
    assert all(bool((v == -7.0).all()) for v in (mean, dmean, cov, dcov)), "a rejected call wrote its outputs"
    assert call() == _capi.GPX_OK
    check_moments((mean, dmean, cov, dcov), ref, op, Xs, "after the rejected calls")
    with pytest.raises(ValueError):
        engine.svgp_moments_grad(prep, 0, X[:7], 4)
    with pytest.raises(GPXError):
        engine.svgp_moments_grad(prep, 0, X.repeat(9, 1)[:66], _capi.GPX_MAX_Q + 1)


# ---- acqf on a SparseGP -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sparse_inputs():
    """Two outputs on d = 4, each with its own kernel parameters, M = 40 inducing points of n = 300."""
    rng = np.random.default_rng(12)
    n, d, M = 300, 4, 40
    X = rng.random((n, d))
    Y = np.stack([np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 + 0.05 * rng.standard_normal(n),
                  np.cos(2.0 * X[:, 2]) - 0.5 * X[:, 3] + 0.05 * rng.standard_normal(n)], axis=1)
    Z = X[rng.permutation(n)[:M]]
    kps = [ard_params("scale_linear_matern52", d, 3, noise=1e-2, const_mean=0.1)[0],
           ard_params("matern52", d, 4, noise=2e-2, outputscale=0.8, const_mean=-0.2)[0]]
    return X, Y, Z, kps


def sparse_model(engine):
    X, Y, Z, kps = sparse_inputs()
    gp = SparseGP(dev(engine, X), dev(engine, Y), kps, dev(engine, Z), jitter=SR.JITTER, engine=engine)
    state = [(gp.svgp.Z[t].cpu().numpy(), gp.svgp.vmean[t].cpu().numpy(), gp.svgp.vchol[t].cpu().numpy(),
              to_oracle_params(kps[t], 4)) for t in range(2)]
    return gp, state


def reference_objective(state, weights, Xq, differentiable=False):
    """Mean (B, q) and covariance (B, q, q) of sum_t w_t f_t from the reference moments (NumPy), or from the torch
    restatement when the gradient is wanted."""
    B, q, d = Xq.shape
    mu, cov = 0.0, 0.0
    for (Z, vm, vc, op), w in zip(state, weights):
        if w == 0.0:
            continue
        if differentiable:
            m_t, c_t = SR.torch_moments(Z, vm, vc, op, Xq)
        else:
            m_t, _, c_t, _ = SR.moments_grad(Z, vm, vc, op, Xq.reshape(B * q, d), q)
            m_t, c_t = torch.tensor(m_t).reshape(B, q), torch.tensor(c_t).reshape(B, q, q)
        mu, cov = mu + w * m_t, cov + w * w * c_t
    return mu, cov


@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("name", ["qpsd", "qlogei"])
def test_acquisitions_on_a_sparse_model_match_the_reference(engine, name, q):
    gp, state = sparse_model(engine)
    seed, B = 11, 5
    if name == "qpsd":
        a = acqf.qPosteriorStandardDeviation(gp, acqf.SobolQMCNormalSampler(torch.Size([256]), seed), output=1)
        weights = (0.0, 1.0)
    else:
        Y = sparse_inputs()[1]
        weights = (0.5, 0.5)
        best_f = float((Y @ np.array(weights)).max())
        a = acqf.qLogExpectedImprovement(gp, best_f=best_f, sampler=acqf.SobolQMCNormalSampler(torch.Size([256]), seed),
                                         objective=acqf.LinearMCObjective(weights))
    z = a.sampler.base_samples(q, engine.device).cpu()

    def value(mu, cov):
        if name == "qlogei":
            return acqf.qlogei_from_moments(mu, cov, z, best_f)
        return mc_acq_ref.qpsd_closed_form(torch.linalg.cholesky(0.5 * (cov + cov.transpose(1, 2))), z)

    Xq = np.random.default_rng(q).random((B, q, 4))
    Xg = dev(engine, Xq).requires_grad_(True)
    got = a(Xg)
    (g,) = torch.autograd.grad(got.sum(), Xg)
    ref = value(*reference_objective(state, weights, Xq))
    np.testing.assert_allclose(got.detach().cpu().numpy(), ref.numpy(), rtol=1e-8)
    Xt = torch.tensor(Xq, requires_grad=True)
    (gr,) = torch.autograd.grad(value(*reference_objective(state, weights, Xt, differentiable=True)).sum(), Xt)
    err = (g.cpu() - gr).abs().max().item()
    print(f"{name} q={q}: |d grad| / max|grad| = {err / gr.abs().max().item():.1e}")
    assert err <= 1e-6 * gr.abs().max().item()


def test_optimize_acqf_on_a_sparse_model(engine, monkeypatch):
    gp, _ = sparse_model(engine)
    a = acqf.qPosteriorStandardDeviation(gp, acqf.SobolQMCNormalSampler(torch.Size([128]), 4), output=0)
    calls = []
    inner = engine.svgp_moments_grad

    def recorded(prep, task, Xs, q=1, need_grad=True):
        calls.append((int(Xs.shape[0]), int(q), bool(need_grad)))
        return inner(prep, task, Xs, q, need_grad)

    monkeypatch.setattr(engine, "svgp_moments_grad", recorded)
    q = 4
    bounds = torch.tensor([[0.0] * 4, [1.0] * 4], dtype=torch.float64)
    X0 = acqf.gen_batch_initial_conditions(a, bounds.to(engine.device), q, 4, 64, seed=5, nonnegative=True)
    assert calls == [(64 * q, q, False)], "the raw samples are scored by one value-only call"
    with torch.no_grad():
        v0 = a(X0).max().item()
    cand, val = acqf.optimize_acqf(a, bounds, q=q, num_restarts=4, raw_samples=64,
                                   options={"batch_limit": 2, "maxiter": 40, "nonnegative": True}, seed=5)
    assert cand.shape == (q, 4) and float(cand.min()) >= 0.0 and float(cand.max()) <= 1.0
    assert val.item() >= v0 - 1e-9
    assert any(c[2] for c in calls), "L-BFGS-B evaluates the gradient call"


def test_dropin_qpsd_round_on_the_sparse_model(tmp_path, engine):
    SR.dropin_round(SR.dropin_optimizer(tmp_path, "qpsd", engine=engine))
