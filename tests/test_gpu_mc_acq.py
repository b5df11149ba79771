"""GPU tests of gpx_mc_acq_f64 (fused MC q-batch acquisition: qLogEI with either q-reduction, qPSD) against the torch
CPU reference tests/mc_acq_ref.py on synthetic moments, and of the acqf / drop-in paths built on it.

Tolerances: values rtol = atol = 1e-8 (the project's qLogEI tolerance, tests/test_acqf.py); gradients norm-wise,
max|g - g_ref| <= 1e-8 max|g_ref| per q-batch (entries that cancel to near zero carry the absolute error of the large
ones).  The largest deviations seen on the device are recorded in DESIGN.md §4."""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import _capi, acqf
from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
from tests import mc_acq_ref as R
from tests.stubs import BOUNDS, StubSimulator
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

TOL = 1e-8
MODES = {"fatplus_fatmax": ("qlogei", True, True), "fatplus_lse": ("qlogei", True, False),
         "softplus_fatmax": ("qlogei", False, True), "softplus_lse": ("qlogei", False, False),
         "qpsd": ("qpsd", True, False)}


def _best_f(mean):
    return float(mean.median())  # inside the range of f


def _run(engine, mean, cov, z, mode, best_f, need_grad=True):
    kind, fat_relu, fat_max = MODES[mode]
    out = engine.mc_acq(mean.to(DEV), cov.to(DEV), z.to(DEV), kind, best_f=best_f, fat_relu=fat_relu, fat_max=fat_max,
                        need_grad=need_grad)
    return tuple(None if o is None else o.cpu() for o in out)


def _ref(mean, cov, z, mode, best_f):
    kind, fat_relu, fat_max = MODES[mode]
    return R.mc_acq(mean, cov, z, kind, best_f=best_f, fat_relu=fat_relu, fat_max=fat_max)


def _grad_dev(g, ref):
    """largest per-batch norm-wise deviation max|g - ref| / max|ref|"""
    B = ref.shape[0]
    num = (g - ref).abs().reshape(B, -1).amax(dim=1)
    den = ref.abs().reshape(B, -1).amax(dim=1)
    return float((num / den).max())


def _check(got, ref, mode, what):
    value, gmean, gcov, info = got
    rv, rgm, rgc, rinfo = ref
    dv = float(((value - rv).abs() / (1.0 + rv.abs())).max())
    dgc = _grad_dev(gcov, rgc)
    dgm = float(gmean.abs().max()) if mode == "qpsd" else _grad_dev(gmean, rgm)
    print(f"mc_acq {mode} {what}: value dev {dv:.2e} gmean dev {dgm:.2e} gcov dev {dgc:.2e}")
    assert torch.equal(info, rinfo)
    np.testing.assert_allclose(value.numpy(), rv.numpy(), rtol=TOL, atol=TOL)
    if mode == "qpsd":
        assert dgm == 0.0  # exactly zero
    else:
        assert dgm <= TOL
    assert dgc <= TOL


@pytest.mark.parametrize("q", [1, 2, 5, 32])
@pytest.mark.parametrize("mode", list(MODES))
def test_value_and_gradients_match_reference(engine, mode, q):
    """q: no off-diagonal, the smallest factor, an odd size, the limit; S: below a wave, a full wave, no multiple of the
    workgroup (2 for qPSD: its least); B: one batch, a few, many."""
    for S in ([2, 3, 64, 257] if mode == "qpsd" else [3, 64, 257]):
        z = R.base_samples(S, q, seed=100 + S)
        for B in (1, 3, 70):
            mean, cov = R.synthetic_moments(B, q, seed=1000 * q + 10 * S + B)
            best_f = _best_f(mean)
            _check(_run(engine, mean, cov, z, mode, best_f), _ref(mean, cov, z, mode, best_f), mode,
                   f"q={q} S={S} B={B}")


def _with_neighbours(mid):
    mean, cov = R.synthetic_moments(3, 2, seed=5)
    cov = cov.clone()
    cov[1] = torch.tensor(mid, dtype=torch.float64)
    return mean, cov


@pytest.mark.parametrize("mode", ["fatplus_fatmax", "qpsd"])
def test_jitter_retry_is_per_batch(engine, mode):
    # second pivot 1 - (1 + 1e-9)^2 = -2e-9; with 1e-8 on the diagonal it is +1.8e-8
    mean, cov = _with_neighbours([[1.0, 1.0 + 1e-9], [1.0 + 1e-9, 1.0]])
    z = R.base_samples(64, 2, seed=3)
    best_f = _best_f(mean)
    got, ref = _run(engine, mean, cov, z, mode, best_f), _ref(mean, cov, z, mode, best_f)
    assert got[3].tolist() == [0, 1, 0]
    _check(got, ref, mode, "jitter batch")


def test_not_positive_definite_batch_is_nan_and_raises(engine):
    mean, cov = _with_neighbours([[1.0, 2.0], [2.0, 1.0]])
    z = R.base_samples(64, 2, seed=3)
    best_f = _best_f(mean)
    value, gmean, gcov, info = _run(engine, mean, cov, z, "fatplus_fatmax", best_f)
    rv, rgm, rgc, rinfo = _ref(mean, cov, z, "fatplus_fatmax", best_f)
    assert info.tolist() == rinfo.tolist() == [0, -1, 0]
    assert bool(value[1].isnan()) and bool(gmean[1].isnan().all()) and bool(gcov[1].isnan().all())
    for b in (0, 2):
        np.testing.assert_allclose(value[b].item(), rv[b].item(), rtol=TOL, atol=TOL)
        assert _grad_dev(gmean[b:b + 1], rgm[b:b + 1]) <= TOL and _grad_dev(gcov[b:b + 1], rgc[b:b + 1]) <= TOL
    opts = {"best_f": best_f, "fat_relu": True, "fat_max": True, "tau_max": 1e-2, "tau_relu": 1e-6}
    with pytest.raises(torch.linalg.LinAlgError):
        acqf._McAcq.apply(mean.to(DEV), cov.to(DEV), engine, z.to(DEV), "qlogei", opts)


@pytest.mark.parametrize("mode", ["fatplus_lse", "qpsd"])
def test_asymmetric_covariance_is_symmetrised(engine, mode):
    mean, cov = R.synthetic_moments(3, 5, seed=9)
    z = R.base_samples(64, 5, seed=4)
    K = torch.randn(3, 5, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    skew = 0.1 * (K - K.transpose(1, 2))
    best_f = _best_f(mean)
    a = _run(engine, mean, cov + skew, z, mode, best_f)
    b = _run(engine, mean, 0.5 * ((cov + skew) + (cov + skew).transpose(1, 2)), z, mode, best_f)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    _check(a, _ref(mean, cov, z, mode, best_f), mode, "asymmetric")


@pytest.mark.parametrize("mode", ["fatplus_fatmax", "softplus_lse", "qpsd"])
def test_value_only_and_repeat_calls_are_bit_equal(engine, mode):
    mean, cov = R.synthetic_moments(70, 5, seed=2)
    z = R.base_samples(257, 5, seed=6)
    best_f = _best_f(mean)
    full = _run(engine, mean, cov, z, mode, best_f)
    again = _run(engine, mean, cov, z, mode, best_f)
    value_only = _run(engine, mean, cov, z, mode, best_f, need_grad=False)
    assert value_only[1] is None and value_only[2] is None
    assert torch.equal(value_only[0], full[0]) and torch.equal(value_only[3], full[3])
    for x, y in zip(full, again):
        assert torch.equal(x, y)


def test_invalid_arguments_launch_nothing(engine):
    B, q, S = 2, 3, 8
    mean, cov = R.synthetic_moments(B, q, seed=1)
    mean, cov, z = mean.to(DEV), cov.to(DEV), R.base_samples(S, q, seed=1).to(DEV)
    value = torch.full((B,), 7.0, dtype=torch.float64, device=DEV)
    gmean = torch.full((B, q), 7.0, dtype=torch.float64, device=DEV)
    gcov = torch.full((B, q, q), 7.0, dtype=torch.float64, device=DEV)
    info = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)

    def call(kind=_capi.MCACQ_QLOGEI, fat_relu=1, fat_max=1, reserved=0, tau_relu=1e-6, tau_max=1e-2, q_=q, S_=S,
             gm=gmean, gc=gcov):
        ap = _capi.McAcqParamsC(kind, fat_relu, fat_max, reserved, 0.0, tau_relu, tau_max)
        p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
        return engine.lib.gpx_mc_acq_f64(engine.handle, ctypes.byref(ap), B, q_, S_, p(mean), p(cov), p(z), p(value),
                                         p(gm), p(gc), p(info), p(ws), ws.numel())

    bad = [dict(reserved=1), dict(q_=0), dict(q_=_capi.GPX_MAX_Q + 1), dict(kind=_capi.MCACQ_QPSD, S_=1), dict(gm=None),
           dict(gc=None), dict(kind=2), dict(fat_max=2), dict(fat_relu=-1), dict(tau_max=0.0), dict(tau_relu=-1.0)]
    for kw in bad:
        assert call(**kw) == _capi.GPX_INVALID_ARG, kw
    torch.cuda.synchronize()
    assert bool((value == 7.0).all()) and bool((gmean == 7.0).all()) and bool((gcov == 7.0).all())
    assert bool((info == 7).all())
    assert call() == _capi.GPX_OK  # the same buffers with valid arguments
    torch.cuda.synchronize()
    assert bool((info == 0).all()) and bool(torch.isfinite(value).all())


@pytest.fixture(scope="module")
def gp_model(engine):
    from tests.test_acqf import _model

    return _model()


@pytest.mark.parametrize("q", [1, 3])
def test_fused_qlogei_equals_unfused(engine, gp_model, q):
    gp, X, Y, op = gp_model
    best_f = float(Y.max())
    B = 6
    Xq = torch.tensor(np.random.default_rng(q).random((B, q, 4)), device=DEV)
    out = {}
    for fused in (False, True):
        a = acqf.qLogExpectedImprovement(gp, best_f=best_f, sampler=acqf.SobolQMCNormalSampler(torch.Size([256]), 11),
                                         fused=fused)
        Xg = Xq.clone().requires_grad_(True)
        v = a(Xg)
        (g,) = torch.autograd.grad(v.sum(), Xg)
        out[fused] = (v.detach().cpu(), g.cpu())
    dv = float((out[True][0] - out[False][0]).abs().max())
    dg = _grad_dev(out[True][1], out[False][1])
    print(f"fused vs unfused qLogEI q={q}: value dev {dv:.2e} gradient dev {dg:.2e}")
    np.testing.assert_allclose(out[True][0].numpy(), out[False][0].numpy(), rtol=TOL, atol=TOL)
    assert dg <= TOL


@pytest.mark.parametrize("which", ["qlogei_fat_max", "qpsd"])
def test_optimize_acqf_on_the_fused_acquisitions(engine, which):
    from tests.test_acqf import _model

    gp, X, Y, op = _model(n=300, d=3)
    if which == "qpsd":
        a, q, nonneg = acqf.qPosteriorStandardDeviation(gp, acqf.SobolQMCNormalSampler(torch.Size([128]), 4)), 2, True
    else:
        a = acqf.qLogExpectedImprovement(gp, best_f=float(Y.max()), fat_max=True,
                                         sampler=acqf.SobolQMCNormalSampler(torch.Size([128]), 4))
        q, nonneg = 3, False
    bounds = torch.tensor([[0.0] * 3, [1.0] * 3], dtype=torch.float64)
    X0 = acqf.gen_batch_initial_conditions(a, bounds.to(DEV), q, 4, 128, seed=5, nonnegative=nonneg)
    with torch.no_grad():
        v0s = a(X0)
    options = {"batch_limit": 2, "maxiter": 50, "nonnegative": nonneg}
    Xall, vall = acqf.optimize_acqf(a, bounds, q=q, num_restarts=4, raw_samples=128, options=options, seed=5,
                                    return_best_only=False)
    assert Xall.shape == (4, q, 3)
    assert bool((vall >= v0s - 1e-9).all()), (vall, v0s)
    assert float(Xall.min()) >= 0.0 and float(Xall.max()) <= 1.0
    if which == "qpsd":
        assert bool((vall > 0).all())


def test_dropin_acquires_with_qpsd(engine, tmp_path):
    cfg = GPConfig(num_restarts=2, acqf_raw_samples=32, fit_hyperparameters=False)
    opt = BayesianOptimizer(StubSimulator(), BOUNDS, str(tmp_path), n_initial_points=64, n_batches=1, batch_size=4,
                            num_outputs=2, target_total=68, engine=engine, gp_config=cfg, acquisition="qpsd", seed=0)
    opt._initial_design()
    opt.fit_gp_model()
    pts = opt.acquire(4)
    assert pts.shape == (4, 5)
    assert float(pts.min()) >= 0.0 and float(pts.max()) <= 1.0
    assert len({tuple(p.tolist()) for p in pts.cpu()}) == 4
