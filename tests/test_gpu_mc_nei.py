"""GPU tests of the noisy expected improvement path: gpx_mc_nei_f64 against the torch CPU reference
tests/mc_nei_ref.py on synthetic moments, gpx_joint_moments_f64 / gpx_cross_cov_grad_f64 against NumPy, and the acqf
classes, optimize_acqf and the drop-in built on them.

Tolerances: the project's MC ones (tests/test_gpu_mc_acq.py) — values rtol = atol = 1e-8, gradients norm-wise,
max|g - g_ref| <= 1e-8 max|g_ref| per q-batch — and the posterior one, 1e-9 of the largest entry, for the moments.  The
largest deviations seen on the device are recorded in DESIGN.md §4."""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import _capi, acqf
from bayesianoptimizer_amd.engine import KernelParams
from bayesianoptimizer_amd.models import ExactGP
from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
from bayesianoptimizer_amd.transforms import Standardize
from oracle import gp_oracle as O
from tests import mc_nei_ref as R
from tests.ard_util import ard_params
from tests.stubs import BOUNDS, StubSimulator
from tests.test_gpu_parity import DEV, pair, t

pytestmark = pytest.mark.gpu

TOL = 1e-8
SHAPES = [(1, 1, 3, 1), (2, 7, 64, 3), (5, 33, 257, 70), (32, 64, 257, 3)]  # (q, nb, S, B)
MODES = {"nei": dict(log=False), "fatplus_fatmax": dict(log=True, fat_relu=True, fat_max=True),
         "fatplus_lse": dict(log=True, fat_relu=True, fat_max=False),
         "softplus_fatmax": dict(log=True, fat_relu=False, fat_max=True),
         "softplus_lse": dict(log=True, fat_relu=False, fat_max=False)}
_inputs = {}


def inputs(q, nb, S, B):
    """(mean, cov, cross, Linv, zb, best, zq) of one shape, shared by the module and never modified"""
    key = (q, nb, S, B)
    if key not in _inputs:
        mu_b, cov_bb, mean, cov, cross = R.synthetic(B, q, nb)
        zb, zq = R.base_samples(S, nb, q)
        Linv, best = R.setup(mu_b, cov_bb, zb)
        _inputs[key] = (mean, cov, cross, Linv, zb, best, zq)
    return _inputs[key]


def _run(engine, args, mode, need_grad=True):
    out = engine.mc_nei(*(a.to(DEV) for a in args), need_grad=need_grad, **MODES[mode])
    return tuple(None if o is None else o.cpu() for o in out)


def _grad_dev(g, ref):
    """largest per-batch norm-wise deviation max|g - ref| / max|ref|"""
    B = ref.shape[0]
    num = (g - ref).abs().reshape(B, -1).amax(dim=1)
    den = ref.abs().reshape(B, -1).amax(dim=1)
    return float((num / den).max())


def _check(got, ref, what, batches=None):
    sel = slice(None) if batches is None else batches
    value, gmean, gcov, gcross, info = (x[sel] for x in got)
    rv, rgm, rgc, rgx, rinfo = (x[sel] for x in ref)
    dv = float(((value - rv).abs() / (1.0 + rv.abs())).max())
    dgm, dgc, dgx = _grad_dev(gmean, rgm), _grad_dev(gcov, rgc), _grad_dev(gcross, rgx)
    print(f"mc_nei {what}: value dev {dv:.2e} gmean dev {dgm:.2e} gcov dev {dgc:.2e} gcross dev {dgx:.2e}")
    assert torch.equal(info, rinfo)
    np.testing.assert_allclose(value.numpy(), rv.numpy(), rtol=TOL, atol=TOL)
    assert dgm <= TOL and dgc <= TOL and dgx <= TOL


@pytest.mark.parametrize("q,nb,S,B", SHAPES)
def test_value_and_gradients_match_reference(engine, q, nb, S, B):
    """q: no off-diagonal, the smallest factor, an odd size, the limit; nb: one point, odd, no multiple of a lane group,
    the limit; S: below a wave, a full wave, no multiple of the workgroup; B: one batch, a few, many."""
    args = inputs(q, nb, S, B)
    value, gap, imp, _ = R.preconditions(*args)
    # on the reference alone: the hard max and the ReLU kink are far from rounding
    assert bool((value > 0).all()) and gap >= 1e-9 and imp >= 1e-9, (value, gap, imp)
    for mode in MODES:
        _check(_run(engine, args, mode), R.mc_nei(*args, **MODES[mode]), f"{mode} q={q} nb={nb} S={S} B={B}")


def test_batch_without_improvement_is_exactly_zero(engine):
    """On this shape the generator's last batch has no improving sample (the others have 1 and 47 of 64)."""
    args = inputs(3, 64, 64, 3)
    value, gap, imp, frac = R.preconditions(*args)
    assert frac.tolist() == [1 / 64, 47 / 64, 0.0] and gap >= 1e-9 and imp >= 1e-9
    got, ref = _run(engine, args, "nei"), R.mc_nei(*args, log=False)
    assert float(got[0][2]) == 0.0 and float(ref[0][2]) == 0.0
    for g in got[1:4]:
        assert bool((g[2] == 0.0).all())
    _check(got, ref, "no improvement: the other batches", batches=[0, 1])
    _check(_run(engine, args, "fatplus_fatmax"), R.mc_nei(*args, **MODES["fatplus_fatmax"]), "no improvement, log")


def _with_neighbours(mid):
    """Three q-batches (q = 2, nb = 7); the middle one's conditional covariance D is ``mid`` to the bit: its
    cross-covariance is zero, so D = cov."""
    mean, cov, cross, Linv, zb, best, zq = inputs(2, 7, 64, 3)
    cov, cross = cov.clone(), cross.clone()
    cov[1] = torch.tensor(mid, dtype=torch.float64)
    cross[1] = 0.0
    return mean, cov, cross, Linv, zb, best, zq


@pytest.mark.parametrize("mode", ["nei", "fatplus_fatmax"])
def test_jitter_retry_is_per_batch(engine, mode):
    # second pivot 1 - (1 + 1e-9)^2 = -2e-9; with 1e-8 on the diagonal it is +1.8e-8
    args = _with_neighbours([[1.0, 1.0 + 1e-9], [1.0 + 1e-9, 1.0]])
    got, ref = _run(engine, args, mode), R.mc_nei(*args, **MODES[mode])
    assert got[4].tolist() == [0, 1, 0]
    _check(got, ref, f"{mode} jitter batch")


def test_not_positive_definite_batch_is_nan_and_raises(engine):
    args = _with_neighbours([[1.0, 2.0], [2.0, 1.0]])
    got, ref = _run(engine, args, "fatplus_fatmax"), R.mc_nei(*args, **MODES["fatplus_fatmax"])
    assert got[4].tolist() == ref[4].tolist() == [0, -1, 0]
    assert bool(got[0][1].isnan()) and all(bool(g[1].isnan().all()) for g in got[1:4])
    _check(got, ref, "not PD: the neighbours", batches=[0, 2])
    mean, cov, cross, Linv, zb, best, zq = (a.to(DEV) for a in args)
    with pytest.raises(torch.linalg.LinAlgError):
        acqf._McNei.apply(mean, cov, cross, engine, (Linv, zb, best, zq), MODES["fatplus_fatmax"])


@pytest.mark.parametrize("mode", ["nei", "fatplus_fatmax", "softplus_lse"])
def test_value_only_and_repeat_calls_are_bit_equal(engine, mode):
    args = inputs(5, 33, 257, 70)
    full = _run(engine, args, mode)
    again = _run(engine, args, mode)
    value_only = _run(engine, args, mode, need_grad=False)
    assert value_only[1] is None and value_only[2] is None and value_only[3] is None
    assert torch.equal(value_only[0], full[0]) and torch.equal(value_only[4], full[4])
    for x, y in zip(full, again):
        assert torch.equal(x, y)


def test_invalid_arguments_launch_nothing(engine):
    q, nb, S, B = 2, 7, 64, 3
    mean, cov, cross, Linv, zb, best, zq = (a.to(DEV).contiguous() for a in inputs(q, nb, S, B))
    full = lambda shape, dt=torch.float64: torch.full(shape, 7, dtype=dt, device=DEV)  # noqa: E731
    value, gmean, gcov, gcross, info = full((B,)), full((B, q)), full((B, q, q)), full((B, q, nb)), full((B,), torch.int32)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)

    def call(log=1, fat_relu=1, fat_max=1, reserved=0, tau_relu=1e-6, tau_max=1e-2, q_=q, nb_=nb, S_=S, B_=B, gm=gmean,
             gc=gcov, gx=gcross, best_=best):
        ap = _capi.McNeiParamsC(log, fat_relu, fat_max, reserved, tau_relu, tau_max)
        p = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None else 0)  # noqa: E731
        return engine.lib.gpx_mc_nei_f64(engine.handle, ctypes.byref(ap), B_, q_, nb_, S_, p(mean), p(cov), p(cross),
                                         p(Linv), p(zb), p(best_), p(zq), p(value), p(gm), p(gc), p(gx), p(info), p(ws),
                                         ws.numel())

    bad = [dict(reserved=1), dict(log=2), dict(log=-1), dict(fat_max=2), dict(fat_relu=-1), dict(tau_max=0.0),
           dict(tau_relu=-1.0), dict(q_=0), dict(q_=_capi.GPX_MAX_Q + 1), dict(nb_=0),
           dict(nb_=_capi.GPX_MAX_BASELINE + 1), dict(S_=0), dict(B_=0), dict(gm=None), dict(gc=None), dict(gx=None),
           dict(gm=None, gc=None), dict(best_=None)]
    for kw in bad:
        assert call(**kw) == _capi.GPX_INVALID_ARG, kw
    torch.cuda.synchronize()
    for out in (value, gmean, gcov, gcross, info):
        assert bool((out == 7).all())
    assert call() == _capi.GPX_OK  # the same buffers with valid arguments
    torch.cuda.synchronize()
    assert bool((info == 0).all()) and bool(torch.isfinite(value).all())


# ---- gpx_joint_moments_f64 / gpx_cross_cov_grad_f64 -------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "matern52", "scale_linear_matern52"])
@pytest.mark.parametrize("n,d,ard", [pytest.param(40, 3, False, id="40-3"), pytest.param(129, 8, False, id="129-8"),
                                     pytest.param(300, 16, False, id="300-16"), pytest.param(70, 4, True, id="70-4-ard"),
                                     pytest.param(129, 17, True, id="129-17-ard"),
                                     pytest.param(257, 32, True, id="257-32-ard")])
def test_joint_moments_and_cross_cov_match_numpy(engine, kind, n, d, ard):
    """n below one tile, just above two, several; d in each of the kernels' register-array sizes (4, 8, 16 and, in the
    ard cases, 32 at its narrowest and its widest d; with DMAX = 32 the value-only cross_value_kernel stages with 128 of
    its 256 threads); mb: one point, odd, just above one 64-tile, just above two; nb: one, odd, the limit; m: one, a few,
    many.  The ard cases take a different lengthscale and linear variance in every dimension (tests/ard_util.py)."""
    X, y = O.synthetic_problem(n, d, n + d)
    kw = dict(noise=1e-3, outputscale=1.4, const_mean=0.2)
    kp, op = ard_params(kind, d, d, **kw) if ard else pair(kind, d, **kw)
    st = engine.fit(t(X), t(y), kp)
    ost = O.fit(X, y, op)
    rng = np.random.default_rng(n)
    Xall = rng.random((130, d))
    worst = {"mean": 0.0, "cov": 0.0, "cross": 0.0, "dcross": 0.0, "fd": 0.0, "sub": 0.0}
    for mb in (1, 7, 65, 130):
        Xb = Xall[:mb]
        mean_b, cov_bb, Sb = engine.joint_moments(st, t(Xb))
        Ks = O.kernel_matrix(ost.X, Xb, op)
        S_ref = np.linalg.solve(ost.L.T, np.linalg.solve(ost.L, Ks))
        mean_r = op.const_mean + Ks.T @ ost.alpha.reshape(n)
        cov_r = O.kernel_matrix(Xb, Xb, op) - Ks.T @ S_ref
        worst["mean"] = max(worst["mean"], np.abs(mean_b.cpu().numpy() - mean_r).max() / np.abs(mean_r).max())
        worst["cov"] = max(worst["cov"], np.abs(cov_bb.cpu().numpy() - cov_r).max() / np.abs(cov_r).max())
        mean_only, cov_only, none = engine.joint_moments(st, t(Xb), want_solve=False)
        assert none is None and torch.equal(mean_only, mean_b) and torch.equal(cov_only, cov_bb)
    for nb in (1, 7, 64):
        Xb = Xall[:nb]
        mean_b, cov_bb, Sb = engine.joint_moments(st, t(Xb))
        cov_bb = cov_bb.cpu().numpy()
        S_ref = np.linalg.solve(ost.L.T, np.linalg.solve(ost.L, O.kernel_matrix(ost.X, Xb, op)))
        for m in (1, 5, 70):
            Xs = rng.random((m, d))
            cross, dcross = (v.cpu().numpy() for v in engine.cross_cov_grad(st, Sb, t(Xb), t(Xs)))

            def ref_cross(Z):
                return O.kernel_matrix(Z, Xb, op) - O.kernel_matrix(Z, ost.X, op) @ S_ref

            cross_r = ref_cross(Xs)
            dcross_r = (O.kernel_grad_first(Xs, Xb, op).transpose(0, 2, 1)
                        - np.einsum("anj,nb->ajb", O.kernel_grad_first(Xs, ost.X, op), S_ref))
            worst["cross"] = max(worst["cross"], np.abs(cross - cross_r).max() / np.abs(cross_r).max())
            worst["dcross"] = max(worst["dcross"], np.abs(dcross - dcross_r).max() / np.abs(dcross_r).max())
            value_only, none = engine.cross_cov_grad(st, Sb, t(Xb), t(Xs), need_grad=False)
            assert none is None  # the value-only kernel is another instantiation: the same tolerance, not the same bits
            worst["cross"] = max(worst["cross"], np.abs(value_only.cpu().numpy() - cross_r).max() / np.abs(cross_r).max())
            if m == 5:  # central differences of the reference's cross in one coordinate at a time
                h = 1e-6
                fd = np.empty_like(dcross)
                for j in range(d):
                    E = np.zeros((m, d))
                    E[:, j] = h
                    fd[:, j, :] = (ref_cross(Xs + E) - ref_cross(Xs - E)) / (2 * h)
                worst["fd"] = max(worst["fd"], np.abs(dcross - fd).max() / np.abs(fd).max())
        # candidates that ARE baseline points: their cross-covariance is the matching rows of cov_bb
        rows = np.arange(nb)[:: max(1, nb // 5)]
        cross_sub = engine.cross_cov_grad(st, Sb, t(Xb), t(Xb[rows]), need_grad=False)[0].cpu().numpy()
        worst["sub"] = max(worst["sub"], np.abs(cross_sub - cov_bb[rows]).max() / np.abs(cov_bb).max())
    print(f"joint/cross {kind} n={n} d={d}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k in ("mean", "cov", "cross", "dcross", "sub"):
        assert worst[k] <= 1e-9, (k, worst[k])
    assert worst["fd"] <= 1e-6


def test_joint_and_cross_invalid_arguments(engine):
    X, y = O.synthetic_problem(40, 3, 1)
    kp, _ = pair("rbf", 3, noise=1e-3)
    st = engine.fit(t(X), t(y), kp)
    Xb = t(np.random.default_rng(0).random((_capi.GPX_MAX_BASELINE + 1, 3)))
    _, _, Sb = engine.joint_moments(st, Xb)
    with pytest.raises(_capi.GPXError):
        engine.cross_cov_grad(st, Sb, Xb, Xb[:3])  # nb above the limit
    with pytest.raises(ValueError):
        engine.joint_moments(st, t(np.zeros((4, 2))))  # wrong d


# ---- the acqf classes on a fitted model -----------------------------------------------------------------------
_models = {}


def models(independent, noise=1e-3):
    """(GPU model, oracle-engine model) on the same data and parameters: n = 300, d = 3, two outputs"""
    key = (independent, noise)
    if key not in _models:
        X, y = O.synthetic_problem(300, 3, 11)
        Y = np.stack([y, 0.5 * y + np.sin(4 * X).sum(1)], axis=1)
        kp = KernelParams("matern52", 0.5, noise=noise)
        params = [kp, kp.replace(lengthscale=0.4)] if independent else kp
        gpu = ExactGP(X, Y, params, outcome_transform=Standardize()).fit()
        cpu = ExactGP(X, Y, params, outcome_transform=Standardize(), engine=R.NeiOracleEngine()).fit()
        _models[key] = (gpu, cpu, torch.tensor(X))
    return _models[key]


def _around_the_best(gp, Xb, objective, B=4, q=3, scale=0.03):
    """q-batches scattered around the baseline point with the highest posterior mean, where samples improve"""
    with torch.no_grad():
        mu, _ = acqf.posterior_moments(gp, Xb.unsqueeze(1), acqf._Objective(gp, objective.weights))
    rng = np.random.default_rng(10)
    return (Xb[int(mu[:, 0].argmax())] + torch.tensor(scale * rng.standard_normal((B, q, 3)))).clamp(0.0, 1.0)


@pytest.mark.parametrize("independent", [False, True], ids=["shared", "independent"])
@pytest.mark.parametrize("cls", ["qnei", "qlognei"])
def test_acqf_classes_match_the_oracle_path(engine, cls, independent):
    gpu, cpu, X = models(independent)
    objective = acqf.LinearMCObjective([0.6, 0.4])
    Xb = acqf.prune_inferior_points(cpu, X, objective, num_samples=256, seed=2)
    assert Xb.shape[0] >= 2
    kept_gpu = acqf.prune_inferior_points(gpu, X.to(DEV), objective, num_samples=256, seed=2)
    print(f"pruned baseline: {Xb.shape[0]} points on the oracle engine, {kept_gpu.shape[0]} on the device")
    Xq = _around_the_best(cpu, Xb, objective)
    out = {}
    for name, gp, dev in (("gpu", gpu, DEV), ("cpu", cpu, torch.device("cpu"))):
        sampler = acqf.SobolQMCNormalSampler(torch.Size([128]), 9)
        kw = dict(sampler=sampler, objective=objective, prune_baseline=False)
        a = (acqf.qNoisyExpectedImprovement(gp, Xb, **kw) if cls == "qnei"
             else acqf.qLogNoisyExpectedImprovement(gp, Xb, **kw))
        Xg = Xq.to(dev).clone().requires_grad_(True)
        v = a(Xg)
        (g,) = torch.autograd.grad(v.sum(), Xg)
        with torch.no_grad():  # value-only scoring
            np.testing.assert_allclose(a(Xg.detach()).cpu().numpy(), v.detach().cpu().numpy(), rtol=TOL, atol=TOL)
        out[name] = (v.detach().cpu(), g.cpu())
    if cls == "qnei":
        assert bool((out["cpu"][0] > 0).all())  # on the oracle path alone: every batch improves in some sample
    dv = float((out["gpu"][0] - out["cpu"][0]).abs().max())
    dg = _grad_dev(out["gpu"][1], out["cpu"][1])
    print(f"{cls} {'independent' if independent else 'shared'}: value dev {dv:.2e} gradient dev {dg:.2e}")
    np.testing.assert_allclose(out["gpu"][0].numpy(), out["cpu"][0].numpy(), rtol=TOL, atol=TOL)
    assert dg <= TOL


class _FixedSampler:
    def __init__(self, z):
        self.z = z

    def base_samples(self, q, device):
        assert self.z.shape[1] == q
        return self.z.to(device)


# |qLogNEI - qLogEI| with one baseline point of tiny posterior variance, measured on the oracle engine (CPU)
SINGLE_POINT_GAP_CPU = 4.992e-5  # at a posterior variance of 9.995e-7 (noise 1e-6)


def single_point_gap(gp, X, dev):
    """max |qLogNEI(X_baseline = one training point) - qLogEI(best_f = mu_b, fused, fat_max)| over a few q-batches, the
    two on the same q-batch base samples, and the baseline point's posterior variance"""
    xb = X[:1].to(dev)
    sampler = acqf.SobolQMCNormalSampler(torch.Size([128]), 3)
    nei = acqf.qLogNoisyExpectedImprovement(gp, xb, sampler=sampler, prune_baseline=False)
    Xq = torch.tensor(np.random.default_rng(5).random((6, 2, 3)), device=dev)
    with torch.no_grad():
        v_nei = nei(Xq)
        mu_b, Lb, _, _ = nei._baseline
        zq = nei._setups[2][3]
        ei = acqf.qLogExpectedImprovement(gp, best_f=float(mu_b[0]), sampler=_FixedSampler(zq), fused=True, fat_max=True)
        v_ei = ei(Xq)
    return float((v_nei - v_ei).abs().max()), float(Lb[0, 0]) ** 2


def test_single_point_baseline_approaches_qlogei(engine):
    gpu, cpu, X = models(False, noise=1e-6)
    gap_cpu, var_cpu = single_point_gap(cpu, X, torch.device("cpu"))
    gap_gpu, var_gpu = single_point_gap(gpu, X, DEV)
    print(f"single-point baseline: posterior variance {var_gpu:.2e}; |qLogNEI - qLogEI| {gap_gpu:.3e} on the device, "
          f"{gap_cpu:.3e} on the oracle engine")
    assert gap_cpu == pytest.approx(SINGLE_POINT_GAP_CPU, rel=1e-3)
    assert gap_gpu <= 10 * SINGLE_POINT_GAP_CPU


# ---- optimize_acqf and the drop-in ----------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["qnei", "qlognei"])
def test_optimize_acqf_on_the_noisy_acquisitions(engine, cls):
    gpu, _, X = models(False)
    sampler = acqf.SobolQMCNormalSampler(torch.Size([128]), 4)
    a = (acqf.qNoisyExpectedImprovement(gpu, X, sampler=sampler) if cls == "qnei"
         else acqf.qLogNoisyExpectedImprovement(gpu, X, sampler=sampler))
    q, nonneg = 3, cls == "qnei"
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
    if cls == "qnei":
        assert bool((vall >= 0).all())


def test_dropin_acquires_with_qnei(engine, tmp_path):
    cfg = GPConfig(num_restarts=2, acqf_raw_samples=32, fit_hyperparameters=False)
    opt = BayesianOptimizer(StubSimulator(), BOUNDS, str(tmp_path), n_initial_points=64, n_batches=1, batch_size=4,
                            num_outputs=2, target_total=68, engine=engine, gp_config=cfg, acquisition="qnei", seed=0)
    opt._initial_design()
    opt.fit_gp_model()
    pts = opt.acquire(4)
    assert pts.shape == (4, 5)
    assert float(pts.min()) >= 0.0 and float(pts.max()) <= 1.0
    assert len({tuple(p.tolist()) for p in pts.cpu()}) == 4
