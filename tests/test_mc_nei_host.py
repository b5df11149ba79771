"""CPU tests of the noisy expected improvement path's host side: the conditional form of the reference against the
whole-joint Cholesky, the C ABI of the three new calls, prune_inferior_points, the drop-in's modes and the acqf classes
on the oracle engine (tests/mc_nei_ref.py NeiOracleEngine)."""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import _capi, acqf
from bayesianoptimizer_amd.engine import KernelParams
from bayesianoptimizer_amd.models import ExactGP
from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
from bayesianoptimizer_amd.transforms import Standardize
from tests import mc_nei_ref as R
from tests.stubs import BOUNDS, StubSimulator

SHAPES = [(1, 1, 3, 1), (2, 7, 64, 3), (5, 33, 257, 70), (32, 64, 257, 3)]  # (q, nb, S, B)
LOG_MODES = [dict(log=False), dict(log=True, fat_relu=True, fat_max=True), dict(log=True, fat_relu=True, fat_max=False),
             dict(log=True, fat_relu=False, fat_max=True), dict(log=True, fat_relu=False, fat_max=False)]


@pytest.mark.parametrize("q,nb,S,B", SHAPES)
def test_conditional_form_equals_the_joint_cholesky(q, nb, S, B):
    mu_b, cov_bb, mean, cov, cross = R.synthetic(B, q, nb)
    zb, zq = R.base_samples(S, nb, q)
    Linv, best = R.setup(mu_b, cov_bb, zb)
    for mode in LOG_MODES:
        value, _, _, _, info = R.mc_nei(mean, cov, cross, Linv, zb, best, zq, **mode)
        joint = R.mc_nei_joint(mu_b, cov_bb, mean, cov, cross, zb, zq, **mode)
        assert bool((info == 0).all())
        assert float((value - joint).abs().max()) <= 1e-12, mode


def test_generator_keeps_the_kinks_away_from_rounding():
    """The generator's properties the GPU comparison relies on: every batch improves in 4-86 % of its samples, and neither
    the hard max (smallest gap 4.8e-5) nor the ReLU kink (smallest |improvement| 7.2e-5) sits near rounding."""
    gaps, imps, fracs = [], [], []
    for q, nb, S, B in SHAPES:
        mu_b, cov_bb, mean, cov, cross = R.synthetic(B, q, nb)
        zb, zq = R.base_samples(S, nb, q)
        Linv, best = R.setup(mu_b, cov_bb, zb)
        value, gap, imp, frac = R.preconditions(mean, cov, cross, Linv, zb, best, zq)
        assert bool((value > 0).all())
        gaps.append(gap)
        imps.append(imp)
        fracs += frac.tolist()
    assert min(gaps) >= 1e-9 and min(imps) >= 1e-9
    assert min(gaps) == pytest.approx(4.8e-5, rel=0.05) and min(imps) == pytest.approx(7.2e-5, rel=0.05)
    assert 0.03 <= min(fracs) and max(fracs) <= 0.87


def test_nei_abi():
    """The header declares the new entry points, the library exports them, the ctypes struct has the library's size and
    the workspace-size calls refuse what the calls refuse."""
    syms = _capi.header_symbols()
    lib = _capi.load()
    for name in ("gpx_joint_moments_workspace_size", "gpx_joint_moments_f64", "gpx_cross_cov_grad_workspace_size",
                 "gpx_cross_cov_grad_f64", "gpx_mcnei_params_size", "gpx_mc_nei_workspace_size", "gpx_mc_nei_f64"):
        assert name in syms and name in _capi._PROTOS and hasattr(lib, name)
    assert lib.gpx_mcnei_params_size() == ctypes.sizeof(_capi.McNeiParamsC) == 4 * 4 + 2 * 8
    assert _capi.McNeiParamsC.tau_relu.offset == 16
    hdr = open(_capi.HEADER_PATH).read()
    assert f"#define GPX_MAX_JOINT {_capi.GPX_MAX_JOINT} " in hdr and _capi.GPX_MAX_JOINT == 8192
    assert f"#define GPX_MAX_BASELINE {_capi.GPX_MAX_BASELINE} " in hdr and _capi.GPX_MAX_BASELINE == 64
    b = ctypes.c_size_t()
    assert lib.gpx_mc_nei_workspace_size(5, 4, 32, 512, ctypes.byref(b)) == _capi.GPX_OK
    assert b.value >= (5 * 512 * (2 * 4 + 1) + 5 * 4 * 32) * 8
    for B, q, nb, S in [(1, 0, 4, 8), (1, _capi.GPX_MAX_Q + 1, 4, 8), (0, 1, 4, 8), (1, 1, 0, 8),
                        (1, 1, _capi.GPX_MAX_BASELINE + 1, 8), (_capi.GPX_MAX_GRAD_CANDIDATES, 2, 4, 8), (1, 1, 4, 0)]:
        assert lib.gpx_mc_nei_workspace_size(B, q, nb, S, ctypes.byref(b)) == _capi.GPX_INVALID_ARG
    assert lib.gpx_mc_nei_workspace_size(1, 1, 1, 8, None) == _capi.GPX_INVALID_ARG
    assert lib.gpx_joint_moments_workspace_size(300, 130, ctypes.byref(b)) == _capi.GPX_OK and b.value > 0
    for n, mb in [(0, 4), (300, 0), (300, _capi.GPX_MAX_JOINT + 1)]:
        assert lib.gpx_joint_moments_workspace_size(n, mb, ctypes.byref(b)) == _capi.GPX_INVALID_ARG
    assert lib.gpx_joint_moments_workspace_size(300, 4, None) == _capi.GPX_INVALID_ARG
    assert lib.gpx_cross_cov_grad_workspace_size(300, 64, 70, ctypes.byref(b)) == _capi.GPX_OK
    for n, nb, m in [(0, 4, 4), (300, 0, 4), (300, _capi.GPX_MAX_BASELINE + 1, 4), (300, 4, 0),
                     (300, 4, _capi.GPX_MAX_GRAD_CANDIDATES + 1)]:
        assert lib.gpx_cross_cov_grad_workspace_size(n, nb, m, ctypes.byref(b)) == _capi.GPX_INVALID_ARG
    assert lib.gpx_cross_cov_grad_workspace_size(300, 4, 4, None) == _capi.GPX_INVALID_ARG


def test_prune_from_samples_cap_and_tie_rule():
    # argmax counts over 5 points: [3, 0, 2, 2, 1]
    rows = [0, 0, 0, 2, 2, 3, 3, 4]
    samples = torch.zeros(len(rows), 5, dtype=torch.float64)
    for s, i in enumerate(rows):
        samples[s, i] = 1.0
    assert acqf._prune_from_samples(samples, 64).tolist() == [0, 2, 3, 4]  # never the maximum: dropped
    assert acqf._prune_from_samples(samples, 4).tolist() == [0, 2, 3, 4]
    assert acqf._prune_from_samples(samples, 3).tolist() == [0, 2, 3]  # the lowest count goes first
    assert acqf._prune_from_samples(samples, 2).tolist() == [0, 2]  # counts tie at 2: the lower index stays
    assert acqf._prune_from_samples(samples, 1).tolist() == [0]
    # torch.argmax takes the first of equal entries: a row of equal values counts for index 0
    assert acqf._prune_from_samples(torch.zeros(3, 4, dtype=torch.float64), 64).tolist() == [0]


def _oracle_model(n=30, d=3, T=1, independent=False, seed=0, noise=1e-2):
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    Y = np.stack([np.sin((3 + t) * X).sum(1) + 0.05 * rng.standard_normal(n) for t in range(T)], 1)
    kp = KernelParams("matern52", 0.6, noise=noise)
    gp = ExactGP(torch.tensor(X), torch.tensor(Y), [kp] * T if independent else kp, engine=R.NeiOracleEngine(),
                 outcome_transform=Standardize()).fit()
    return gp, torch.tensor(X), Y


def test_prune_inferior_points_on_a_model():
    gp, X, Y = _oracle_model()
    kept = acqf.prune_inferior_points(gp, X, num_samples=512, seed=1)
    assert 1 <= kept.shape[0] < X.shape[0]
    rows = [int((X == k).all(dim=1).nonzero()[0]) for k in kept]
    assert rows == sorted(rows)  # ascending order of the rows of X
    assert int(np.argmax(Y[:, 0])) in rows  # the best observed point can be the incumbent
    again = acqf.prune_inferior_points(gp, X, num_samples=512, seed=1)
    assert torch.equal(kept, again)
    capped = acqf.prune_inferior_points(gp, X, num_samples=512, seed=1, max_points=2)
    assert capped.shape[0] == min(2, kept.shape[0])
    assert all(any(torch.equal(c, k) for k in kept) for c in capped)
    with pytest.raises(ValueError):
        acqf.prune_inferior_points(gp, X, max_points=0)


def test_baseline_limit_without_pruning():
    gp, X, _ = _oracle_model(n=70)
    with pytest.raises(ValueError, match="baseline"):
        acqf.qNoisyExpectedImprovement(gp, X, prune_baseline=False)
    a = acqf.qNoisyExpectedImprovement(gp, X)
    assert 1 <= a.X_baseline.shape[0] <= _capi.GPX_MAX_BASELINE


@pytest.mark.parametrize("independent", [False, True])
@pytest.mark.parametrize("cls", ["qnei", "qlognei"])
def test_acqf_gradient_matches_central_differences(cls, independent):
    T = 2
    gp, X, _ = _oracle_model(T=T, independent=independent)
    objective = acqf.LinearMCObjective([0.7, 0.3])
    sampler = acqf.SobolQMCNormalSampler(torch.Size([64]), 5)
    if cls == "qnei":
        a = acqf.qNoisyExpectedImprovement(gp, X, sampler=sampler, objective=objective)
    else:
        a = acqf.qLogNoisyExpectedImprovement(gp, X, sampler=sampler, objective=objective, tau_relu=1e-3)
    assert a.X_baseline.shape[0] >= 2
    # q-batches around baseline points, where some samples improve on the incumbent
    rng = np.random.default_rng(4)
    near = a.X_baseline[torch.arange(6) % a.X_baseline.shape[0]].reshape(2, 3, 3)
    Xq = (near + torch.tensor(0.1 * rng.standard_normal((2, 3, 3)))).clamp(0.0, 1.0).requires_grad_(True)
    v = a(Xq)
    assert v.shape == (2,) and bool(torch.isfinite(v).all())
    if cls == "qnei":
        assert bool((v > 0).all())
    (g,) = torch.autograd.grad(v.sum(), Xq)
    h = 1e-6
    fd = torch.zeros_like(g)
    with torch.no_grad():
        for idx in np.ndindex(*Xq.shape):
            Xp, Xm = Xq.detach().clone(), Xq.detach().clone()
            Xp[idx] += h
            Xm[idx] -= h
            fd[idx] = (a(Xp).sum() - a(Xm).sum()) / (2 * h)
    # central differences of a piecewise-smooth MC mean: O(h^2) truncation plus the few samples that change their
    # arg max or cross the ReLU kink within h
    assert float((g - fd).abs().max()) <= 1e-5 * max(1.0, float(fd.abs().max())), (g, fd)
    assert len(a._setups) == 1  # the per-q set-up is formed once


def test_dropin_accepts_qnei_and_qlognei(tmp_path):
    assert GPConfig().nei_baseline_pool == 1024
    for k, acq in enumerate(["qnei", "qlognei"]):
        opt = BayesianOptimizer(StubSimulator(), BOUNDS, str(tmp_path / str(k)), n_initial_points=4, n_batches=1,
                                batch_size=2, target_total=6, engine=R.NeiOracleEngine(), acquisition=acq)
        assert opt.acquisition == acq


def test_dropin_acquires_with_qnei_on_the_oracle_engine(tmp_path):
    cfg = GPConfig(num_restarts=2, acqf_raw_samples=16, fit_hyperparameters=False, mc_samples=32, maxiter=5,
                   nei_baseline_pool=8)
    opt = BayesianOptimizer(StubSimulator(), BOUNDS, str(tmp_path), n_initial_points=12, n_batches=1, batch_size=2,
                            num_outputs=2, target_total=14, engine=R.NeiOracleEngine(), gp_config=cfg,
                            acquisition="qnei", seed=0)
    opt._initial_design()
    opt.fit_gp_model()
    pts = opt.acquire(2)
    assert pts.shape == (2, 5)
    assert float(pts.min()) >= 0.0 and float(pts.max()) <= 1.0
