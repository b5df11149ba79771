"""CPU tests of the fused MC q-batch acquisition's host side: the fatmax limits (reference and acqf helper), the qPSD
closed form, initialize_q_batch_nonneg, the drop-in's argument check and the C ABI of gpx_mc_acq_f64."""
import ctypes
import math

import pytest
import torch

from bayesianoptimizer_amd import _capi, acqf
from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
from tests import mc_acq_ref as R
from tests.oracle_engine import OracleEngine
from tests.stubs import BOUNDS, StubSimulator


def _fatmax_impls():
    return [("reference", lambda x, tau: R.fatmax(x, tau)), ("acqf", lambda x, tau: acqf.fatmax(x, tau))]


@pytest.mark.parametrize("name,fatmax", _fatmax_impls(), ids=["reference", "acqf"])
def test_fatmax_limits(name, fatmax):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(7, 5, dtype=torch.float64, generator=g)
    # q = 1: the identity
    assert torch.equal(fatmax(x[:, :1], 1e-2), x[:, 0])
    # tau -> 0: the maximum (each other entry adds (alpha tau / gap)^alpha to the sum)
    gap = (x.amax(dim=-1, keepdim=True) - x)
    gap = torch.where(gap > 0, gap, torch.full_like(gap, float("inf"))).amin()
    tau = 1e-7
    bound = tau * 4 * (2.0 * tau / float(gap)) ** 2
    assert float((fatmax(x, tau) - x.amax(dim=-1)).abs().max()) <= bound + 1e-15
    # all entries equal: x + tau log q
    c = torch.full((3, 4), 0.7, dtype=torch.float64)
    torch.testing.assert_close(fatmax(c, 0.3), torch.full((3,), 0.7 + 0.3 * math.log(4), dtype=torch.float64),
                               rtol=1e-15, atol=1e-15)


@pytest.mark.parametrize("name,fatmax", _fatmax_impls(), ids=["reference", "acqf"])
def test_fatmax_tail_gradient(name, fatmax):
    """One entry far below the others: its gradient is t^-3 / sum_k t_k^-2, a power of the distance, where logsumexp's
    is exponentially small; the gradients sum to one."""
    tau = 1e-2
    x = torch.tensor([0.0, -0.01, -1.0], dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(fatmax(x.unsqueeze(0), tau).sum(), x)
    t = 1.0 + (0.0 - x.detach()) / (2.0 * tau)
    assert float(g[2]) == pytest.approx(float(t[2] ** -3 / (t ** -2).sum()), rel=1e-12)
    assert float(g.sum()) == pytest.approx(1.0, abs=1e-14)
    (gl,) = torch.autograd.grad(tau * torch.logsumexp(x / tau, dim=0), x)
    assert float(g[2]) > 1e-6 > 1e-30 > float(gl[2])


@pytest.mark.parametrize("S", [2, 64])
def test_qpsd_closed_form_equals_sample_std(S):
    mean, cov = R.synthetic_moments(4, 5, seed=S)
    z = R.base_samples(S, 5, seed=1)
    L = torch.linalg.cholesky(cov)
    f = mean.unsqueeze(0) + torch.einsum("bij,sj->sbi", L, z)
    per_sample = f.std(dim=0).sum(dim=-1)
    torch.testing.assert_close(R.qpsd_closed_form(L, z), per_sample, rtol=1e-12, atol=1e-12)
    value, gmean, _, info = R.mc_acq(mean, cov, z, "qpsd")
    torch.testing.assert_close(value, per_sample, rtol=1e-12, atol=1e-12)
    assert bool((info == 0).all()) and float(gmean.abs().max()) <= 1e-15


def _raw(N=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, 2, 3, dtype=torch.float64, generator=g), g


def test_initialize_q_batch_nonneg_keeps_the_best_point():
    X, g = _raw()
    for trial in range(20):
        Y = torch.rand(40, dtype=torch.float64, generator=g) * 1e-3
        Y[int(torch.randint(0, 40, (1,), generator=g))] = 1.0  # one point far above the rest
        out = acqf.initialize_q_batch_nonneg(X, Y, 4, generator=torch.Generator().manual_seed(trial))
        assert out.shape == (4, 2, 3)
        assert any(torch.equal(o, X[int(Y.argmax())]) for o in out)
        assert len({tuple(o.flatten().tolist()) for o in out}) == 4  # without replacement


def test_initialize_q_batch_nonneg_relative_threshold():
    # values below alpha * max never qualify while enough others do
    X, _ = _raw()
    Y = torch.full((40,), 1e-6, dtype=torch.float64)
    Y[:6] = torch.tensor([1.0, 0.9, 0.8, 0.7, 0.6, 0.5], dtype=torch.float64)
    for trial in range(10):
        out = acqf.initialize_q_batch_nonneg(X, Y, 4, generator=torch.Generator().manual_seed(trial))
        assert all(any(torch.equal(o, X[i]) for i in range(6)) for o in out)


def test_initialize_q_batch_nonneg_all_nonpositive_is_random():
    X, _ = _raw()
    Y = -torch.rand(40, dtype=torch.float64)
    a = acqf.initialize_q_batch_nonneg(X, Y, 5, generator=torch.Generator().manual_seed(1))
    b = acqf.initialize_q_batch_nonneg(X, Y, 5, generator=torch.Generator().manual_seed(2))
    assert a.shape == b.shape == (5, 2, 3)
    assert not torch.equal(a, b)
    assert torch.equal(acqf.initialize_q_batch_nonneg(X, torch.zeros(40, dtype=torch.float64), 40), X)  # n == N


def test_initialize_q_batch_nonneg_fills_up_when_few_are_positive():
    X, _ = _raw()
    Y = torch.zeros(40, dtype=torch.float64)
    Y[[3, 17]] = torch.tensor([0.5, 0.2], dtype=torch.float64)
    out = acqf.initialize_q_batch_nonneg(X, Y, 6, generator=torch.Generator().manual_seed(0))
    assert out.shape == (6, 2, 3)
    assert any(torch.equal(o, X[3]) for o in out) and any(torch.equal(o, X[17]) for o in out)
    with pytest.raises(ValueError):
        acqf.initialize_q_batch_nonneg(X, Y, 41)


def test_dropin_accepts_qpsd_and_fat_max(tmp_path):
    cfg = GPConfig(qlogei_fat_max=True)
    assert cfg.qlogei_fat_max is True and GPConfig().qlogei_fat_max is False
    for k, acq in enumerate(["qpsd", "qlogei"]):
        opt = BayesianOptimizer(StubSimulator(), BOUNDS, str(tmp_path / str(k)), n_initial_points=4, n_batches=1,
                                batch_size=2, target_total=6, engine=OracleEngine(), gp_config=cfg, acquisition=acq)
        assert opt.acquisition == acq
    with pytest.raises(ValueError, match="unknown acquisition"):
        BayesianOptimizer(StubSimulator(), BOUNDS, str(tmp_path / "x"), n_initial_points=4, n_batches=1, batch_size=2,
                          target_total=6, engine=OracleEngine(), acquisition="qstd")
    with pytest.raises(TypeError):
        GPConfig(qlogei_fatmax=True)


def test_mc_acq_abi():
    """The header declares the three entry points, the library exports them and the ctypes struct has the library's
    size."""
    syms = _capi.header_symbols()
    lib = _capi.load()
    for name in ("gpx_mc_acq_f64", "gpx_mc_acq_workspace_size", "gpx_mcacq_params_size"):
        assert name in syms and name in _capi._PROTOS and hasattr(lib, name)
    assert lib.gpx_mcacq_params_size() == ctypes.sizeof(_capi.McAcqParamsC) == 4 * 4 + 3 * 8
    assert _capi.McAcqParamsC.best_f.offset == 16
    hdr = open(_capi.HEADER_PATH).read()
    assert "GPX_MCACQ_QLOGEI = 0" in hdr and "GPX_MCACQ_QPSD = 1" in hdr
    assert (_capi.MCACQ_QLOGEI, _capi.MCACQ_QPSD) == (0, 1)
    b = ctypes.c_size_t()
    assert lib.gpx_mc_acq_workspace_size(5, 4, 512, ctypes.byref(b)) == _capi.GPX_OK
    assert b.value >= 5 * 512 * (2 * 4 + 1) * 8
    for B, q, S in [(1, 0, 8), (1, _capi.GPX_MAX_Q + 1, 8), (0, 1, 8), (_capi.GPX_MAX_GRAD_CANDIDATES, 2, 8), (1, 1, 0)]:
        assert lib.gpx_mc_acq_workspace_size(B, q, S, ctypes.byref(b)) == _capi.GPX_INVALID_ARG
    assert lib.gpx_mc_acq_workspace_size(1, 1, 8, None) == _capi.GPX_INVALID_ARG
