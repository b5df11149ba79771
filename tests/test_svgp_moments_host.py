"""Host checks of the SVGP q-batch moments (gpx_svgp_moments_grad_f64): the NumPy reference of
tests/svgp_moments_ref.py against autograd through an independent torch restatement and against the SVGP predictive, the
drop-in's "qpsd" / "qlogei" modes on the sparse model with the oracle engine, and the C ABI's new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import _capi
from tests import sgpr_ref as R
from tests import svgp_moments_ref as SR

CASES = [(50, 4, 4, 2), (129, 1, 1, 5), (200, 5, 3, 3), (140, 17, 2, 2)]


def states(M, d, q, B, kind):
    """The two models of the GPU tests: the closed-form fit and the arbitrary state."""
    kp, op, Z, X, y, Xs, vmean, vchol = SR.problem(M, d, q, B, kind)
    fit = R.fit_collapsed_task(Z, X, y, op, SR.JITTER)
    return op, Z, Xs, {"fit": (fit["m"], fit["C"]), "arbitrary": (vmean, vchol)}


@pytest.mark.parametrize("kind", SR.KINDS)
@pytest.mark.parametrize("M,d,q,B", CASES)
def test_reference_derivatives_equal_autograd_of_the_torch_restatement(M, d, q, B, kind):
    op, Z, Xs, models = states(M, d, q, B, kind)
    for name, (vm, vc) in models.items():
        mean, dmean, cov, dcov = SR.moments_grad(Z, vm, vc, op, Xs, q)
        X = torch.tensor(Xs.reshape(B, q, d), requires_grad=True)
        tm, tc = SR.torch_moments(Z, vm, vc, op, X)
        assert np.abs(tm.detach().numpy().reshape(-1) - mean).max() <= 1e-10 * np.abs(mean).max(), name
        assert np.abs(tc.detach().numpy().reshape(B * q, q) - cov).max() <= 1e-10 * np.abs(cov).max(), name
        jm = np.zeros_like(dmean)
        jc = np.zeros_like(dcov)
        for b in range(B):
            for i in range(q):
                (g,) = torch.autograd.grad(tm[b, i], X, retain_graph=True)
                jm[b * q + i] = g[b, i].numpy()
                for c in range(q):
                    (g,) = torch.autograd.grad(tc[b, i, c], X, retain_graph=True)
                    # x_a enters cov[a][c] through the first argument only, except on the diagonal (twice)
                    jc[b * q + i, :, c] = g[b, i].numpy() / (2.0 if c == i else 1.0)
        assert np.abs(jm - dmean).max() <= 1e-10 * np.abs(dmean).max(), name
        assert np.abs(jc - dcov).max() <= 1e-10 * np.abs(dcov).max(), name


@pytest.mark.parametrize("kind", SR.KINDS)
@pytest.mark.parametrize("M,d,q,B", CASES)
def test_reference_q1_equals_the_svgp_predictive(M, d, q, B, kind):
    """The q = 1 variance plus the noise, and the mean, are SVGPPredictor.predict on the oracle engine."""
    from bayesianoptimizer_amd.svgp import SVGPModel, SVGPPredictor

    kp = SR.problem(M, d, q, B, kind)[0]
    op, Z, Xs, models = states(M, d, q, B, kind)
    eng = SR.SvgpOracleEngine()
    for name, (vm, vc) in models.items():
        model = SVGPModel(Z=torch.tensor(Z[None]), vmean=torch.tensor(vm[None]), vchol=torch.tensor(vc[None]),
                          params=[kp], jitter=SR.JITTER)
        mu, var = SVGPPredictor(model, engine=eng).predict(torch.tensor(Xs), transformed=True)
        mean, _, cov, _ = SR.moments_grad(Z, vm, vc, op, Xs, 1)
        assert np.abs(mu.numpy()[:, 0] - mean).max() <= 1e-12 * np.abs(mean).max(), name
        keep = var.numpy()[:, 0] > 1e-10  # (the predictive's floor)
        assert keep.any()
        scale = np.abs(var.numpy()[:, 0]).max()
        assert np.abs(var.numpy()[:, 0] - (cov[:, 0] + op.noise))[keep].max() <= 1e-12 * scale, name


# ---- the drop-in --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acquisition", ["qpsd", "qlogei"])
def test_dropin_round_on_the_sparse_model(tmp_path, acquisition):
    opt = SR.dropin_optimizer(tmp_path, acquisition)
    SR.dropin_round(opt)
    calls = opt.engine.calls["svgp_moments_grad"]
    q = 1 if acquisition == "qpsd" else 8  # qpsd: one point for each of the 8 outputs
    assert (32 * q, q, False) in calls, "the raw samples are scored by the value-only call"
    assert any(c[2] for c in calls), "L-BFGS-B evaluates the gradient call"


def test_dropin_other_modes_still_raise_on_the_sparse_model(tmp_path):
    for acquisition in ("logei", "qnei"):
        with pytest.raises(ValueError, match="sparse"):
            SR.dropin_optimizer(tmp_path, acquisition)
    opt = SR.dropin_optimizer(tmp_path, "qlogei", batch_size=40)
    opt._initial_design()
    opt.fit_gp_model()
    with pytest.raises(ValueError, match="cannot be conditioned on a chunk"):
        opt.acquire(40)


# ---- the C ABI --------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("gpx_svgp_moments_grad_workspace_size", "gpx_svgp_moments_grad_f64")


def test_header_declares_and_library_exports_the_new_symbols():
    symbols = _capi.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in symbols and name in _capi._PROTOS, name
        assert re.search(r"gpx_status\s+" + name + r"\s*\(", open(_capi.HEADER_PATH).read()), name
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libgpx.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported, name
