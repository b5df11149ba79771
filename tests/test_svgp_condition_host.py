"""Host checks of the sparse model's conditioning (gpx_svgp_condition_f64): the NumPy restatement of
tests/svgp_condition_ref.py against a refit on all points and against the dense information-form update, the drop-in's
"qlogei" mode above GPX_MAX_Q points on the sparse model with the stand-in engine, and the C ABI's new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import _capi
from tests import sgpr_ref as R
from tests import svgp_acquire_ref as AR
from tests import svgp_condition_ref as CR

TOL = 1e-11  # of max(1, max|.|): 30 x the 3.3e-13 the restatement was measured at
# the rows each conditioning step ends at, counted back from n
SPLITS = {"k40": (40, 0), "k150": (150, 0), "two_steps": (200, 70, 0), "three_single": (3, 2, 1, 0)}


def close(a, b):
    return np.abs(a - b).max() <= TOL * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("split", sorted(SPLITS))
@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_restatement_equals_the_refit_on_all_points(shape, split):
    pb = R.problem(shape)
    n, M, d, T, s, _ = R.SHAPES[shape]
    Xs = s * np.random.default_rng(50 + shape).standard_normal((512, d))
    cuts = [n - back for back in SPLITS[split]]
    vmean, vchol = [], []
    for t in range(T):
        fit = R.fit_collapsed_task(pb.Z[t], pb.X[:cuts[0]], pb.Y[:cuts[0], t], pb.ops[t])
        m, C = fit["m"], fit["C"]
        for a, b in zip(cuts[:-1], cuts[1:]):
            res = CR.condition_task(pb.Z[t], m, C, pb.ops[t], pb.X[a:b], pb.Y[a:b, t])
            m, C = res["m"], res["C"]
        assert np.all(np.triu(C, 1) == 0.0) and np.all(np.diag(C) > 0.0)
        vmean.append(m)
        vchol.append(C)
    ref_m, ref_C, _ = R.fit_collapsed(pb)
    mean, var = AR.latent_moments(pb.Z, np.stack(vmean), np.stack(vchol), pb.ops, Xs)
    rmean, rvar = AR.latent_moments(pb.Z, ref_m, ref_C, pb.ops, Xs)
    print(f"shape {shape} {split}: mean {np.abs(mean - rmean).max() / max(1.0, np.abs(rmean).max()):.2e} "
          f"var {np.abs(var - rvar).max() / max(1.0, np.abs(rvar).max()):.2e}")
    assert close(mean, rmean) and close(var, rvar)


def arbitrary_state(shape, seed=0):
    """A state that is no collapsed optimum: vchol = 1.5 I plus a small strictly-lower part (S S^T <= I fails), and a
    random vmean.  (vmean T x M, vchol T x M x M)."""
    n, M, d, T, s, _ = R.SHAPES[shape]
    rng = np.random.default_rng(7000 + 10 * shape + seed)
    vmean = rng.standard_normal((T, M))
    vchol = np.tril(rng.standard_normal((T, M, M)) / np.sqrt(M), -1) + 1.5 * np.eye(M)
    return vmean, vchol


@pytest.mark.parametrize("shape", [1, 3])
def test_restatement_equals_the_dense_update_of_an_arbitrary_state(shape):
    pb = R.problem(shape)
    n, M, d, T, s, _ = R.SHAPES[shape]
    Xs = s * np.random.default_rng(60 + shape).standard_normal((512, d))
    vmean, vchol = arbitrary_state(shape)
    Xn, Yn = pb.X[:60], pb.Y[:60]
    m_new, C_new = CR.condition(pb.Z, vmean, vchol, pb.ops, Xn, Yn)
    dm, dC = [], []
    for t in range(T):
        md, Sd = CR.dense_update(pb.Z[t], vmean[t], vchol[t], pb.ops[t], Xn, Yn[:, t])
        dm.append(md)
        dC.append(np.linalg.cholesky(Sd))
    mean, var = AR.latent_moments(pb.Z, m_new, C_new, pb.ops, Xs)
    rmean, rvar = AR.latent_moments(pb.Z, np.stack(dm), np.stack(dC), pb.ops, Xs)
    print(f"shape {shape}: mean {np.abs(mean - rmean).max() / max(1.0, np.abs(rmean).max()):.2e} "
          f"var {np.abs(var - rvar).max() / max(1.0, np.abs(rvar).max()):.2e}")
    assert close(mean, rmean) and close(var, rvar)


# ---- the drop-in --------------------------------------------------------------------------------------------------
def test_dropin_round_of_40_points_conditions_the_sparse_model_once(tmp_path):
    from bayesianoptimizer_amd.models import SparseGP
    from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
    from tests.stubs import BOUNDS, StubSimulator

    cfg = GPConfig(large_n_policy=True, large_n_model="sparse", num_restarts=2, acqf_raw_samples=32,
                   sparse_condition=True)
    opt = BayesianOptimizer(StubSimulator(), BOUNDS, str(tmp_path / "qlogei"), n_initial_points=40, n_batches=1,
                            batch_size=40, svgp_threshold=30, target_total=80,
                            engine=CR.SvgpConditionOracleEngine(), gp_config=cfg, acquisition="qlogei", seed=4)
    opt._initial_design()
    opt.fit_gp_model()
    assert isinstance(opt.gp_model, SparseGP)
    batch = opt.acquire(40)
    assert batch.shape == (40, 5) and bool(torch.isfinite(batch).all())
    assert float(batch.min()) >= 0.0 and float(batch.max()) <= 1.0
    assert opt.engine.calls["svgp_condition"] == [32], "one conditioning, on the first chunk of GPX_MAX_Q points"
    assert opt.gp_model.train_X.shape[0] == 40, "the round's own model is left as it was"


# ---- the C ABI --------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("gpx_svgp_condition_workspace_size", "gpx_svgp_condition_f64")


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
