"""Gradient of the collapsed SVGP bound with respect to the inducing locations on the GPU (gpx_svgp_bound_grad_z_f64,
GPEngine.svgp_bound_grad_z, svgp_bound_value_grad(inducing_grad=True), mll.fit_hyperparameters_sparse(learn_inducing=True),
SVGPModel.fit(learn_inducing_locations=True), GPConfig.sparse_inducing = "learned") against the torch-autograd reference
(a) of tests/sgpr_zgrad_ref.py.

Tolerance: every entry of dZ within TAUZ of the sum of the absolute values of its summands (sgpr_zgrad_ref.TAUZ =
32 TAUZ0, TAUZ0 the measured disagreement of the two CPU references; tests/test_svgp_zgrad_host.py)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import NotPositiveDefiniteError, _capi
from bayesianoptimizer_amd.engine import KernelParamsC
from tests import sgpr_grad_ref as G
from tests import sgpr_ref as R
from tests import sgpr_zgrad_ref as ZR

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def dev(engine, a):
    return torch.tensor(np.asarray(a), device=engine.device)


def check_dz(got, ref, scale, what):
    """The suite's check of one task's dZ, the ratio printed before it is asserted."""
    r = ZR.ratio(got, ref, scale)
    print(f"{what}: max |d dZ| / scale = {r:.3e} (TAUZ = {ZR.TAUZ:.2e})")
    assert got.shape == ref.shape and r <= ZR.TAUZ, what


def raw_grad_z(engine, kps, Z, X, Y, jitter, chunk=0, ws_bytes=None, dZ="new", lddz=None, stride_dz=None):
    """The C call itself (no exception on info): (status, out, dZ, info)."""
    T, M, d = Z.shape
    n = X.shape[0]
    pcs = (KernelParamsC * T)(*[p.to_c(d) for p in kps])
    out = torch.full((T, _capi.SVGP_GRAD_NOUT), float("nan"), dtype=torch.float64, device=engine.device)
    info = torch.full((T,), -7, dtype=torch.int32, device=engine.device)
    if isinstance(dZ, str):
        dZ = torch.full((T, M, d), float("nan"), dtype=torch.float64, device=engine.device)
    lddz = d if lddz is None else lddz
    stride_dz = M * lddz if stride_dz is None else stride_dz
    nb = ctypes.c_size_t()
    assert engine.lib.gpx_svgp_bound_grad_z_workspace_size(M, n, T, chunk, ctypes.byref(nb)) == _capi.GPX_OK
    ws = torch.empty(nb.value, dtype=torch.uint8, device=engine.device)
    p = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
    engine._bind_stream()
    st = engine.lib.gpx_svgp_bound_grad_z_f64(engine.handle, pcs, T, M, float(jitter), p(Z), Z.stride(1), Z.stride(0),
                                              p(X), n, X.stride(0), p(Y), Y.stride(0), p(out), p(dZ), lddz, stride_dz,
                                              p(info), p(ws), nb.value if ws_bytes is None else ws_bytes)
    torch.cuda.synchronize()
    return st, out, dZ, info


# ---- 1: dZ against autograd ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,chunk", [(1, 128), (1, None), (2, None), (3, None), (16, None)]
                         + [(s, None) for s in G.DSHAPES] + [(117, 128), (132, 128)])
@pytest.mark.parametrize("kind", G.KINDS)
def test_dz_matches_autograd(engine, shape, chunk, kind):
    """Shape 1 (M = 130): two row tiles, the second of 2 rows; with chunk 128 five column blocks over five chunks, the
    last of 8 columns.  Shape 2 (M = 200, T = 3): per-task parameters.  Shape 16 (d = 12): the DMAX = 16 kernels.
    sgpr_grad_ref.DSHAPES (d = 4, 9, 16, 17, 32): each instance at its widest and its narrowest d; the DMAX = 32 ones
    (117, 132) also with chunk 128: n = 300 in three chunks, the last of 44 columns."""
    pb, kps, refs = ZR.reference(shape, kind)
    out, dZ, info = engine.svgp_bound_grad_z(kps, dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y),
                                             jitter=R.JITTER, chunk=chunk)
    assert int(info.abs().sum()) == 0 and dZ.shape == pb.Z.shape
    got = dZ.cpu().numpy()
    for t, (a, scale) in enumerate(refs):
        check_dz(got[t], a, scale, f"shape {shape} chunk {chunk} {kind} task {t}")


# ---- 2: out is the hyperparameter gradient call's, bit for bit ------------------------------------------------------
@pytest.mark.parametrize("shape,chunk", [pytest.param(2, 128, id="128"), pytest.param(2, None, id="None"),
                                         pytest.param(132, 128, id="132-128"), pytest.param(132, None, id="132-None")])
def test_out_bits_equal_the_hyperparameter_gradient_call(engine, chunk, shape):
    """Shape 132 (d = 32): the ZG instance keeps the other instance's sums bit for bit at DMAX = 32 too."""
    pb = G.problem(shape)
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    base, ib = engine.svgp_bound_grad(pb.kps, Z, X, Y, chunk=chunk)
    out, dZ, info = engine.svgp_bound_grad_z(pb.kps, Z, X, Y, chunk=chunk)
    assert int(info.abs().sum()) == 0 and torch.equal(info, ib)
    assert torch.equal(out, base)
    assert bool(torch.isfinite(dZ).all())


# ---- 3: determinism and chunk widths --------------------------------------------------------------------------------
def test_calls_are_bit_identical_and_chunk_widths_agree(engine):
    pb, kps, refs = ZR.reference(1, "scale_linear_matern52")
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    got = {}
    for chunk in (128, 256):
        _, a, _ = engine.svgp_bound_grad_z(kps, Z, X, Y, chunk=chunk)
        _, b, _ = engine.svgp_bound_grad_z(kps, Z, X, Y, chunk=chunk)
        assert torch.equal(a, b), f"chunk {chunk}: two calls differ"
        got[chunk] = a.cpu().numpy()
    for t, (a, scale) in enumerate(refs):
        check_dz(got[256][t], a, scale, f"chunk 256 task {t}")
        check_dz(got[128][t], got[256][t], scale, f"chunk 128 against chunk 256, task {t}")


# ---- 4: every task its own Z ----------------------------------------------------------------------------------------
def test_per_task_inducing_points(engine):
    pb = G.problem(2)
    kind = "scale_linear_matern52"
    kps = [G.with_kind(p, kind) for p in pb.kps]
    T = len(kps)
    noise = np.random.default_rng(11).standard_normal(pb.Z.shape[1:])
    Z = np.stack([pb.Z[t] + 0.01 * t * noise for t in range(T)])
    assert not np.array_equal(Z[1], Z[2]) and not np.array_equal(Z[0], Z[1])
    _, dZ, info = engine.svgp_bound_grad_z(kps, dev(engine, Z), dev(engine, pb.X), dev(engine, pb.Y), jitter=R.JITTER)
    assert int(info.abs().sum()) == 0
    got = dZ.cpu().numpy()
    for t in range(T):
        a = ZR.autograd_dz(Z[t], pb.X, pb.Y[:, t], kps[t])
        scale = ZR.formula_dz(Z[t], pb.X, pb.Y[:, t], kps[t])[1]
        check_dz(got[t], a, scale, f"task {t} on its own Z")


# ---- 5: strided Z and dZ --------------------------------------------------------------------------------------------
def test_strided_arguments_give_the_same_bits(engine):
    pb = G.problem(2)
    T, M, d = pb.Z.shape
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    base_out, base, _ = engine.svgp_bound_grad_z(pb.kps, Z, X, Y)
    Zw = torch.full((T, M + 2, d + 5), float("nan"), dtype=torch.float64, device=engine.device)
    Zw[:, :M, :d] = Z
    Zs = Zw[:, :M, :d]
    lddz, rows = d + 3, M + 4
    dZw = torch.full((T, rows, lddz), SENTINEL, dtype=torch.float64, device=engine.device)
    st, out, _, info = raw_grad_z(engine, pb.kps, Zs, X, Y, R.JITTER, dZ=dZw, lddz=lddz, stride_dz=rows * lddz)
    assert st == _capi.GPX_OK and int(info.abs().sum()) == 0
    assert torch.equal(out, base_out)
    assert torch.equal(dZw[:, :M, :d], base)
    assert bool((dZw[:, :M, d:] == SENTINEL).all()) and bool((dZw[:, M:, :] == SENTINEL).all())
    # a row or task stride too small for the array is refused
    st, _, _, _ = raw_grad_z(engine, pb.kps, Z, X, Y, R.JITTER, dZ=dZw, lddz=d - 1)
    assert st == _capi.GPX_INVALID_ARG
    st, _, _, _ = raw_grad_z(engine, pb.kps, Z, X, Y, R.JITTER, dZ=dZw, lddz=lddz, stride_dz=M * lddz - 1)
    assert st == _capi.GPX_INVALID_ARG


# ---- 6: a failed K_ZZ is reported, and the other tasks are computed ------------------------------------------------
def test_kzz_failure_is_reported_per_task(engine):
    """jitter = 0 and, in task 1 of 2, one inducing point repeated seven times (test_gpu_svgp_grad.py): K_ZZ of task 1
    is exactly singular; task 0 still meets test 1's check against the jitter = 0 reference."""
    pb = G.problem(3)
    kind = "scale_linear_matern52"
    kps = [G.with_kind(p, kind) for p in pb.kps]
    Z = pb.Z.copy()
    Z[1, 40:47] = Z[1, 39]
    Zd, X, Y = dev(engine, Z), dev(engine, pb.X), dev(engine, pb.Y)
    with pytest.raises(NotPositiveDefiniteError, match="task 1"):
        engine.svgp_bound_value_grad(kps, Zd, X, Y, jitter=0.0, inducing_grad=True)
    st, out, dZ, info = raw_grad_z(engine, kps, Zd, X, Y, 0.0)
    info = info.cpu().numpy()
    assert st == _capi.GPX_OK and info[0] == 0 and info[1] > 0
    a = ZR.autograd_dz(Z[0], pb.X, pb.Y[:, 0], kps[0], 0.0)
    scale = ZR.formula_dz(Z[0], pb.X, pb.Y[:, 0], kps[0], 0.0)[1]
    check_dz(dZ[0].cpu().numpy(), a, scale, "task 0 beside a failed task")


# ---- 7: the workspace and the arguments ------------------------------------------------------------------------------
def test_workspace_size_and_refusals(engine):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = json.load(open(os.path.join(root, "tests", "golden", "svgp_z_workspace_sizes.json")))
    for M, T, chunk, want in rows["gpx_svgp_bound_grad_z_workspace_size"]:
        nb = ctypes.c_size_t()
        assert engine.lib.gpx_svgp_bound_grad_z_workspace_size(M, 100_000, T, chunk, ctypes.byref(nb)) == _capi.GPX_OK
        assert nb.value == want, (M, T, chunk)
    pb = G.problem(3)
    T, M, d = pb.Z.shape
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    nb = ctypes.c_size_t()
    assert engine.lib.gpx_svgp_bound_grad_z_workspace_size(M, X.shape[0], T, 128, ctypes.byref(nb)) == _capi.GPX_OK
    st, _, _, _ = raw_grad_z(engine, pb.kps, Z, X, Y, R.JITTER, chunk=128, ws_bytes=nb.value - 1)
    assert st == _capi.GPX_INVALID_ARG
    st, out, dZ, info = raw_grad_z(engine, pb.kps, Z, X, Y, R.JITTER, chunk=128, ws_bytes=nb.value)
    assert st == _capi.GPX_OK and bool(torch.isfinite(out).all()) and bool(torch.isfinite(dZ).all())
    st, _, _, _ = raw_grad_z(engine, pb.kps, Z, X, Y, R.JITTER, chunk=128, dZ=None)
    assert st == _capi.GPX_INVALID_ARG
    # the engine passes the size it asked for: a narrow call after a wide one still runs narrow
    engine.svgp_bound_grad_z(pb.kps, Z, X, Y)
    _, narrow, _ = engine.svgp_bound_grad_z(pb.kps, Z, X, Y, chunk=128)
    assert torch.equal(narrow, dZ)


# ---- 8: the value / gradient dicts ----------------------------------------------------------------------------------
def test_value_grad_carries_inducing_only_when_asked(engine):
    pb, kps, refs = ZR.reference(3, "matern52")
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    plain = engine.svgp_bound_value_grad(kps, Z, X, Y, jitter=R.JITTER)
    with_z = engine.svgp_bound_value_grad(kps, Z, X, Y, jitter=R.JITTER, inducing_grad=True)
    for t, (g, gz) in enumerate(zip(plain, with_z)):
        assert "inducing" not in g and sorted(gz) == sorted(list(g) + ["inducing"])
        assert g["nll"] == gz["nll"] and np.array_equal(g["lengthscale"], gz["lengthscale"])
        check_dz(gz["inducing"], refs[t][0], refs[t][1], f"dict of task {t}")


# ---- 9: end to end ---------------------------------------------------------------------------------------------------
def test_fit_with_learned_inducing_locations(engine):
    from bayesianoptimizer_amd.svgp import SVGPModel, SVGPPredictor

    pb = G.problem(1)
    X, Y, Z = dev(engine, pb.X), dev(engine, pb.Y), dev(engine, pb.Z)
    opts = {"maxiter": 15}
    fixed = SVGPModel.fit(X, Y, Z, pb.kps, options=opts, engine=engine)
    learned = SVGPModel.fit(X, Y, Z, pb.kps, options=opts, engine=engine, learn_inducing_locations=True)
    F_fixed, F_learned = float(fixed.bound[:, 0].sum()), float(learned.bound[:, 0].sum())
    moved = float((learned.Z - Z).abs().max())
    print(f"F: fixed Z {F_fixed:.6f}, learned Z {F_learned:.6f}; max |Z - Z0| = {moved:.3e}; "
          f"{learned.hyper_result.n_evals} evaluations")
    assert fixed.hyper_result.Z is None and torch.equal(fixed.Z, Z)
    assert learned.hyper_result.Z.shape == pb.Z.shape and learned.Z.shape == Z.shape
    assert F_learned >= F_fixed
    assert moved > 0.0
    mean, var = SVGPPredictor(learned, engine=engine).predict(X[:64], transformed=True)
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(var).all()) and bool((var > 0).all())


def test_dropin_learned_inducing_points(tmp_path, engine):
    from bayesianoptimizer_amd.models import SparseGP
    from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
    from tests.stubs import BOUNDS, StubSimulator

    cfg = GPConfig(large_n_policy=True, large_n_model="sparse", fit_hyperparameters=True, prior_set="none",
                   mll_options={"maxiter": 20}, sparse_hyperparameters="bound", sparse_inducing="learned",
                   max_inducing_points=16, candidates_pool_size=512, acq_batch_size=8)
    sim = StubSimulator()
    opt = BayesianOptimizer(sim, BOUNDS, str(tmp_path / "learned"), n_initial_points=40, n_batches=2, batch_size=8,
                            svgp_threshold=30, target_total=56, engine=engine, gp_config=cfg, seed=4,
                            acquisition="variance")
    best_params, best_value = opt.optimize()  # fit -> predict -> pool scan, twice
    assert best_params.shape == (5,) and np.isfinite(best_value)
    opt.fit_gp_model()
    sim.cleanup()
    gp = opt.gp_model
    assert isinstance(gp, SparseGP) and gp.train_X.shape[0] == 56 and gp.svgp.Z.shape == (8, 16, 5)
    res = opt.sparse_hyper_result
    assert res is not None and np.isfinite(res.loss) and res.Z.shape == (8, 16, 5)
    assert np.array_equal(gp.svgp.Z.cpu().numpy(), res.Z)
    assert not np.array_equal(res.Z[0], res.Z[1])  # every output moved its own copy
    y, v = opt.predict(np.array([[0.5, 100.0, 200.0, 4.0, 5.0]]), return_var=True)
    assert np.all(np.isfinite(y)) and np.all(v > 0)
