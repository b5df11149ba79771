"""Closed-form SVGP variational posterior on the GPU (gpx_svgp_fit_collapsed_f64, GPEngine.svgp_fit_collapsed,
SVGPModel.fit_collapsed, the drop-in's sparse large-n model) against the NumPy restatement tests/sgpr_ref.py.

Tolerances are the project's (tests/test_svgp.py): what the model is used for, the predictive, at |d mu| <= 1e-9 max|mu|
and |d var| <= 1e-9 max var; the bound and each of its terms at 1e-9 of the sum of the terms' absolute values.  vmean /
vchol are not compared entrywise: two sound fp64 routes to them differ by a few 1e-9 (conditioning of B), while the
predictive they give agrees to 1e-13."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import NotPositiveDefiniteError, _capi
from bayesianoptimizer_amd.engine import KernelParamsC
from bayesianoptimizer_amd.svgp import SVGPModel, SVGPPredictor
from oracle import gp_oracle as O
from tests import sgpr_grad_ref as G
from tests import sgpr_ref as R

pytestmark = pytest.mark.gpu
RTOL = 1e-9
NQ = 500


@functools.lru_cache(maxsize=None)
def reference(shape, jitter=R.JITTER):
    """(problem, reference vmean / vchol / bound, query points, reference predictive), computed once per shape."""
    pb = G.problem(shape) if shape in G.DSHAPES else R.problem(shape)
    vmean, vchol, bound = R.fit_collapsed(pb, jitter)
    s = (G.DSHAPES[shape] if shape in G.DSHAPES else R.SHAPES[shape])[4]
    Xq = s * np.random.default_rng(77 + shape).standard_normal((NQ, pb.X.shape[1]))
    mu, var, _ = O.svgp_predict(pb.Z, vmean, vchol, pb.ops, Xq, jitter=jitter)
    for a in (vmean, vchol, bound, Xq, mu, var, pb.X, pb.Y, pb.Z):
        a.setflags(write=False)
    return pb, vmean, vchol, bound, Xq, mu, var


def dev(engine, a):
    return torch.tensor(np.asarray(a), device=engine.device)


def check_predictive(mu, var, mu_r, var_r, tasks=None, what=""):
    mu, var = np.asarray(mu), np.asarray(var)
    if tasks is not None:
        mu_r, var_r = mu_r[:, tasks], var_r[:, tasks]
    dmu = np.abs(mu - mu_r).max() / np.abs(mu_r).max()
    dvar = np.abs(var - var_r).max() / np.abs(var_r).max()
    print(f"{what} |dmu|/max|mu| = {dmu:.2e}  |dvar|/max var = {dvar:.2e}")
    assert dmu <= RTOL and dvar <= RTOL, what


def check_fit(engine, shape, vmean, vchol, jitter=R.JITTER, what=""):
    """Test 1's checks of a (vmean, vchol) pair of device tensors."""
    pb, _, _, _, Xq, mu_r, var_r = reference(shape, jitter)
    vm, vc = vmean.cpu().numpy(), vchol.cpu().numpy()
    T, M = vm.shape
    for t in range(T):
        assert np.all(np.triu(vc[t], 1) == 0.0), f"{what} task {t}: strict upper triangle of vchol"
        assert np.all(np.diag(vc[t]) > 0.0), f"{what} task {t}: diagonal of vchol"
    # the returned parameters through the oracle's predictive ...
    mu_o, var_o, _ = O.svgp_predict(pb.Z, vm, vc, pb.ops, Xq, jitter=jitter)
    check_predictive(mu_o, var_o, mu_r, var_r, what=f"{what} shape {shape} oracle predictive of the GPU (m, C):")
    # ... and through the engine's own
    model = SVGPModel(Z=dev(engine, pb.Z), vmean=vmean, vchol=vchol, params=pb.kps, jitter=jitter)
    mu_g, var_g = SVGPPredictor(model, engine).predict(dev(engine, Xq))
    check_predictive(mu_g.cpu().numpy(), var_g.cpu().numpy(), mu_r, var_r,
                     what=f"{what} shape {shape} GPU predictive of the GPU (m, C):")


def check_bound(bound, bound_r, what=""):
    bound = np.asarray(bound)
    for t in range(bound_r.shape[0]):
        scale = np.abs(bound_r[t, 1:]).sum()
        err = np.abs(bound[t] - bound_r[t]) / scale
        print(f"{what} task {t}: F = {bound[t, 0]:.6f} (ref {bound_r[t, 0]:.6f}), |d| / sum|terms| = "
              + " ".join(f"{e:.1e}" for e in err))
        assert np.all(err <= RTOL), (what, t)


def raw_fit(engine, kps, Z, X, Y, jitter, chunk=0):
    """The C call itself (no exception on info): (vmean, vchol, bound, info) device tensors."""
    T, M, d = Z.shape
    n = X.shape[0]
    pcs = (KernelParamsC * T)(*[p.to_c(d) for p in kps])
    f64 = dict(dtype=torch.float64, device=engine.device)
    vmean, vchol = torch.empty((T, M), **f64), torch.empty((T, M, M), **f64)
    bound = torch.empty((T, _capi.SVGP_BOUND_NOUT), **f64)
    info = torch.full((T,), -7, dtype=torch.int32, device=engine.device)
    nb = ctypes.c_size_t()
    assert engine.lib.gpx_svgp_fit_collapsed_workspace_size(M, n, T, chunk, ctypes.byref(nb)) == _capi.GPX_OK
    ws = torch.empty(nb.value, dtype=torch.uint8, device=engine.device)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    engine._bind_stream()
    st = engine.lib.gpx_svgp_fit_collapsed_f64(engine.handle, pcs, T, M, float(jitter), p(Z), d, M * d, p(X), n,
                                               X.stride(0), p(Y), Y.stride(0), p(vmean), M, p(vchol), M, M * M,
                                               p(bound), p(info), p(ws), nb.value)
    assert st == _capi.GPX_OK, engine.lib.gpx_last_error(engine.handle)
    torch.cuda.synchronize()
    return vmean, vchol, bound, info


# ---- 1 + 2: parity of the predictive and of the bound, every shape --------------------------------------------------
@pytest.mark.parametrize("shape", [1, 2, 3, 4] + list(G.DSHAPES))
def test_fit_collapsed_predictive_and_bound_match_reference(engine, shape):
    """sgpr_grad_ref.DSHAPES (d = 4, 9, 16, 17, 32) beside sgpr_ref's: the K_ZZ and chunk kernels and the predictive's
    K* build at the widest and the narrowest d of every DMAX instance."""
    pb, _, _, bound_r, Xq, mu_r, var_r = reference(shape)
    model = SVGPModel.fit_collapsed(dev(engine, pb.X), dev(engine, pb.Y), pb.kps, dev(engine, pb.Z), engine=engine)
    assert model.num_tasks == len(pb.kps) and model.bound.shape == (len(pb.kps), 6) and not model.bound.is_cuda
    mu, var = SVGPPredictor(model, engine).predict(dev(engine, Xq))
    check_predictive(mu.cpu().numpy(), var.cpu().numpy(), mu_r, var_r, what=f"shape {shape} model predictive:")
    check_fit(engine, shape, model.vmean, model.vchol)
    check_bound(model.bound.numpy(), bound_r, what=f"shape {shape}")


# ---- 3: chunking and determinism ----------------------------------------------------------------------------------
def test_chunk_widths_agree_and_calls_are_bit_identical(engine):
    pb, _, _, bound_r, *_ = reference(2)
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    narrow = engine.svgp_fit_collapsed(pb.kps, Z, X, Y, chunk=128)   # 700 points: six chunks, the last of 60
    wide = engine.svgp_fit_collapsed(pb.kps, Z, X, Y)                # the default: one chunk
    for name, out in (("chunk 128", narrow), ("default chunk", wide)):
        check_fit(engine, 2, out[0], out[1], what=name)
        check_bound(out[2].cpu().numpy(), bound_r, what=name)
    for chunk, first in ((128, narrow), (None, wide)):
        again = engine.svgp_fit_collapsed(pb.kps, Z, X, Y, chunk=chunk)
        for a, b in zip(first, again):
            assert torch.equal(a, b), f"chunk {chunk}: two calls differ"


def test_chunk_width_follows_the_workspace_size(engine):
    """Below the chunk = 128 size the call is refused; the engine passes the size it asked for, not its cached
    buffer's, so a narrow call after a wide one still runs narrow (bit-equal to a first narrow call)."""
    pb = reference(2)[0]
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    T, M, d = pb.Z.shape
    nb = ctypes.c_size_t()
    assert engine.lib.gpx_svgp_fit_collapsed_workspace_size(M, X.shape[0], T, 128, ctypes.byref(nb)) == _capi.GPX_OK
    pcs = (KernelParamsC * T)(*[p.to_c(d) for p in pb.kps])
    ws = torch.empty(nb.value, dtype=torch.uint8, device=engine.device)
    out = [torch.empty(s, dtype=torch.float64, device=engine.device) for s in ((T, M), (T, M, M), (T, 6))]
    info = torch.zeros(T, dtype=torch.int32, device=engine.device)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    st = engine.lib.gpx_svgp_fit_collapsed_f64(engine.handle, pcs, T, M, 1e-4, p(Z), d, M * d, p(X), X.shape[0], d, p(Y),
                                               T, p(out[0]), M, p(out[1]), M, M * M, p(out[2]), p(info), p(ws),
                                               nb.value - 4096)
    assert st == _capi.GPX_INVALID_ARG
    engine.svgp_fit_collapsed(pb.kps, Z, X, Y)  # grows the engine's cached workspace to the default width
    a = engine.svgp_fit_collapsed(pb.kps, Z, X, Y, chunk=128)
    b = raw_fit(engine, pb.kps, Z, X, Y, R.JITTER, chunk=128)
    for u, v in zip(a, b[:3]):
        assert torch.equal(u, v)


# ---- 4: strided arguments ------------------------------------------------------------------------------------------
def test_strided_arguments_give_the_same_bits(engine):
    pb = reference(2)[0]
    n, d = pb.X.shape
    T = pb.Y.shape[1]
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    base = engine.svgp_fit_collapsed(pb.kps, Z, X, Y)
    Xw = torch.full((n, d + 3), float("nan"), dtype=torch.float64, device=engine.device)
    Xw[:, :d] = X
    Yw = torch.full((n, T + 4), float("nan"), dtype=torch.float64, device=engine.device)
    Yw[:, 2:2 + T] = Y
    Xs, Ys = Xw[:, :d], Yw[:, 2:2 + T]
    assert Xs.stride(0) == d + 3 and Ys.stride(0) == T + 4 and not Xs.is_contiguous()
    strided = engine.svgp_fit_collapsed(pb.kps, Z, Xs, Ys)
    for a, b in zip(base, strided):
        assert torch.equal(a, b)
    # Z shared by the tasks (M x d) against the same points expanded to T x M x d
    shared = SVGPModel.fit_collapsed(Xs, Ys, pb.kps, Z[0], engine=engine)
    expanded = SVGPModel.fit_collapsed(X, Y, pb.kps, Z, engine=engine)
    assert shared.Z.shape == (T, Z.shape[1], d)
    for a, b in ((shared.vmean, expanded.vmean), (shared.vchol, expanded.vchol), (shared.bound, expanded.bound)):
        assert torch.equal(a, b)
    assert torch.equal(shared.vmean, base[0]) and torch.equal(shared.bound, base[2].cpu())


# ---- 5: a failed K_ZZ is reported, and the other tasks are computed ----------------------------------------------------
def test_kzz_failure_is_reported_per_task(engine):
    """jitter = 0 and, in task 1 of 2, one inducing point repeated: K_ZZ of task 1 is exactly singular.  (The row is
    repeated seven times: a single copy leaves a pivot of +-1 ulp, whose sign rounding decides; every further copy
    repeats that draw.)"""
    pb, *_ = reference(3, 0.0)
    Z = pb.Z.copy()
    Z[1, 40:47] = Z[1, 39]
    Zd, X, Y = dev(engine, Z), dev(engine, pb.X), dev(engine, pb.Y)
    with pytest.raises(NotPositiveDefiniteError, match="task 1"):
        engine.svgp_fit_collapsed(pb.kps, Zd, X, Y, jitter=0.0)
    vmean, vchol, bound, info = raw_fit(engine, pb.kps, Zd, X, Y, 0.0)
    info = info.cpu().numpy()
    assert info[0] == 0 and info[1] > 0
    # task 0 (Z untouched) still meets test 1 against the jitter = 0 reference
    _, _, _, bound_r, Xq, mu_r, var_r = reference(3, 0.0)
    vm, vc = vmean.cpu().numpy()[:1], vchol.cpu().numpy()[:1]
    assert np.all(np.triu(vc[0], 1) == 0.0) and np.all(np.diag(vc[0]) > 0.0)
    mu_o, var_o, _ = O.svgp_predict(pb.Z[:1], vm, vc, pb.ops[:1], Xq, jitter=0.0)
    check_predictive(mu_o, var_o, mu_r, var_r, tasks=[0], what="task 0 beside a failed task:")
    check_bound(bound.cpu().numpy()[:1], bound_r[:1], what="task 0 beside a failed task")


def test_null_pointers_are_rejected(engine):
    pb = reference(1)[0]
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    T, M, d = pb.Z.shape
    n = X.shape[0]
    pcs = (KernelParamsC * T)(*[p.to_c(d) for p in pb.kps])
    buf = torch.empty(1 << 24, dtype=torch.uint8, device=engine.device)
    q = ctypes.c_void_p(buf.data_ptr())
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    args = [pcs, T, M, 1e-4, p(Z), d, M * d, p(X), n, d, p(Y), T, q, M, q, M, M * M, q, q, q, 1 << 24]
    for k in (0, 4, 7, 10, 12, 14, 17, 18, 19):  # p, Z, X, Y, vmean, vchol, bound, info, ws
        bad = list(args)
        bad[k] = None
        assert engine.lib.gpx_svgp_fit_collapsed_f64(engine.handle, *bad) == _capi.GPX_INVALID_ARG, k
    for k, v in ((3, -1.0), (5, d - 1), (9, d - 1), (11, T - 1), (15, M - 1), (1, 0), (2, 0), (8, 0)):
        bad = list(args)
        bad[k] = v
        assert engine.lib.gpx_svgp_fit_collapsed_f64(engine.handle, *bad) == _capi.GPX_INVALID_ARG, k


# ---- 6: the drop-in's sparse large-n model, end to end -----------------------------------------------------------------
def test_dropin_sparse_large_n_model(tmp_path, engine):
    from bayesianoptimizer_amd.models import SparseGP
    from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
    from tests.oracle_engine import to_oracle_params
    from tests.stubs import BOUNDS, StubSimulator

    cfg = GPConfig(large_n_policy=True, large_n_model="sparse", fit_hyperparameters=False, max_inducing_points=16,
                   candidates_pool_size=512, acq_batch_size=8)
    sim = StubSimulator()
    opt = BayesianOptimizer(sim, BOUNDS, str(tmp_path / "sparse"), n_initial_points=40, n_batches=2, batch_size=8,
                            svgp_threshold=30, target_total=56, engine=engine, gp_config=cfg, seed=4)
    best_params, best_value = opt.optimize()
    assert best_params.shape == (5,) and np.isfinite(best_value)
    data = np.loadtxt(tmp_path / "sparse" / "optimization_results.csv", delimiter=",", skiprows=1)
    assert data.shape[0] == 56
    assert isinstance(opt.gp_model, SparseGP)
    opt.fit_gp_model()
    gp = opt.gp_model
    assert isinstance(gp, SparseGP) and gp.train_X.shape[0] == 56 and gp.svgp.Z.shape == (8, 16, 5)
    assert gp.svgp.bound.shape == (8, 6) and bool(torch.isfinite(gp.svgp.bound).all())
    # predict() is the sparse model's predictive
    xq = np.array([[0.5, 100.0, 200.0, 4.0, 5.0], [0.8, 10.0, 50.0, 3.0, 2.5], [0.3, 250.0, 20.0, 6.0, 7.0]])
    Xt = opt.x_tf(opt._tensor(opt._to_unit(xq)))
    ops = [to_oracle_params(p, 5) for p in gp.svgp.params]
    mu_r, var_r, _ = O.svgp_predict(gp.svgp.Z.cpu().numpy(), gp.svgp.vmean.cpu().numpy(), gp.svgp.vchol.cpu().numpy(),
                                    ops, Xt.cpu().numpy(), jitter=gp.svgp.jitter)
    post = gp.posterior(Xt)
    check_predictive(post.mean.cpu().numpy(), post.variance.cpu().numpy(), mu_r, var_r, what="drop-in posterior:")
    y, v = opt.predict(xq, return_var=True)
    np.testing.assert_allclose(y, opt.y_tf.inverse_mean(post.mean).cpu().numpy(), rtol=1e-12)
    np.testing.assert_array_equal(v, post.variance.cpu().numpy())
    # and it is the closed-form fit of the data the optimizer holds
    ref = SVGPModel.fit_collapsed(gp.train_X, gp.train_Y, gp.svgp.params, gp.svgp.Z, jitter=gp.svgp.jitter,
                                  engine=engine)
    assert torch.equal(ref.vmean, gp.svgp.vmean) and torch.equal(ref.vchol, gp.svgp.vchol)
    sim.cleanup()
    # every other acquisition mode says that it is not available on the sparse model
    with pytest.raises(ValueError, match="sparse"):
        BayesianOptimizer(StubSimulator(), BOUNDS, str(tmp_path / "logei"), n_initial_points=40, n_batches=2,
                          batch_size=8, svgp_threshold=30, target_total=56, engine=engine, gp_config=cfg,
                          acquisition="logei", seed=4)
