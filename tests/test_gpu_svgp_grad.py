"""Hyperparameter gradient of the collapsed SVGP bound on the GPU (gpx_svgp_bound_grad_f64,
GPEngine.svgp_bound_value_grad, mll.fit_hyperparameters_sparse, GPConfig.sparse_hyperparameters = "bound") against the
torch-autograd reference (a) of tests/sgpr_grad_ref.py.

Tolerance: every gradient entry within tau of the sum of the absolute values of its parts (sgpr_grad_ref.TAU = 32 tau0,
tau0 the measured disagreement of the two CPU references; tests/test_svgp_grad_host.py).  The bound itself as
test_gpu_svgp_collapsed.py checks it, and bit for bit against gpx_svgp_fit_collapsed_f64."""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import NotPositiveDefiniteError, _capi
from bayesianoptimizer_amd.engine import KernelParamsC
from bayesianoptimizer_amd.mll import default_spec, fit_hyperparameters_sparse, objective_outputs
from tests import sgpr_grad_ref as G
from tests import sgpr_ref as R

pytestmark = pytest.mark.gpu


def dev(engine, a):
    return torch.tensor(np.asarray(a), device=engine.device)


def check_value(got, ref, what=""):
    scale = np.abs(ref["bound"][1:]).sum()
    err = np.abs(got["bound"] - ref["bound"]) / scale
    print(f"{what}: F = {got['bound'][0]:.6f} (ref {ref['bound'][0]:.6f}), |d| / sum|terms| = "
          + " ".join(f"{e:.1e}" for e in err))
    assert np.all(err <= 1e-9), what
    assert got["nll"] == -got["bound"][0]


def raw_grad(engine, kps, Z, X, Y, jitter, chunk=0, ws_bytes=None):
    """The C call itself (no exception on info): (status, out, info)."""
    T, M, d = Z.shape
    n = X.shape[0]
    pcs = (KernelParamsC * T)(*[p.to_c(d) for p in kps])
    out = torch.full((T, _capi.SVGP_GRAD_NOUT), float("nan"), dtype=torch.float64, device=engine.device)
    info = torch.full((T,), -7, dtype=torch.int32, device=engine.device)
    nb = ctypes.c_size_t()
    assert engine.lib.gpx_svgp_bound_grad_workspace_size(M, n, T, chunk, ctypes.byref(nb)) == _capi.GPX_OK
    ws = torch.empty(nb.value, dtype=torch.uint8, device=engine.device)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    engine._bind_stream()
    st = engine.lib.gpx_svgp_bound_grad_f64(engine.handle, pcs, T, M, float(jitter), p(Z), Z.stride(1), Z.stride(0),
                                            p(X), n, X.stride(0), p(Y), Y.stride(0), p(out), p(info), p(ws),
                                            nb.value if ws_bytes is None else ws_bytes)
    torch.cuda.synchronize()
    return st, out, info


# ---- 1: the gradient against autograd, every shape and kind ---------------------------------------------------------
@pytest.mark.parametrize("shape", [1, 2, 3, 4, 16] + list(G.DSHAPES))
@pytest.mark.parametrize("kind", G.KINDS)
def test_gradient_matches_autograd(engine, shape, kind):
    """sgpr_grad_ref.DSHAPES (d = 4, 9, 16, 17, 32): every DMAX instance at its widest d and the next at its narrowest;
    d = 17 and 32 run the two 16-dimension sweeps of the DMAX = 32 instance."""
    pb, kps, refs = G.reference(shape, kind)
    got = engine.svgp_bound_value_grad(kps, dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y), jitter=R.JITTER)
    assert len(got) == len(refs)
    for t, (g, a) in enumerate(zip(got, refs)):
        check_value(g, a, what=f"shape {shape} {kind} task {t}")
        G.check_grad(g, a, what=f"shape {shape} {kind} task {t}")
        if kind != "scale_linear_matern52":
            assert np.all(g["linear_variance"] == 0.0)


# ---- 2: the bound's bits are the fit's ------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [128, None])
def test_bound_bits_equal_the_fit(engine, chunk):
    pb = G.problem(2)
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    _, _, bound = engine.svgp_fit_collapsed(pb.kps, Z, X, Y, chunk=chunk)
    out, info = engine.svgp_bound_grad(pb.kps, Z, X, Y, chunk=chunk)
    assert int(info.abs().sum()) == 0
    assert torch.equal(out[:, _capi.SVGP_GRAD_BOUND:_capi.SVGP_GRAD_BOUND + _capi.SVGP_BOUND_NOUT], bound)
    assert torch.equal(out[:, _capi.SVGP_GRAD_MLL + _capi.MLL_NLL], -bound[:, _capi.SVGP_BOUND_F])


# ---- 3: chunk widths and determinism -------------------------------------------------------------------------------
def test_chunk_widths_agree_and_calls_are_bit_identical(engine):
    pb, kps, refs = G.reference(1, "scale_linear_matern52")
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    narrow = engine.svgp_bound_value_grad(kps, Z, X, Y, chunk=128)  # 520 points: five chunks, the last of 8
    wide = engine.svgp_bound_value_grad(kps, Z, X, Y)
    for t, a in enumerate(refs):
        G.check_grad(narrow[t], a, what=f"chunk 128 task {t}")
        G.check_grad(wide[t], a, what=f"default chunk task {t}")
        # the two widths against each other, on the same yardstick
        assert G.entry_ratio(dict(narrow[t], scale=a["scale"]), dict(wide[t], scale=a["scale"])) <= G.TAU
    for chunk in (128, None):
        a, ia = engine.svgp_bound_grad(kps, Z, X, Y, chunk=chunk)
        b, ib = engine.svgp_bound_grad(kps, Z, X, Y, chunk=chunk)
        assert torch.equal(a, b) and torch.equal(ia, ib), f"chunk {chunk}: two calls differ"


# ---- 4: strided arguments ------------------------------------------------------------------------------------------
def test_strided_arguments_give_the_same_bits(engine):
    pb = G.problem(2)
    n, d = pb.X.shape
    T, M = pb.Y.shape[1], pb.Z.shape[1]
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    base, _ = engine.svgp_bound_grad(pb.kps, Z, X, Y)
    nan = dict(fill_value=float("nan"), dtype=torch.float64, device=engine.device)
    Xw, Yw, Zw = torch.full((n, d + 3), **nan), torch.full((n, T + 4), **nan), torch.full((T, M + 2, d + 5), **nan)
    Xw[:, :d], Yw[:, 2:2 + T], Zw[:, :M, :d] = X, Y, Z
    Xs, Ys, Zs = Xw[:, :d], Yw[:, 2:2 + T], Zw[:, :M, :d]
    assert Xs.stride(0) == d + 3 and Ys.stride(0) == T + 4 and Zs.stride(1) == d + 5 and Zs.stride(0) == (M + 2) * (d + 5)
    st, strided, info = raw_grad(engine, pb.kps, Zs, Xs, Ys, R.JITTER)
    assert st == _capi.GPX_OK and int(info.abs().sum()) == 0
    assert torch.equal(base, strided)
    again, _ = engine.svgp_bound_grad(pb.kps, Zs, Xs, Ys)  # the engine keeps the strides too
    assert torch.equal(base, again)


# ---- 5: a failed K_ZZ is reported, and the other tasks are computed ----------------------------------------------------
def test_kzz_failure_is_reported_per_task(engine):
    """jitter = 0 and, in task 1 of 2, one inducing point repeated seven times (test_gpu_svgp_collapsed.py): K_ZZ of
    task 1 is exactly singular; task 0 still meets test 1's check against the jitter = 0 reference."""
    pb, kps, refs = G.reference(3, "scale_linear_matern52", 0.0, (0,))
    Z = pb.Z.copy()
    Z[1, 40:47] = Z[1, 39]
    Zd, X, Y = dev(engine, Z), dev(engine, pb.X), dev(engine, pb.Y)
    with pytest.raises(NotPositiveDefiniteError, match="task 1"):
        engine.svgp_bound_value_grad(kps, Zd, X, Y, jitter=0.0)
    st, out, info = raw_grad(engine, kps, Zd, X, Y, 0.0)
    info = info.cpu().numpy()
    assert st == _capi.GPX_OK and info[0] == 0 and info[1] > 0
    r = out[0].cpu().numpy()
    g = r[_capi.SVGP_GRAD_MLL:]
    d = pb.X.shape[1]
    got = {"nll": g[_capi.MLL_NLL], "noise": g[_capi.MLL_D_NOISE], "outputscale": g[_capi.MLL_D_OUTPUTSCALE],
           "const_mean": g[_capi.MLL_D_MEAN], "lengthscale": g[_capi.MLL_D_LENGTHSCALE:_capi.MLL_D_LENGTHSCALE + d],
           "linear_variance": g[_capi.MLL_D_LINVAR:_capi.MLL_D_LINVAR + d], "bound": r[:_capi.SVGP_BOUND_NOUT]}
    check_value(got, refs[0], what="task 0 beside a failed task")
    G.check_grad(got, refs[0], what="task 0 beside a failed task")


# ---- 6: the workspace ----------------------------------------------------------------------------------------------
def test_workspace_size_and_refusal(engine):
    pb = G.problem(3)
    T, M, d = pb.Z.shape
    sizes = []
    for n in (pb.X.shape[0], 100_000):
        nb = ctypes.c_size_t()
        assert engine.lib.gpx_svgp_bound_grad_workspace_size(M, n, T, 128, ctypes.byref(nb)) == _capi.GPX_OK
        sizes.append(nb.value)
    assert sizes[0] == sizes[1], "the workspace must not depend on n"
    Z, X, Y = dev(engine, pb.Z), dev(engine, pb.X), dev(engine, pb.Y)
    st, _, _ = raw_grad(engine, pb.kps, Z, X, Y, R.JITTER, chunk=128, ws_bytes=sizes[0] - 1)
    assert st == _capi.GPX_INVALID_ARG
    st, out, info = raw_grad(engine, pb.kps, Z, X, Y, R.JITTER, chunk=128, ws_bytes=sizes[0])
    assert st == _capi.GPX_OK and bool(torch.isfinite(out).all())
    # the engine passes the size it asked for: a narrow call after a wide one still runs narrow
    engine.svgp_bound_grad(pb.kps, Z, X, Y)
    narrow, _ = engine.svgp_bound_grad(pb.kps, Z, X, Y, chunk=128)
    assert torch.equal(narrow, out)


# ---- 7: the driver on the GPU --------------------------------------------------------------------------------------
def test_fit_hyperparameters_sparse_gpu(engine):
    pb = G.problem(3)
    n, d = pb.X.shape
    T = pb.Y.shape[1]
    kind = "scale_linear_matern52"
    res = fit_hyperparameters_sparse(engine, dev(engine, pb.X), dev(engine, pb.Y), dev(engine, pb.Z), kind, "none",
                                     options={"maxiter": 15})
    assert np.isfinite(res.loss) and res.n_evals >= 2
    specs = [default_spec(kind, d, "none") for _ in range(T)]
    vg = G.value_grad_all(pb.Z, pb.X, pb.Y)
    f = objective_outputs(specs, vg, n)
    start, _ = f(np.concatenate([sp.x0() for sp in specs]))
    refs = vg(res.params)  # (a) at the returned parameters
    scale = sum(np.abs(a["bound"][1:]).sum() for a in refs) / n
    ref_loss = sum(a["nll"] for a in refs) / n
    print(f"loss {res.loss:.12f}, (a) at the result {ref_loss:.12f}, |d| / sum|terms| = "
          f"{abs(res.loss - ref_loss) / scale:.2e}; start {start:.6f}; {res.n_evals} evaluations")
    assert abs(res.loss - ref_loss) <= 1e-9 * scale
    assert res.loss < start


# ---- 8: the drop-in with sparse_hyperparameters = "bound" ------------------------------------------------------------
def test_dropin_bound_hyperparameters(tmp_path, engine):
    from bayesianoptimizer_amd.models import SparseGP
    from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
    from bayesianoptimizer_amd.svgp import SVGPModel
    from tests.stubs import BOUNDS, StubSimulator

    def make(mode):
        cfg = GPConfig(large_n_policy=True, large_n_model="sparse", fit_hyperparameters=True, prior_set="none",
                       mll_options={"maxiter": 20}, sparse_hyperparameters=mode, max_inducing_points=16,
                       candidates_pool_size=512, acq_batch_size=8)
        sim = StubSimulator()
        return sim, BayesianOptimizer(sim, BOUNDS, str(tmp_path / mode), n_initial_points=40, n_batches=2, batch_size=8,
                                      svgp_threshold=30, target_total=56, engine=engine, gp_config=cfg, seed=4,
                                      acquisition="variance")

    sim, opt = make("bound")
    best_params, best_value = opt.optimize()  # fit -> predict -> pool scan, twice
    assert best_params.shape == (5,) and np.isfinite(best_value)
    opt.fit_gp_model()
    sim.cleanup()
    gp = opt.gp_model
    assert isinstance(gp, SparseGP) and gp.train_X.shape[0] == 56 and gp.svgp.Z.shape == (8, 16, 5)
    assert opt.sparse_hyper_result is not None and np.isfinite(opt.sparse_hyper_result.loss)
    y, v = opt.predict(np.array([[0.5, 100.0, 200.0, 4.0, 5.0]]), return_var=True)
    assert np.all(np.isfinite(y)) and np.all(v > 0)
    # The "subsample" mode's hyperparameters for the same data, and their bound on the same Z: "bound" maximises it
    sim, sub = make("subsample")
    sub.train_X, sub.train_Y_raw = opt.train_X.clone(), opt.train_Y_raw.clone()
    sub.fit_gp_model()
    sim.cleanup()
    assert sub.sparse_hyper_result is None and torch.equal(sub.gp_model.train_X, gp.train_X)
    assert torch.equal(sub.gp_model.train_Y, gp.train_Y)
    other = SVGPModel.fit_collapsed(gp.train_X, gp.train_Y, sub.gp_model.params, gp.svgp.Z, jitter=gp.svgp.jitter,
                                    engine=engine)
    F_bound, F_sub = float(gp.svgp.bound[:, 0].sum()), float(other.bound[:, 0].sum())
    print(f"sum over tasks of F: bound mode {F_bound:.4f}, subsample hyperparameters {F_sub:.4f}")
    assert F_bound >= F_sub
