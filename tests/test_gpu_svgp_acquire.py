"""GPU tests of gpx_svgp_acquire_f64 (GPEngine.svgp_acquire): the analytic acquisition sweep on the sparse model.

* Parity with the NumPy restatement (tests/svgp_acquire_ref.py: the latent variant of oracle.svgp_predict, then
  oracle.acquisition) at the project's sweep tolerance, max |d| <= 1e-9 max(1, max |s_ref|) (tests/test_gpu_outputs.py),
  on sgpr_ref's shapes 1 (T = 1, M = 130: two row tiles, d = 3), 2 (T = 3, M = 200, d = 5) and 4 (T = 8, M = 64, d = 8)
  with 1000 candidates s N(0, 1): weights 1/T, their negation (the drop-in's min mode) and a non-trivial y_mean /
  y_scale, all four kinds with best_f = max(Y w); k = 16 gives the reference's top-k indices wherever the reference's
  17 best scores lie further apart than the measured error, and the values are the call's own scores at them.  One case
  runs on a state whose S is not contractive.
* The two bit identities with gpx_svgp_predict_f64 (the launches and the summation order are shared).
* Tails (m = 1, 255, 257) and position: a candidate's score does not depend on m, its row, index_offset or k; one call
  crosses a chunk boundary (M = 64, m = 2^20 + 300: padded M = 128 gives the chunk its 2^20 cap).
* Rejected arguments, and the drop-in with GPConfig.sparse_analytic.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import _capi
from bayesianoptimizer_amd._capi import AcqParamsC, KernelParamsC
from bayesianoptimizer_amd.engine import ACQ_KINDS
from oracle import gp_oracle as O
from tests import sgpr_ref as R
from tests import svgp_acquire_ref as AR
from tests import svgp_moments_ref as SR
from tests.oracle_engine import to_oracle_params

pytestmark = pytest.mark.gpu
KINDS = ("ei", "logei", "ucb", "variance")
M_CAND, K = 1000, 16


def dev(engine, a):
    return torch.tensor(np.array(a, dtype=np.float64), device=engine.device)


@functools.lru_cache(maxsize=None)
def case(shape, state="fit"):
    """(problem, vmean, vchol, Xs, latent mean, latent var) of one sgpr_ref shape, computed once and read-only.  state
    "fit": the closed-form fit; "arbitrary": a random mean and a random lower-triangular factor with diagonal 1.5, for
    which S S^T <= I fails (tests/svgp_moments_ref.problem's state)."""
    pb = R.problem(shape)
    T, M, s = pb.Z.shape[0], pb.Z.shape[1], R.SHAPES[shape][4]
    rng = np.random.default_rng(40 + shape)
    Xs = s * rng.standard_normal((M_CAND, pb.X.shape[1]))
    if state == "fit":
        vmean, vchol, _ = R.fit_collapsed(pb)
    else:
        vmean = rng.standard_normal((T, M))
        vchol = np.tril(rng.standard_normal((T, M, M)) / np.sqrt(M), -1) + 1.5 * np.eye(M)
    mean, var = AR.latent_moments(pb.Z, vmean, vchol, pb.ops, Xs)
    for a in (vmean, vchol, Xs, mean, var):
        a.setflags(write=False)
    return pb, vmean, vchol, Xs, mean, var


def settings(pb, setting):
    """(weights, y_mean, y_scale, best_f) of one objective over the problem's T tasks."""
    T = pb.Y.shape[1]
    w = np.full(T, 1.0 / T)
    ym = ys = None
    if setting == "negated":
        w = -w
    elif setting == "untransform":
        ym, ys = 0.3 - 0.1 * np.arange(T), 0.5 + 0.25 * np.arange(T)
    return w, ym, ys, float((pb.Y @ w).max())


def prepare(engine, pb, vmean, vchol):
    return engine.svgp_prepare(pb.kps, dev(engine, pb.Z), dev(engine, vmean), dev(engine, vchol), jitter=SR.JITTER)


def check_sweep(engine, prep, Xs, mean, var, w, ym, ys, best_f, what):
    """All four kinds: scores at the sweep tolerance, the k = 16 indices under the margin guard, values = own scores."""
    Xd = dev(engine, Xs)
    for kind in KINDS:
        ref = AR.objective_scores(mean, var, kind, w, ym, ys, best_f=best_f, beta=4.0)
        val, idx, sc = engine.svgp_acquire(prep, Xd, K, kind, best_f=best_f, beta=4.0, weights=w, y_mean=ym, y_scale=ys,
                                           return_scores=True)
        sg, val, idx = sc.cpu().numpy(), val.cpu().numpy(), idx.cpu().numpy()
        assert np.isfinite(ref).all() and np.isfinite(sg).all()
        err, tol = np.abs(sg - ref).max(), 1e-9 * max(1.0, np.abs(ref).max())
        v_ref, i_ref = O.topk_desc(ref, K + 1)
        gap = np.abs(np.diff(v_ref)).min()
        print(f"{what} {kind}: max |d score| {err:.2e} (tolerance {tol:.2e}), smallest gap of the top {K + 1} {gap:.2e}")
        assert err <= tol, f"{what} {kind}"
        # margin guard: the ranking is meaningful only where neighbours lie further apart than the score error
        assert gap > 2.0 * err, f"{what} {kind}: near-tie among the top {K + 1} (gap {gap:.3e} vs error {err:.3e})"
        np.testing.assert_array_equal(idx, i_ref[:K], err_msg=f"{what} {kind}")
        assert np.array_equal(val.view(np.int64), sg[idx].view(np.int64)), f"{what} {kind}: values are not the scores"
        # without scores_out (the workspace's own score array) and as an argmax: the same bits
        val2, idx2 = engine.svgp_acquire(prep, Xd, K, kind, best_f=best_f, beta=4.0, weights=w, y_mean=ym, y_scale=ys)
        assert np.array_equal(val2.cpu().numpy().view(np.int64), val.view(np.int64)) and \
            np.array_equal(idx2.cpu().numpy(), idx)
        v1, i1 = engine.svgp_acquire(prep, Xd, 1, kind, best_f=best_f, beta=4.0, weights=w, y_mean=ym, y_scale=ys)
        assert float(v1) == val[0] and int(i1) == idx[0]


@pytest.mark.parametrize("setting", ["mean", "negated", "untransform"])
@pytest.mark.parametrize("shape", [1, 2, 4])
def test_scores_and_topk_match_reference(engine, shape, setting):
    pb, vmean, vchol, Xs, mean, var = case(shape)
    w, ym, ys, best_f = settings(pb, setting)
    check_sweep(engine, prepare(engine, pb, vmean, vchol), Xs, mean, var, w, ym, ys, best_f, f"shape {shape} {setting}")


def test_state_that_is_not_contractive(engine):
    """S S^T <= I fails (diagonal 1.5): the second product raises the variance above the prior's; nothing assumes it
    does not."""
    pb, vmean, vchol, Xs, mean, var = case(1, "arbitrary")
    assert (var[:, 0] > O.kernel_diag(Xs, pb.ops[0])).any()
    w, ym, ys, best_f = settings(pb, "mean")
    check_sweep(engine, prepare(engine, pb, vmean, vchol), Xs, mean, var, w, ym, ys, best_f, "shape 1 arbitrary state")


# ---- the two bit identities with the predictive ----------------------------------------------------------------------
def bits(a):
    return a.view(torch.int64)


@pytest.mark.parametrize("shape", [1, 2, 4])
def test_variance_with_unit_weights_is_the_noise_free_predictive_score(engine, shape):
    pb, vmean, vchol, Xs, _, _ = case(shape)
    prep = prepare(engine, pb, vmean, vchol)
    latent = dict(prep, params=[p.replace(noise=0.0) for p in pb.kps])  # (W, W2 and alpha do not depend on the noise)
    Xd = dev(engine, Xs)
    _, _, score = engine.svgp_predict(latent, Xd, min_var=1e-10, want=("score",))
    _, _, sc = engine.svgp_acquire(prep, Xd, 1, "variance", return_scores=True)
    assert torch.equal(bits(sc), bits(score))


def test_single_task_ucb_with_beta_zero_is_the_predictive_mean(engine):
    pb, vmean, vchol, Xs, _, _ = case(1)
    prep = prepare(engine, pb, vmean, vchol)
    Xd = dev(engine, Xs)
    mu, _, _ = engine.svgp_predict(prep, Xd, want=("mean",))
    _, _, sc = engine.svgp_acquire(prep, Xd, 1, "ucb", beta=0.0, weights=[1.0], return_scores=True)
    assert torch.equal(bits(sc), bits(mu[:, 0].contiguous()))


# ---- tails and position ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 255, 257])
def test_tails(engine, m):
    """The first m rows alone, and the last m rows with an index offset: the scores of the 1000-candidate call, bit for
    bit, and the top-k of them."""
    pb, vmean, vchol, Xs, _, _ = case(2)
    w, ym, ys, best_f = settings(pb, "untransform")
    prep = prepare(engine, pb, vmean, vchol)
    kw = dict(best_f=best_f, weights=w, y_mean=ym, y_scale=ys)
    Xd = dev(engine, Xs)
    _, _, full = engine.svgp_acquire(prep, Xd, 1, "logei", return_scores=True, **kw)
    k = min(m, K)
    for rows, off in ((slice(0, m), 0), (slice(M_CAND - m, M_CAND), 12345)):
        val, idx, sc = engine.svgp_acquire(prep, Xd[rows], k, "logei", index_offset=off, return_scores=True, **kw)
        assert torch.equal(bits(sc), bits(full[rows]))
        v_ref, i_ref = O.topk_desc(sc.cpu().numpy(), k)
        np.testing.assert_array_equal(idx.cpu().numpy(), i_ref + off)
        assert np.array_equal(val.cpu().numpy().view(np.int64), v_ref.view(np.int64))
        val_m, idx_m = engine.svgp_acquire(prep, Xd[rows], m, "logei", index_offset=off, **kw)  # k = m: a full sort
        assert torch.equal(idx_m[:k], idx) and torch.equal(bits(val_m[:k]), bits(val))


def test_call_that_crosses_a_chunk(engine):
    """M = 64 (padded 128: the chunk is its 2^20 cap), T = 2, d = 3, m = 2^20 + 300: the rows past the boundary score as
    in a call of their own, and the k = 8 result is the stable top-k of the call's own scores, shifted."""
    T, M, d, C = 2, 64, 3, 1 << 20
    m = C + 300
    rng = np.random.default_rng(77)
    pb = R.problem(1)
    kps = [pb.kps[0], pb.kps[0].replace(outputscale=0.9, const_mean=0.15, lengthscale=[1.1, 0.7, 1.4])]
    Z = 0.3 * rng.standard_normal((T, M, d))
    vmean = rng.standard_normal((T, M))
    vchol = np.tril(rng.standard_normal((T, M, M)) / np.sqrt(M), -1) + 0.5 * np.eye(M)
    prep = engine.svgp_prepare(kps, dev(engine, Z), dev(engine, vmean), dev(engine, vchol), jitter=SR.JITTER)
    gen = torch.Generator(device=engine.device).manual_seed(5)
    Xd = 0.3 * torch.randn((m, d), dtype=torch.float64, device=engine.device, generator=gen)
    kw = dict(best_f=0.4, weights=[0.5, -0.5], y_mean=[0.1, -0.2], y_scale=[1.5, 0.75])
    off = 1 << 33
    val, idx, sc = engine.svgp_acquire(prep, Xd, 8, "logei", index_offset=off, return_scores=True, **kw)
    _, _, tail = engine.svgp_acquire(prep, Xd[C:], 1, "logei", return_scores=True, **kw)
    assert torch.equal(bits(sc[C:]), bits(tail))
    _, _, head = engine.svgp_acquire(prep, Xd[C - 700:C], 1, "logei", return_scores=True, **kw)
    assert torch.equal(bits(sc[C - 700:C]), bits(head))
    s = sc.cpu().numpy()
    assert np.isfinite(s).all()
    v_ref, i_ref = O.topk_desc(s, 8)
    np.testing.assert_array_equal(idx.cpu().numpy(), i_ref + off)
    assert np.array_equal(val.cpu().numpy().view(np.int64), v_ref.view(np.int64))
    # a spot check of the last rows against the reference
    mean, var = AR.latent_moments(Z, vmean, vchol, [to_oracle_params(p, d) for p in kps], Xd[C:].cpu().numpy())
    ref = AR.objective_scores(mean, var, "logei", kw["weights"], kw["y_mean"], kw["y_scale"], best_f=0.4)
    assert np.abs(s[C:] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())


# ---- rejection -------------------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing(engine):
    pb, vmean, vchol, Xs, mean, var = case(2)
    prep = prepare(engine, pb, vmean, vchol)
    T, M, d, m, k = 3, 200, 5, 300, 16
    X = dev(engine, Xs[:m])
    f64 = dict(dtype=torch.float64, device=engine.device)
    val, sc = torch.full((k,), -7.0, **f64), torch.full((m,), -7.0, **f64)
    idx = torch.full((k,), -7, dtype=torch.int64, device=engine.device)
    nb = ctypes.c_size_t()
    assert engine.lib.gpx_svgp_acquire_workspace_size(M, m, k, ctypes.byref(nb)) == _capi.GPX_OK
    ws = torch.empty(nb.value, dtype=torch.uint8, device=engine.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
    pcs = (KernelParamsC * T)(*[q.to_c(d) for q in pb.kps])
    dbl = lambda v: None if v is None else (ctypes.c_double * T)(*v)  # noqa: E731
    w = [1.0 / T] * T

    def call(k=k, m=m, beta=4.0, kind="ucb", w=w, ys=None, stride_z=M * d, ws_bytes=nb.value, index_offset=0, ldxs=d,
             Z=prep["Z"], W=prep["W"], W2=prep["W2"], alpha=prep["alpha"], Xs=X, val=val, idx=idx, ws=ws, acq=True,
             reserved=0):
        ap = AcqParamsC()
        ap.kind, ap.best_f, ap.beta, ap.y_mean, ap.y_scale, ap.reserved = ACQ_KINDS[kind], 0.1, beta, 0.0, 1.0, reserved
        engine._bind_stream()
        return engine.lib.gpx_svgp_acquire_f64(
            engine.handle, pcs, T, M, p(Z), d, stride_z, p(W), p(W2), p(alpha), dbl(w), None, dbl(ys), p(Xs), m, ldxs,
            ctypes.byref(ap) if acq else None, index_offset, k, p(val), p(idx), p(sc), p(ws), ws_bytes)

    for bad in (dict(k=0), dict(k=m + 1), dict(k=-1), dict(beta=-1.0), dict(beta=float("nan")), dict(ys=[1.0, 0.0, 1.0]),
                dict(ys=[1.0, -2.0, 1.0]), dict(Z=None), dict(W=None), dict(W2=None), dict(alpha=None), dict(Xs=None),
                dict(val=None), dict(idx=None), dict(ws=None), dict(w=None), dict(acq=False),
                dict(stride_z=M * d - 1), dict(ws_bytes=nb.value - 1), dict(index_offset=-1), dict(ldxs=d - 1),
                dict(m=0), dict(w=[1.0, float("inf"), 1.0]), dict(reserved=1)):
        assert call(**bad) == _capi.GPX_INVALID_ARG, bad
        assert engine.lib.gpx_last_error(engine.handle)
    torch.cuda.synchronize()
    assert bool((val == -7.0).all()) and bool((idx == -7).all()) and bool((sc == -7.0).all()), \
        "a rejected call wrote its outputs"
    # a negative beta is rejected for UCB only, as in the exact sweeps
    assert call(beta=-1.0, kind="logei") == _capi.GPX_OK
    assert call() == _capi.GPX_OK
    ref = AR.objective_scores(mean[:m], var[:m], "ucb", w, best_f=0.1, beta=4.0)
    assert np.abs(sc.cpu().numpy() - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    np.testing.assert_array_equal(idx.cpu().numpy(), O.topk_desc(sc.cpu().numpy(), k)[1])
    with pytest.raises(ValueError):
        engine.svgp_acquire(prep, X, 4, "ucb", weights=[1.0, 1.0])
    with pytest.raises(_capi.GPXError):
        engine.svgp_acquire(prep, X, m + 1, "ucb")


# ---- the drop-in -----------------------------------------------------------------------------------------------------
def test_dropin_sparse_analytic(tmp_path, engine):
    """tests/test_gpu_svgp_collapsed.py::test_dropin_sparse_large_n_model's settings with sparse_analytic, logEI and a
    512-point grid: optimize() completes, and acquire(8) returns the grid rows the reference ranks first."""
    from bayesianoptimizer_amd.models import SparseGP
    from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
    from tests.stubs import BOUNDS, StubSimulator

    cfg = GPConfig(large_n_policy=True, large_n_model="sparse", fit_hyperparameters=False, max_inducing_points=16,
                   candidates_pool_size=512, acq_batch_size=8, sparse_analytic=True, raw_samples=512)
    sim = StubSimulator()
    opt = BayesianOptimizer(sim, BOUNDS, str(tmp_path / "sparse"), n_initial_points=40, n_batches=2, batch_size=8,
                            svgp_threshold=30, target_total=56, engine=engine, gp_config=cfg, acquisition="logei",
                            seed=4)
    best_params, best_value = opt.optimize()
    assert best_params.shape == (5,) and np.isfinite(best_value)
    data = np.loadtxt(tmp_path / "sparse" / "optimization_results.csv", delimiter=",", skiprows=1)
    assert data.shape[0] == 56
    opt.fit_gp_model()
    gp = opt.gp_model
    assert isinstance(gp, SparseGP) and gp.train_X.shape[0] == 56
    seen = {}
    grid_of = opt._sobol_grid
    opt._sobol_grid = lambda n: seen.setdefault("grid", grid_of(n))
    batch = opt.acquire(8)
    grid = opt._tensor(seen["grid"])
    assert grid.shape == (512, 5)
    w = opt._acq_weights()
    best_f = opt._incumbent(w)
    Xg = opt.x_tf(grid)
    mean, var = AR.latent_moments(gp.svgp.Z.cpu().numpy(), gp.svgp.vmean.cpu().numpy(), gp.svgp.vchol.cpu().numpy(),
                                  [to_oracle_params(p, 5) for p in gp.params], Xg.cpu().numpy(), jitter=gp.svgp.jitter)
    ref = AR.objective_scores(mean, var, "logei", w.tolist(), best_f=best_f, beta=cfg.beta)
    _, _, sc = gp.sweep_objective(Xg, "logei", w.tolist(), best_f=best_f, beta=cfg.beta, return_scores=True)
    err = np.abs(sc.cpu().numpy() - ref).max()
    assert err <= 1e-9 * max(1.0, np.abs(ref).max())
    v_ref, order = O.topk_desc(ref, 9)
    assert np.abs(np.diff(v_ref)).min() > 2.0 * err, "near-tie among the reference's 9 best grid rows"
    assert torch.equal(batch, grid[torch.tensor(order[:8], device=grid.device)])
    sim.cleanup()
