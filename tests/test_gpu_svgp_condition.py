"""Conditioning the sparse model on new data on the GPU (gpx_svgp_condition_f64, GPEngine.svgp_condition,
SVGPPredictor / SparseGP.condition_on_observations, the drop-in's GPConfig.sparse_condition) against the NumPy refit on
all points (tests/sgpr_ref.py) and the NumPy restatement of the update (tests/svgp_condition_ref.py).

The tolerance is the project's for the predictive (tests/test_gpu_svgp_collapsed.py): |d mu| <= 1e-9 max|mu| and
|d var| <= 1e-9 max var of the likelihood-wrapped predictive.  As there, vmean / vchol are not compared entrywise."""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import NotPositiveDefiniteError, _capi
from bayesianoptimizer_amd.engine import KernelParamsC
from bayesianoptimizer_amd.models import SparseGP
from oracle import gp_oracle as O
from tests import sgpr_ref as R
from tests import svgp_acquire_ref as AR
from tests import svgp_condition_ref as CR
from tests import svgp_moments_ref as SR
from tests.test_gpu_svgp_collapsed import RTOL, check_predictive, dev, reference
from tests.test_svgp_condition_host import arbitrary_state

pytestmark = pytest.mark.gpu

# the rows each conditioning step ends at, counted back from n, and the chunk width asked for
SPLITS = {"k1": ((1, 0), 0), "k40": ((40, 0), 0), "k150": ((150, 0), 128), "two_steps": ((200, 70, 0), 0)}


def ptr(a):
    return None if a is None else ctypes.c_void_p(a.data_ptr())


def fitted_prep(engine, pb, n0):
    """The GPU's collapsed fit of the first n0 rows and its prepared state: (prep, vmean, vchol)."""
    Z = dev(engine, pb.Z)
    vmean, vchol, _ = engine.svgp_fit_collapsed(pb.kps, Z, dev(engine, pb.X[:n0]), dev(engine, pb.Y[:n0]))
    return engine.svgp_prepare(pb.kps, Z, vmean, vchol, jitter=R.JITTER), vmean, vchol


def raw_condition(engine, prep, X, Y, vmean=None, vchol=None, chunk=0, ws_bytes=None, poison=False):
    """The C call itself (no exception on info): (status, W2_out, alpha_out, vmean_out, vchol_out, info)."""
    Z = prep["Z"]
    T, M, d = Z.shape
    Mpad = prep["W2"].shape[1]
    k = X.shape[0]
    pcs = (KernelParamsC * T)(*[p.to_c(d) for p in prep["params"]])
    f64 = dict(dtype=torch.float64, device=engine.device)
    fill = float("nan") if poison else 0.0
    W2, alpha = torch.full((T, Mpad, Mpad), fill, **f64), torch.full((T, Mpad), fill, **f64)
    vm = vc = None
    if vmean is not None:
        vm, vc = torch.full((T, M), fill, **f64), torch.full((T, M, M), fill, **f64)
    info = torch.full((T,), -7, dtype=torch.int32, device=engine.device)
    nb = ctypes.c_size_t()
    assert engine.lib.gpx_svgp_condition_workspace_size(M, k, T, chunk, ctypes.byref(nb)) == _capi.GPX_OK
    ws = torch.empty(nb.value, dtype=torch.uint8, device=engine.device)
    engine._bind_stream()
    st = engine.lib.gpx_svgp_condition_f64(
        engine.handle, pcs, T, M, ptr(Z), d, M * d, ptr(prep["W"]), ptr(prep["W2"]), ptr(prep["alpha"]), ptr(X), k,
        X.stride(0), ptr(Y), Y.stride(0), ptr(W2), ptr(alpha), ptr(vmean), M, ptr(vchol), M, M * M, ptr(vm), ptr(vc),
        ptr(info), ptr(ws), nb.value if ws_bytes is None else ws_bytes)
    torch.cuda.synchronize()
    return st, W2, alpha, vm, vc, info


def check_state(prep_new, vm, vc, M):
    """The outputs' structure: the prepared blocks' padding exactly 0, vchol lower triangular with positive diagonal."""
    W2, alpha = prep_new["W2"].cpu().numpy(), prep_new["alpha"].cpu().numpy()
    assert np.all(W2[:, M:, :] == 0.0) and np.all(W2[:, :, M:] == 0.0) and np.all(alpha[:, M:] == 0.0)
    assert np.isfinite(W2).all() and np.isfinite(alpha).all()
    vc = vc.cpu().numpy()
    for t in range(vc.shape[0]):
        assert np.all(np.triu(vc[t], 1) == 0.0), f"task {t}: strict upper triangle of vchol_out"
        assert np.all(np.diag(vc[t]) > 0.0), f"task {t}: diagonal of vchol_out"
    assert np.isfinite(vm.cpu().numpy()).all()


# ---- 1: against the NumPy refit on all rows -------------------------------------------------------------------------
@pytest.mark.parametrize("split", sorted(SPLITS))
@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_conditioned_fit_matches_the_refit_on_all_points(engine, shape, split):
    pb, _, _, _, Xq, mu_r, var_r = reference(shape)
    n, M = pb.X.shape[0], pb.Z.shape[1]
    backs, chunk = SPLITS[split]
    cuts = [n - b for b in backs]
    prep, vmean, vchol = fitted_prep(engine, pb, cuts[0])
    what = f"shape {shape} {split}"
    for a, b in zip(cuts[:-1], cuts[1:]):
        before = {k: prep[k].clone() for k in ("Z", "W", "W2", "alpha")}
        vm0, vc0 = vmean.clone(), vchol.clone()
        new, vmean_new, vchol_new = engine.svgp_condition(prep, dev(engine, pb.X[a:b]), dev(engine, pb.Y[a:b]),
                                                          vmean=vmean, vchol=vchol, chunk=chunk)
        torch.cuda.synchronize()
        assert all(torch.equal(prep[k], before[k]) for k in before), f"{what}: the input state was written"
        assert torch.equal(vmean, vm0) and torch.equal(vchol, vc0), f"{what}: the input pair was written"
        assert new["W"] is prep["W"] and new["Z"] is prep["Z"] and new["M"] == prep["M"]
        check_state(new, vmean_new, vchol_new, M)
        prep, vmean, vchol = new, vmean_new, vchol_new
    Xd = dev(engine, Xq)
    mu, var, _ = engine.svgp_predict(prep, Xd, want=("mean", "var"))
    check_predictive(mu.cpu().numpy(), var.cpu().numpy(), mu_r, var_r, what=f"{what} conditioned prep:")
    again = engine.svgp_prepare(pb.kps, prep["Z"], vmean, vchol, jitter=R.JITTER)
    mu, var, _ = engine.svgp_predict(again, Xd, want=("mean", "var"))
    check_predictive(mu.cpu().numpy(), var.cpu().numpy(), mu_r, var_r, what=f"{what} prepare(vmean_out, vchol_out):")


# ---- 2: a state that is not a collapsed optimum ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", [1, 3])
def test_arbitrary_state_matches_the_restatement(engine, shape):
    pb, _, _, _, Xq, _, _ = reference(shape)
    vmean, vchol = arbitrary_state(shape)
    Xn, Yn = pb.X[:60], pb.Y[:60]
    m_ref, C_ref = CR.condition(pb.Z, vmean, vchol, pb.ops, Xn, Yn)
    mu_r, var_r, _ = O.svgp_predict(pb.Z, m_ref, C_ref, pb.ops, Xq, jitter=R.JITTER)
    vm, vc = dev(engine, vmean), dev(engine, vchol)
    prep = engine.svgp_prepare(pb.kps, dev(engine, pb.Z), vm, vc, jitter=R.JITTER)
    new, vm_new, vc_new = engine.svgp_condition(prep, dev(engine, Xn), dev(engine, Yn), vmean=vm, vchol=vc)
    check_state(new, vm_new, vc_new, pb.Z.shape[1])
    mu, var, _ = engine.svgp_predict(new, dev(engine, Xq), want=("mean", "var"))
    check_predictive(mu.cpu().numpy(), var.cpu().numpy(), mu_r, var_r, what=f"shape {shape} arbitrary state:")
    again = engine.svgp_prepare(pb.kps, prep["Z"], vm_new, vc_new, jitter=R.JITTER)
    mu, var, _ = engine.svgp_predict(again, dev(engine, Xq), want=("mean", "var"))
    check_predictive(mu.cpu().numpy(), var.cpu().numpy(), mu_r, var_r, what=f"shape {shape} arbitrary state, pair:")


# ---- 3: kriging believer --------------------------------------------------------------------------------------------
def latent_variance(engine, prep, Xs, T):
    """m x T: the latent variance of every task through the variance sweep with a one-hot weight."""
    cols = []
    for t in range(T):
        w = [1.0 if u == t else 0.0 for u in range(T)]
        cols.append(engine.svgp_acquire(prep, Xs, 1, "variance", weights=w, return_scores=True)[2])
    return torch.stack(cols, 1).cpu().numpy()


def test_conditioning_on_the_own_mean_keeps_the_mean_and_shrinks_the_variance(engine):
    pb, *_ = reference(2)
    n, d, T = pb.X.shape[0], pb.X.shape[1], pb.Y.shape[1]
    s = R.SHAPES[2][4]
    rng = np.random.default_rng(31)
    Xn, Xt = dev(engine, s * rng.standard_normal((32, d))), dev(engine, s * rng.standard_normal((512, d)))
    prep, _, _ = fitted_prep(engine, pb, n)
    fantasy, _, _ = engine.svgp_predict(prep, Xn, want=("mean",))
    new, _, _ = engine.svgp_condition(prep, Xn, fantasy)
    mu0 = engine.svgp_predict(prep, Xt, want=("mean",))[0].cpu().numpy()
    mu1 = engine.svgp_predict(new, Xt, want=("mean",))[0].cpu().numpy()
    dmu = np.abs(mu1 - mu0).max() / np.abs(mu0).max()
    both = torch.cat([Xt, Xn])
    v0, v1 = latent_variance(engine, prep, both, T), latent_variance(engine, new, both, T)
    rise = (v1 - v0).max() / v0.max()
    drop = (v0[512:] - v1[512:]).min()
    print(f"|d mu| / max|mu| = {dmu:.2e}, largest rise of the variance / max var = {rise:.2e}, smallest drop at the "
          f"conditioned points = {drop:.3e}")
    assert dmu <= RTOL and rise <= RTOL
    assert drop > 0.0, "the latent variance falls at every conditioned point"


# ---- 4 + 5: determinism, chunk widths, the optional pair -------------------------------------------------------------
def test_calls_are_bit_identical_and_chunk_widths_agree(engine):
    pb, _, _, _, Xq, mu_r, var_r = reference(2)
    n = pb.X.shape[0]
    prep, vmean, vchol = fitted_prep(engine, pb, n - 150)
    Xn, Yn = dev(engine, pb.X[n - 150:]), dev(engine, pb.Y[n - 150:])
    outs = {}
    for chunk in (128, 0):  # two chunks of 128 and 22 columns; the default: one chunk
        first = raw_condition(engine, prep, Xn, Yn, vmean, vchol, chunk=chunk)
        again = raw_condition(engine, prep, Xn, Yn, vmean, vchol, chunk=chunk)
        assert first[0] == _capi.GPX_OK and again[0] == _capi.GPX_OK
        assert int(first[5].abs().max()) == 0
        for a, b in zip(first[1:], again[1:]):
            assert torch.equal(a, b), f"chunk {chunk}: two calls differ"
        new = dict(prep, W2=first[1], alpha=first[2])
        mu, var, _ = engine.svgp_predict(new, dev(engine, Xq), want=("mean", "var"))
        check_predictive(mu.cpu().numpy(), var.cpu().numpy(), mu_r, var_r, what=f"chunk {chunk}:")
        outs[chunk] = first
    # the variational pair left out: the same bits of the prepared blocks
    for chunk in (128, 0):
        bare = raw_condition(engine, prep, Xn, Yn, None, None, chunk=chunk)
        assert bare[0] == _capi.GPX_OK and bare[3] is None
        assert torch.equal(bare[1], outs[chunk][1]) and torch.equal(bare[2], outs[chunk][2])
    # the engine passes the size it asked for, not its cached buffer's: a narrow call after a wide one still runs narrow
    engine.svgp_condition(prep, Xn, Yn)
    narrow, _, _ = engine.svgp_condition(prep, Xn, Yn, chunk=128)
    assert torch.equal(narrow["W2"], outs[128][1]) and torch.equal(narrow["alpha"], outs[128][2])


# ---- 6: what stands on the conditioned model ------------------------------------------------------------------------
def test_sweep_and_moments_on_a_conditioned_sparse_model_match_the_refit(engine):
    pb, ref_m, ref_C, _, _, _, _ = reference(3)
    n, d, T = pb.X.shape[0], pb.X.shape[1], pb.Y.shape[1]
    s = R.SHAPES[3][4]
    rng = np.random.default_rng(41)
    Xs = s * rng.standard_normal((700, d))
    w = [1.0, -0.5]
    best_f = float((pb.Y @ np.array(w)).mean())
    # the reference's eight best EI scores are separated (checked on the CPU), so the indices are decided
    mean_r, var_r = AR.latent_moments(pb.Z, ref_m, ref_C, pb.ops, Xs)
    scores_r = AR.objective_scores(mean_r, var_r, "ei", w, best_f=best_f)
    top = np.sort(scores_r)[::-1][:9]
    gap = np.abs(np.diff(top)).min()
    print(f"smallest gap among the nine best reference EI scores: {gap:.3e}")
    assert gap > 1e-6
    X, Y, Z = dev(engine, pb.X), dev(engine, pb.Y), dev(engine, pb.Z)
    part = SparseGP(X[:n - 40], Y[:n - 40], pb.kps, Z, jitter=R.JITTER, engine=engine)
    cond = part.condition_on_observations(X[n - 40:], Y[n - 40:])
    full = SparseGP(X, Y, pb.kps, Z, jitter=R.JITTER, engine=engine)
    assert isinstance(cond, SparseGP) and cond.train_X.shape[0] == n and cond.train_Y.shape == (n, T)
    assert part.train_X.shape[0] == n - 40 and cond.svgp.bound is None and cond.svgp.Z is part.svgp.Z
    Xd = dev(engine, Xs)
    val_c, idx_c = cond.sweep_objective_topk(Xd, "ei", w, 8, best_f=best_f)
    val_f, idx_f = full.sweep_objective_topk(Xd, "ei", w, 8, best_f=best_f)
    assert idx_c.tolist() == idx_f.tolist() == np.argsort(-scores_r, kind="stable")[:8].tolist()
    np.testing.assert_allclose(val_c.cpu().numpy(), val_f.cpu().numpy(), rtol=0, atol=1e-9 * np.abs(top).max())
    q = 4
    Xq = Xd[:64]
    for t in range(T):
        got = [v.cpu().numpy() for v in engine.svgp_moments_grad(cond.predictor.prep, t, Xq, q)]
        ref = [v.cpu().numpy() for v in engine.svgp_moments_grad(full.predictor.prep, t, Xq, q)]
        ps = SR.prior_scale(pb.ops[t], Xs[:64])
        e = (np.abs(got[0] - ref[0]).max() / np.abs(ref[0]).max(), np.abs(got[1] - ref[1]).max() / np.abs(ref[1]).max(),
             np.abs(got[2] - ref[2]).max() / ps, np.abs(got[3] - ref[3]).max() / np.abs(ref[3]).max())
        print(f"task {t}: |d mean| {e[0]:.1e}  |d dmean| {e[1]:.1e}  |d cov| / prior {e[2]:.1e}  |d dcov| {e[3]:.1e}")
        assert e[0] <= 1e-9 and e[2] <= 1e-9 and e[1] <= 1e-8 and e[3] <= 1e-8
    # the states the MC acquisitions read come from the conditioned prep
    assert all(st.prep is cond.predictor.prep for st in cond.states)


# ---- 7: argument checks ---------------------------------------------------------------------------------------------
def test_invalid_arguments_are_rejected_and_a_nan_is_reported_per_task(engine):
    pb, _, _, _, Xq, mu_r, var_r = reference(3)
    n = pb.X.shape[0]
    T, M, d = pb.Z.shape
    Mpad = 256
    prep, vmean, vchol = fitted_prep(engine, pb, n - 40)
    Xn, Yn = dev(engine, pb.X[n - 40:]), dev(engine, pb.Y[n - 40:])
    pcs = (KernelParamsC * T)(*[p.to_c(d) for p in pb.kps])
    f64 = dict(dtype=torch.float64, device=engine.device)
    W2o, ao = torch.zeros((T, Mpad, Mpad), **f64), torch.zeros((T, Mpad), **f64)
    vmo, vco = torch.zeros((T, M), **f64), torch.zeros((T, M, M), **f64)
    info = torch.zeros(T, dtype=torch.int32, device=engine.device)
    nb = ctypes.c_size_t()
    assert engine.lib.gpx_svgp_condition_workspace_size(M, 40, T, 128, ctypes.byref(nb)) == _capi.GPX_OK
    ws = torch.empty(nb.value, dtype=torch.uint8, device=engine.device)
    #       0    1  2  3            4  5      6               7                8
    args = [pcs, T, M, ptr(prep["Z"]), d, M * d, ptr(prep["W"]), ptr(prep["W2"]), ptr(prep["alpha"]),
            # 9     10  11 12       13 14        15       16          17 18          19 20     21        22
            ptr(Xn), 40, d, ptr(Yn), T, ptr(W2o), ptr(ao), ptr(vmean), M, ptr(vchol), M, M * M, ptr(vmo), ptr(vco),
            # 23       24       25
            ptr(info), ptr(ws), nb.value]
    call = lambda a: engine.lib.gpx_svgp_condition_f64(engine.handle, *a)  # noqa: E731
    for k in (0, 3, 6, 7, 8, 9, 12, 14, 15, 23, 24):  # every required pointer
        bad = list(args)
        bad[k] = None
        assert call(bad) == _capi.GPX_INVALID_ARG, k
    for k in (16, 18, 21, 22):  # a mixed optional set
        bad = list(args)
        bad[k] = None
        assert call(bad) == _capi.GPX_INVALID_ARG, k
    for k, v in ((14, args[7]), (15, args[8]), (21, args[16]), (22, args[18])):  # every forbidden alias
        bad = list(args)
        bad[k] = v
        assert call(bad) == _capi.GPX_INVALID_ARG, k
    for k, v in ((10, 0), (10, (1 << 30) + 1), (4, d - 1), (11, d - 1), (13, T - 1), (19, M - 1), (5, M * d - 1),
                 (17, M - 1), (20, M * M - 1), (1, 0), (2, 0), (25, nb.value - 1)):
        bad = list(args)
        bad[k] = v
        assert call(bad) == _capi.GPX_INVALID_ARG, (k, v)
    zero_noise = (KernelParamsC * T)(*[p.to_c(d) for p in pb.kps])
    zero_noise[1].noise = 0.0
    assert call([zero_noise] + args[1:]) == _capi.GPX_INVALID_ARG
    assert "noise" in engine.lib.gpx_last_error(engine.handle).decode()
    torch.cuda.synchronize()
    assert float(W2o.abs().max()) == 0.0 and float(vco.abs().max()) == 0.0, "a rejected call launches nothing"
    # the arguments as they stand are a valid call
    assert call(args) == _capi.GPX_OK, engine.lib.gpx_last_error(engine.handle)
    torch.cuda.synchronize()
    assert info.tolist() == [0, 0]
    # a NaN among the new observations of task 1: reported for that task, task 0 is computed
    Ybad = Yn.clone()
    Ybad[7, 1] = float("nan")
    st, W2, alpha, vm, vc, inf = raw_condition(engine, prep, Xn, Ybad, vmean, vchol)
    assert st == _capi.GPX_OK
    inf = inf.tolist()
    assert inf[0] == 0 and inf[1] > 0
    with pytest.raises(NotPositiveDefiniteError, match="task 1"):
        engine.svgp_condition(prep, Xn, Ybad)
    one = {"Z": prep["Z"][:1], "W": prep["W"][:1], "W2": W2[:1].contiguous(), "alpha": alpha[:1].contiguous(),
           "params": pb.kps[:1], "M": M}
    mu, var, _ = engine.svgp_predict(one, dev(engine, Xq), want=("mean", "var"))
    check_predictive(mu.cpu().numpy(), var.cpu().numpy(), mu_r, var_r, tasks=[0], what="task 0 beside a failed task:")


# ---- 8: the drop-in -------------------------------------------------------------------------------------------------
def test_dropin_round_of_40_points_on_the_sparse_model(tmp_path, engine):
    from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
    from tests.stubs import BOUNDS, StubSimulator

    cfg = GPConfig(large_n_policy=True, large_n_model="sparse", fit_hyperparameters=False, max_inducing_points=16,
                   num_restarts=2, acqf_raw_samples=32, maxiter=20, mc_samples=64, sparse_condition=True)
    sim = StubSimulator()
    opt = BayesianOptimizer(sim, BOUNDS, str(tmp_path / "qlogei"), n_initial_points=40, n_batches=1, batch_size=40,
                            svgp_threshold=30, target_total=80, engine=engine, gp_config=cfg, acquisition="qlogei",
                            seed=4)
    opt._initial_design()
    opt.fit_gp_model()
    assert isinstance(opt.gp_model, SparseGP)
    batch = opt.acquire(40)
    assert batch.shape == (40, 5) and bool(torch.isfinite(batch).all())
    assert float(batch.min()) >= 0.0 and float(batch.max()) <= 1.0
    sim.cleanup()
