"""The pruned top-k sweep over independent outputs (gpx_acquire_topk_multi_f64) against the composition it
replaces.

The yardstick everywhere is int64-equal values and equal indices against ``acquire_multi(return_scores=True)`` followed
by ``engine.topk`` on the same handle, and a second check against a numpy stable sort of those scores' keys (gpx_topk_f64
sorts the key NaN -> -inf, -0 -> +0 and returns it).  Problem and candidates: tests/multi_sweep_util.py (T = 3 outputs with
their own kernels, d = 4, m = 5000: a 1024-candidate seed block, then 3976 staged candidates with a partial last tile;
padded n = 384, 640, 1024: 3, 5 and 8 row tiles).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import KernelParams, _capi
from bayesianoptimizer_amd._capi import GPXError
from tests import multi_sweep_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
M = U.M
_fits = {}


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def fitted(engine, n, T=3, **kw):
    """(states, problem) of one configuration, fitted once for the whole module; never modified."""
    key = (n, T, tuple(sorted(kw.items())))
    if key not in _fits:
        pr = U.problem(n, T, **kw)
        _fits[key] = (engine.fit_outputs(t(pr["X"]), t(pr["Y"]), pr["params"]), pr)
    return _fits[key]


def objective(pr, **over):
    kw = dict(best_f=pr["best_f"], beta=U.BETA, weights=pr["w"], y_mean=pr["ym"], y_scale=pr["ys"])
    kw.update(over)
    return kw


def bits(v):
    return v.view(torch.int64).cpu().numpy()


def topk(engine, prune, states, Xs, k, acq, **kw):
    """(value bits, indices, sweep_stats) of one acquire_topk_multi call with sweep_prune = prune, restored afterwards."""
    before = engine.get_option("sweep_prune")
    engine.set_option("sweep_prune", prune)
    try:
        v, i = engine.acquire_topk_multi(states, Xs, k, acq, **kw)
        stats = engine.sweep_stats()
    finally:
        engine.set_option("sweep_prune", before)
    assert v.shape == (k,) and i.shape == (k,) and v.dtype == torch.float64 and i.dtype == torch.int64
    return bits(v), i.cpu().numpy(), stats


def composition(engine, states, Xs, acq, **kw):
    """The scores of the full multi-output sweep (a device tensor) and their numpy key (NaN -> -inf, -0 -> +0)."""
    kw = {k: v for k, v in kw.items() if k != "index_offset"}
    _, _, sc = engine.acquire_multi(states, Xs, acq, return_scores=True, **kw)
    s = sc.cpu().numpy()
    return sc, np.where(np.isnan(s), -np.inf, s) + 0.0


def check(engine, got, sc, key, k, offset=0):
    """got = (value bits, indices, ...) against engine.topk of the scores and against a stable sort of their keys."""
    v_ref, i_ref = engine.topk(sc, k)
    assert np.array_equal(got[1], i_ref.cpu().numpy() + offset), (got[1][:8], i_ref[:8])
    assert np.array_equal(got[0], bits(v_ref))
    order = np.argsort(-key, kind="stable")[:k]
    assert np.array_equal(got[1], order + offset)
    assert np.array_equal(got[0], key[order].view(np.int64))


@pytest.mark.parametrize("n", [384, 640, 1000])
@pytest.mark.parametrize("acq", U.ACQS)
def test_equal_bits(engine, acq, n):
    states, pr = fitted(engine, n)
    Xs = t(U.candidates())
    kw = objective(pr)
    sc, key = composition(engine, states, Xs, acq, **kw)
    full_tiles = 3 * ((M + 127) // 128) * (engine.padded_n(n) // 128)
    for k in (1, 16, 300):
        for prune in (2, 0):
            got = topk(engine, prune, states, Xs, k, acq, **kw)
            print(f"n = {n}, {acq}, k = {k}, sweep_prune = {prune}: sweep_stats {got[2]}")
            check(engine, got, sc, key, k)
            assert got[2][0] == M and got[2][3] == full_tiles
            if prune == 0:
                assert got[2][1] == M and got[2][2] == got[2][3]


@pytest.mark.parametrize("acq", U.ACQS)
def test_k1_is_the_argmax_call(engine, acq):
    """The pair gpx_acquire_argmax_multi_f64 returns, after the top-k call's keying (NaN -> -inf, -0 -> +0)."""
    for n in (384, 640, 1000):
        states, pr = fitted(engine, n)
        Xs = t(U.candidates())
        kw = objective(pr)
        bv, bi = engine.acquire_multi(states, Xs, acq, **kw)
        got = topk(engine, 2, states, Xs, 1, acq, **kw)
        ref = torch.where(torch.isnan(bv), torch.full_like(bv, -np.inf), bv) + 0.0
        assert got[0][0] == int(bits(ref)[0]) and got[1][0] == int(bi.item())


@pytest.mark.parametrize("kind", U.KINDS)
def test_one_output_with_unit_weight_is_acquire_topk(engine, kind):
    states, pr = fitted(engine, 640, 1, kinds=(kind,))
    Xs = t(U.candidates())
    for acq in U.ACQS:
        for k in (1, 16):
            engine.set_option("sweep_prune", 2)
            try:
                v1, i1 = engine.acquire_topk(states[0], Xs, k, acq, best_f=0.3, beta=2.0, y_mean=0.2, y_scale=1.5)
            finally:
                engine.set_option("sweep_prune", 1)
            got = topk(engine, 2, states, Xs, k, acq, best_f=0.3, beta=2.0, weights=[1.0], y_mean=[0.2], y_scale=[1.5])
            assert np.array_equal(got[0], bits(v1)) and np.array_equal(got[1], i1.cpu().numpy()), (kind, acq, k)


@pytest.mark.parametrize("acq", ["ucb", "logei"])
def test_negative_and_zero_weights(engine, acq):
    """The mean is exact whatever the weights' signs; the variance's terms carry w_t^2."""
    states, pr = fitted(engine, 640)
    Xs = t(U.candidates())
    kw = objective(pr, weights=[0.7, -0.4, 0.0])
    sc, key = composition(engine, states, Xs, acq, **kw)
    for k in (1, 16):
        got = topk(engine, 2, states, Xs, k, acq, **kw)
        check(engine, got, sc, key, k)
        assert got[2][2] < got[2][3]


@pytest.mark.parametrize("acq", U.ACQS)
def test_call_options(engine, acq):
    states, pr = fitted(engine, 640)
    Xs = t(U.candidates())
    off = 7 * 2 ** 20
    kw = objective(pr, index_offset=off, y_mean=[0.3, -0.2, 0.05], y_scale=[1.7, 0.6, 1.1])
    sc, key = composition(engine, states, Xs, acq, **kw)
    first = topk(engine, 2, states, Xs, 16, acq, **kw)
    check(engine, first, sc, key, 16, offset=off)
    again = topk(engine, 2, states, Xs, 16, acq, **kw)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        on_stream = topk(engine, 2, states, Xs, 16, acq, **kw)
    stream.synchronize()
    assert np.array_equal(first[0], on_stream[0]) and np.array_equal(first[1], on_stream[1])


def test_limits(engine):
    states, pr = fitted(engine, 640)
    kw = objective(pr)
    Xs = t(U.candidates())
    sc, key = composition(engine, states, Xs, "logei", **kw)
    check(engine, topk(engine, 2, states, Xs, 1024, "logei", **kw), sc, key, 1024)
    # below the seed block: no staged columns, the whole set comes back sorted
    Xs7 = t(U.candidates()[:700])
    sc7, key7 = composition(engine, states, Xs7, "logei", **kw)
    got = topk(engine, 2, states, Xs7, 700, "logei", **kw)
    check(engine, got, sc7, key7, 700)
    assert sorted(got[1].tolist()) == list(range(700)) and got[2][1] == 700
    for Xq, k in [(Xs, 1025), (Xs7, 701), (Xs, 0)]:
        with pytest.raises(GPXError) as e:
            engine.acquire_topk_multi(states, Xq, k, "logei", **kw)
        assert e.value.status == _capi.GPX_INVALID_ARG
    # the entry point itself, with a workspace that is large enough for any legal k
    nbytes = ctypes.c_size_t()
    n, T = states[0].n, len(states)
    assert engine.lib.gpx_acquire_topk_multi_workspace_size(n, M, 1024, ctypes.byref(nbytes)) == _capi.GPX_OK
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    val = torch.full((1100,), 7.0, dtype=torch.float64, device=DEV)
    idx = torch.full((1100,), 7, dtype=torch.int64, device=DEV)
    ap = _capi.AcqParamsC()
    ap.kind, ap.best_f, ap.beta, ap.y_mean, ap.y_scale = 1, kw["best_f"], 4.0, 0.0, 1.0
    pcs = (_capi.KernelParamsC * T)(*[st.params.to_c(st.d) for st in states])
    alphas = [st.alpha[:, 0].contiguous() for st in states]
    wp = (ctypes.c_void_p * T)(*[st.W.data_ptr() for st in states])
    ldw = (ctypes.c_int64 * T)(*[st.W.stride(0) for st in states])
    ap_ = (ctypes.c_void_p * T)(*[a.data_ptr() for a in alphas])
    dbl = ctypes.c_double * T
    vp = ctypes.c_void_p
    X = states[0].X
    for m, k in [(M, 1025), (700, 701), (M, 0), (M, -1)]:
        rc = engine.lib.gpx_acquire_topk_multi_f64(
            engine.handle, pcs, T, n, vp(X.data_ptr()), X.stride(0), wp, ldw, ap_, dbl(*kw["weights"]),
            dbl(*kw["y_mean"]), dbl(*kw["y_scale"]), vp(Xs.data_ptr()), m, Xs.stride(0), ctypes.byref(ap), 0, k,
            vp(val.data_ptr()), vp(idx.data_ptr()), vp(ws.data_ptr()), ws.numel())
        assert rc == _capi.GPX_INVALID_ARG, (m, k)
    torch.cuda.synchronize()
    assert bool((val == 7.0).all()) and bool((idx == 7).all())  # nothing was launched


def test_ties_at_the_kth_place(engine):
    """n = 640, ei, k = 256.  With the problem's incumbent the 256th score is positive but far below the bound test's
    absolute margin (PRUNE_EPS = 1e-9), so no candidate can be dropped.  With the incumbent raised by 6 fewer than 256
    candidates score above 0 and thousands tie at 0.0 on the 256th place (the oracle: 166 above, 4834 at 0): nothing
    is prunable, every staged candidate ties the incumbent, and the lowest indices win."""
    states, pr = fitted(engine, 640)
    Xs = t(U.candidates())
    for shift, tied in ((0.0, False), (6.0, True)):
        kw = objective(pr, best_f=pr["best_f"] + shift)
        sc, key = composition(engine, states, Xs, "ei", **kw)
        kth = np.sort(key)[::-1][255]
        print(f"best_f + {shift}: 256th score {kth!r}, shared by {int((key == kth).sum())} candidates")
        assert 0.0 <= kth < 1e-9
        if tied:
            assert kth == 0.0 and int((key == kth).sum()) > 1000
        got = topk(engine, 2, states, Xs, 256, "ei", **kw)
        check(engine, got, sc, key, 256)
        assert got[2][1] == M, got[2]


def test_duplicates_across_seed_and_staged_part(engine):
    states, pr = fitted(engine, 640)
    base = U.candidates()
    kw = objective(pr)
    i0 = int(topk(engine, 0, states, t(base), 1, "logei", **kw)[1][0])
    Xs = base.copy()
    spots = sorted({(i0 + 300) % 1024, 1024 + (i0 + 1500) % (M - 1024), 1024 + (i0 + 2900) % (M - 1024)} - {i0})
    assert len(spots) == 3
    for j in spots:
        Xs[j] = base[i0]
    sc, key = composition(engine, states, t(Xs), "logei", **kw)
    got = topk(engine, 2, states, t(Xs), 16, "logei", **kw)
    check(engine, got, sc, key, 16)
    assert got[1][:4].tolist() == sorted([i0] + spots) and len(set(got[0][:4].tolist())) == 1


def test_nan_candidates(engine):
    states, pr = fitted(engine, 640)
    kw = objective(pr)
    clean = topk(engine, 0, states, t(U.candidates()), 16, "logei", **kw)
    Xs = U.candidates().copy()
    taken = set(clean[1].tolist())
    bad = [next(j for j in range(2000, M) if j not in taken), next(j for j in range(5, 1024) if j not in taken)]
    Xs[bad] = np.nan  # one in the staged part, one in the seed block
    sc, key = composition(engine, states, t(Xs), "logei", **kw)
    got = topk(engine, 2, states, t(Xs), 16, "logei", **kw)
    check(engine, got, sc, key, 16)
    assert not set(bad) & set(got[1].tolist())
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])
    # every score NaN: gpx_topk_f64 ranks (and returns) a NaN as -inf, so the lowest indices come back
    off = 3 * 2 ** 20
    Xn = t(np.full_like(Xs, np.nan))
    scn, keyn = composition(engine, states, Xn, "logei", **kw)
    assert bool(torch.isnan(scn).all())
    for prune in (2, 0):
        gn = topk(engine, prune, states, Xn, 8, "logei", index_offset=off, **kw)
        check(engine, gn, scn, keyn, 8, offset=off)
        assert gn[1].tolist() == [off + j for j in range(8)]


def test_across_chunks(engine):
    """Padded n = 384, T = 2: a chunk holds 349 440 candidates; the top three are duplicated into the other chunk."""
    states, pr = fitted(engine, 384, 2)
    m, chunk = 400_000, 349_440
    Xs = U.candidates(m).copy()
    kw = objective(pr)
    top3 = topk(engine, 0, states, t(Xs), 3, "logei", **kw)[1].tolist()
    for q, i in enumerate(top3):
        j = 360_000 + 1000 * q if i < chunk else 1000 + 1000 * q
        assert j not in top3
        Xs[j] = Xs[i]
    Xg = t(Xs)
    sc, key = composition(engine, states, Xg, "logei", **kw)
    got = topk(engine, 2, states, Xg, 64, "logei", **kw)
    print(f"sweep_stats {got[2]}")
    check(engine, got, sc, key, 64)
    assert len(set(got[0][:6].tolist())) == 3 and got[2][2] < got[2][3]


def test_fallbacks(engine):
    """The fused small-n sweep (n = 200; the golden T = 8 problem, padded n = 256), an output with the fp32 covariance
    build and d > 16 compose the full multi-output sweep and the sort inside the call."""
    Xs = t(U.candidates())
    states, pr = fitted(engine, 200)
    kw = objective(pr)
    sc, key = composition(engine, states, Xs, "logei", **kw)
    got = topk(engine, 2, states, Xs, 16, "logei", index_offset=11, **kw)
    check(engine, got, sc, key, 16, offset=11)
    assert got[2] == (M, M, 0, 0)  # the fused path has no tiles
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synthetic_slm_n150_d5_T8.npz"))
    T8 = g["Y"].shape[1]
    kp = KernelParams("scale_linear_matern52", [float(v) for v in g["lengthscale"]], outputscale=float(g["outputscale"]),
                      noise=float(g["noise"]), const_mean=float(g["const_mean"]),
                      linear_variance=[float(v) for v in g["linear_variance"]])
    st8 = engine.fit_outputs(t(g["X"]), t(g["Y"]), [kp] * T8)
    assert T8 == 8 and engine.padded_n(st8[0].n) == 256
    kw8 = dict(best_f=float(g["Y"].mean(1).max()), beta=4.0, weights=[1.0 / T8] * T8)
    Xg = t(g["Xs"])
    for acq in ("logei", "variance"):
        sc8, key8 = composition(engine, st8, Xg, acq, **kw8)
        got8 = topk(engine, 2, st8, Xg, 16, acq, **kw8)
        check(engine, got8, sc8, key8, 16)
        assert got8[2] == (len(g["Xs"]), len(g["Xs"]), 0, 0)
    for cfg, d in ((dict(cov_fp32=(1,)), U.D), (dict(d=20), 20)):
        stc, prc = fitted(engine, 640, **cfg)
        Xc = t(U.candidates(M, d))
        kwc = objective(prc)
        for acq in ("logei", "ucb"):
            scc, keyc = composition(engine, stc, Xc, acq, **kwc)
            gotc = topk(engine, 2, stc, Xc, 16, acq, **kwc)
            check(engine, gotc, scc, keyc, 16)
            assert gotc[2][1] == M and gotc[2][2] == gotc[2][3] > 0


@pytest.mark.parametrize("acq,k,oracle_count", [("logei", 16, 279), ("ucb", 16, 131), ("ei", 1, 3)])
def test_pruning_engaged(engine, acq, k, oracle_count):
    """n = 640, T = 3, beta = 4.  The cap m / 2 keeps a silent fall-back to the full sweep from passing; it is a
    condition, not a performance figure.  Oracle: the incumbent after the seed block is the k-th best of the first 1024
    exact scores; the staged candidates whose bound from the first 128 rows of every output's L^-1 K* still reaches it
    are computed to the end (1024 + 599 of 5000 at most over n in {384, 640, 1000}, EI / LogEI / UCB, k <= 16)."""
    n = 640
    unprunable = U.oracle_survivors(n, acq, k)
    print(f"oracle ({acq}, k = {k}): {unprunable} staged candidates reach the incumbent after the head rows "
          f"({1024 + unprunable} computed to the end)")
    assert abs(unprunable - oracle_count) <= 2
    states, pr = fitted(engine, n)
    Xs = t(U.candidates())
    kw = objective(pr)
    sc, key = composition(engine, states, Xs, acq, **kw)
    got = topk(engine, 2, states, Xs, k, acq, **kw)
    check(engine, got, sc, key, k)
    print(f"sweep_stats {got[2]}")
    assert got[2][1] <= M / 2
    assert got[2][2] < got[2][3]


def test_dropin_default_analytic_sweep(engine, tmp_path, monkeypatch):
    """The drop-in's default configuration (independent outputs): BayesianOptimizer._analytic_sweep(k) takes
    acquire_topk_multi once and returns the points the composition (sweep_objective with scores + topk) returns.
    The drop-in models independent outputs only together with the hyperparameter fit (with fixed hyperparameters the
    outputs share one factor, test_dropin_shared_factor_analytic_sweep), so the fit stays on, as by default, with a
    few L-BFGS iterations."""
    from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
    from tests.stubs import BOUNDS, StubSimulator

    cfg = GPConfig(raw_samples=4096, mll_options={"maxiter": 4})
    assert cfg.fit_hyperparameters and cfg.independent_outputs
    opt = BayesianOptimizer(StubSimulator(), BOUNDS, str(tmp_path), n_initial_points=300, n_batches=0, batch_size=8,
                            target_total=300, engine=engine, seed=5, gp_config=cfg, acquisition="logei")
    opt.optimize()
    opt.fit_gp_model()
    gp = opt.gp_model
    assert gp.independent and engine.padded_n(gp.states[0].n) >= 384
    grid = opt._sobol_grid(4096)
    monkeypatch.setattr(opt, "_sobol_grid", lambda n: grid[:n])
    calls = []
    real = engine.acquire_topk_multi
    monkeypatch.setattr(engine, "acquire_topk_multi", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    got = opt._analytic_sweep(8)
    assert calls == [1]
    w = opt._acq_weights()
    gt = opt._tensor(grid)
    _, _, score = gp.sweep_objective(opt.x_tf(gt), "logei", w.tolist(), best_f=opt._incumbent(w),
                                     beta=opt.config.beta, return_scores=True)
    _, order = engine.topk(score, 8)
    assert torch.equal(got, gt[order.to(gt.device)])
