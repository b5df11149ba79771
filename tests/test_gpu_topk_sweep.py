"""The pruned top-k sweep (gpx_acquire_topk_f64) against the composition it replaces.

The yardstick everywhere is int64-equal values and equal indices against ``acquire(return_scores=True)`` followed by
``engine.topk`` on the same handle, and a second check against a numpy stable sort of those scores' keys (gpx_topk_f64
sorts the key NaN -> -inf, -0 -> +0 and returns it).  Fits and candidates are those of tests/test_gpu_sweep_prune.py:
padded n = 384 (three row tiles), 640, 1024 from n = 1000, d = 4, m = 5000 (a 1024-candidate seed block, then 3976 staged
candidates with a partial last tile).
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from bayesianoptimizer_amd import KernelParams, _capi, botorch_default_lengthscale
from bayesianoptimizer_amd._capi import GPXError
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KINDS = ["rbf", "matern52", "scale_linear_matern52"]
ACQS = ["ei", "logei", "ucb", "variance"]
OACQ = {"ei": O.ACQ_EI, "logei": O.ACQ_LOGEI, "ucb": O.ACQ_UCB, "variance": O.ACQ_VARIANCE}
D, M = 4, 5000
_fits = {}
_cands = {}


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def fitted(engine, n, kind="rbf", d=D, cov_fp32=False):
    """One fit per configuration for the whole module; never modified."""
    key = (n, kind, d, cov_fp32)
    if key not in _fits:
        X, y = O.synthetic_problem(n, d, 21)
        kp = KernelParams(kind, botorch_default_lengthscale(d), linear_variance=0.3, noise=1e-4, cov_fp32=cov_fp32)
        _fits[key] = (engine.fit(t(X), t(y), kp), X, y)
    return _fits[key]


def candidates(m=M, d=D):
    if (m, d) not in _cands:
        _cands[(m, d)] = O.sobol_candidates(m, d, 22)
    return _cands[(m, d)]


def bits(v):
    return v.view(torch.int64).cpu().numpy()


def topk(engine, prune, st, Xs, k, acq, **kw):
    """(value bits, indices, sweep_stats) of one acquire_topk call with sweep_prune = prune, restored afterwards."""
    before = engine.get_option("sweep_prune")
    engine.set_option("sweep_prune", prune)
    try:
        v, i = engine.acquire_topk(st, Xs, k, acq, **kw)
        stats = engine.sweep_stats()
    finally:
        engine.set_option("sweep_prune", before)
    assert v.shape == (k,) and i.shape == (k,) and v.dtype == torch.float64 and i.dtype == torch.int64
    return bits(v), i.cpu().numpy(), stats


def composition(engine, st, Xs, acq, **kw):
    """The scores of the full sweep (a device tensor) and their numpy key (NaN -> -inf, -0 -> +0)."""
    _, _, sc = engine.acquire(st, Xs, acq, return_scores=True, **kw)
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
@pytest.mark.parametrize("acq", ACQS)
@pytest.mark.parametrize("kind", KINDS)
def test_equal_bits(engine, kind, acq, n):
    st, _, y = fitted(engine, n, kind)
    Xs = t(candidates())
    kw = dict(best_f=float(y.max()), beta=4.0)
    sc, key = composition(engine, st, Xs, acq, **kw)
    for k in (1, 16, 300):
        for prune in (2, 0):
            got = topk(engine, prune, st, Xs, k, acq, **kw)
            check(engine, got, sc, key, k)
            assert got[2][0] == M and got[2][3] > 0
            if prune == 0:
                assert got[2][1] == M and got[2][2] == got[2][3]


@pytest.mark.parametrize("acq", ACQS)
@pytest.mark.parametrize("n,kind", [(384, "rbf"), (640, "matern52"), (1000, "scale_linear_matern52")])
def test_k1_is_the_argmax_call(engine, n, kind, acq):
    """Same (value, index) bits and the same counters: with k = 1 the pool's incumbent takes the values the argmax
    form's atomicMax gives it, and no bound pass runs inside a scoring launch."""
    st, _, y = fitted(engine, n, kind)
    Xs = t(candidates())
    kw = dict(best_f=float(y.max()), beta=4.0)
    engine.set_option("sweep_prune", 2)
    try:
        bv, bi = engine.acquire(st, Xs, acq, **kw)
        ref_stats = engine.sweep_stats()
    finally:
        engine.set_option("sweep_prune", 1)
    got = topk(engine, 2, st, Xs, 1, acq, **kw)
    assert got[0][0] == int(bv.view(torch.int64).item()) and got[1][0] == int(bi.item())
    assert got[2] == ref_stats, (got[2], ref_stats)


def test_limits(engine):
    st, _, y = fitted(engine, 640, "rbf")
    kw = dict(best_f=float(y.max()))
    Xs = t(candidates())
    sc, key = composition(engine, st, Xs, "logei", **kw)
    check(engine, topk(engine, 2, st, Xs, 1024, "logei", **kw), sc, key, 1024)
    # below the seed block: no staged columns, the whole set comes back sorted
    Xs7 = t(candidates()[:700])
    sc7, key7 = composition(engine, st, Xs7, "logei", **kw)
    got = topk(engine, 2, st, Xs7, 700, "logei", **kw)
    check(engine, got, sc7, key7, 700)
    assert sorted(got[1].tolist()) == list(range(700)) and got[2][1] == 700
    for Xq, k in [(Xs, 1025), (Xs7, 701), (Xs, 0)]:
        with pytest.raises(GPXError) as e:
            engine.acquire_topk(st, Xq, k, "logei", **kw)
        assert e.value.status == _capi.GPX_INVALID_ARG
    # the entry point itself, with a workspace that is large enough for any legal k
    nbytes = ctypes.c_size_t()
    assert engine.lib.gpx_acquire_topk_workspace_size(st.n, M, 1024, ctypes.byref(nbytes)) == _capi.GPX_OK
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    val = torch.full((1100,), 7.0, dtype=torch.float64, device=DEV)
    idx = torch.full((1100,), 7, dtype=torch.int64, device=DEV)
    ap = _capi.AcqParamsC()
    ap.kind, ap.best_f, ap.beta, ap.y_mean, ap.y_scale = 1, kw["best_f"], 4.0, 0.0, 1.0
    pc = st.params.to_c(st.d)
    vp = ctypes.c_void_p
    for m, k in [(M, 1025), (700, 701), (M, 0), (M, -1)]:
        rc = engine.lib.gpx_acquire_topk_f64(
            engine.handle, ctypes.byref(pc), st.n, vp(st.X.data_ptr()), st.X.stride(0), vp(st.W.data_ptr()),
            st.W.stride(0), vp(st.alpha[:, 0].contiguous().data_ptr()), vp(Xs.data_ptr()), m, Xs.stride(0),
            ctypes.byref(ap), 0, k, vp(val.data_ptr()), vp(idx.data_ptr()), vp(ws.data_ptr()), ws.numel())
        assert rc == _capi.GPX_INVALID_ARG, (m, k)
    torch.cuda.synchronize()
    assert bool((val == 7.0).all()) and bool((idx == 7).all())  # nothing was launched


def test_ties_at_the_kth_place(engine):
    """RBF, n = 640, ei, k = 256: the 256th score is 0.0 and thousands of candidates share it.  Nothing is prunable
    (the test is strict), every staged candidate ties the incumbent, and the lowest indices win."""
    st, X, y = fitted(engine, 640, "rbf")
    Xs = candidates()
    kw = dict(best_f=float(y.max()))
    sc, key = composition(engine, st, t(Xs), "ei", **kw)
    kth = np.sort(key)[::-1][255]
    print(f"256th score {kth!r}, shared by {int((key == kth).sum())} candidates")
    assert kth == 0.0 and int((key == kth).sum()) > 1000
    got = topk(engine, 2, st, t(Xs), 256, "ei", **kw)
    check(engine, got, sc, key, 256)
    assert got[2][1] == M, got[2]


def test_duplicates_across_seed_and_staged_part(engine):
    st, _, y = fitted(engine, 640, "matern52")
    base = candidates()
    kw = dict(best_f=float(y.max()))
    i0 = int(topk(engine, 0, st, t(base), 1, "logei", **kw)[1][0])
    Xs = base.copy()
    spots = sorted({(i0 + 300) % 1024, 1024 + (i0 + 1500) % (M - 1024), 1024 + (i0 + 2900) % (M - 1024)} - {i0})
    assert len(spots) == 3
    for j in spots:
        Xs[j] = base[i0]
    sc, key = composition(engine, st, t(Xs), "logei", **kw)
    got = topk(engine, 2, st, t(Xs), 16, "logei", **kw)
    check(engine, got, sc, key, 16)
    assert got[1][:4].tolist() == sorted([i0] + spots) and len(set(got[0][:4].tolist())) == 1


def test_nan_candidates(engine):
    st, _, y = fitted(engine, 640, "rbf")
    kw = dict(best_f=float(y.max()))
    clean = topk(engine, 0, st, t(candidates()), 16, "logei", **kw)
    Xs = candidates().copy()
    taken = set(clean[1].tolist())
    bad = [next(j for j in range(2000, M) if j not in taken), next(j for j in range(5, 1024) if j not in taken)]
    Xs[bad] = np.nan  # one in the staged part, one in the seed block
    sc, key = composition(engine, st, t(Xs), "logei", **kw)
    got = topk(engine, 2, st, t(Xs), 16, "logei", **kw)
    check(engine, got, sc, key, 16)
    assert not set(bad) & set(got[1].tolist())
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])
    # every score NaN: gpx_topk_f64 ranks (and returns) a NaN as -inf, so the lowest indices come back
    off = 3 * 2 ** 20
    Xn = t(np.full_like(Xs, np.nan))
    scn, keyn = composition(engine, st, Xn, "logei", **kw)
    assert bool(torch.isnan(scn).all())
    for prune in (2, 0):
        gn = topk(engine, prune, st, Xn, 8, "logei", index_offset=off, **kw)
        check(engine, gn, scn, keyn, 8, offset=off)
        assert gn[1].tolist() == [off + j for j in range(8)]


def test_across_chunks_and_super_chunks(engine):
    """Padded n = 384: a chunk holds 349 440 candidates; the top three are duplicated into the other chunk."""
    st, _, y = fitted(engine, 384, "rbf")
    m, chunk = 400_000, 349_440
    Xs = candidates(m).copy()
    kw = dict(best_f=float(y.max()))
    top3 = topk(engine, 0, st, t(Xs), 3, "logei", **kw)[1].tolist()
    for q, i in enumerate(top3):
        j = 360_000 + 1000 * q if i < chunk else 1000 + 1000 * q
        assert j not in top3
        Xs[j] = Xs[i]
    Xg = t(Xs)
    sc, key = composition(engine, st, Xg, "logei", **kw)
    got = topk(engine, 2, st, Xg, 64, "logei", **kw)
    check(engine, got, sc, key, 64)
    assert len(set(got[0][:6].tolist())) == 3 and got[2][2] < got[2][3]


@pytest.mark.parametrize("d,cov_fp32", [(20, False), (4, True)])
def test_chunked_form(engine, d, cov_fp32):
    """d > 16 and the fp32 covariance build keep the chunked (non-lazy) pruned sweep."""
    st, _, y = fitted(engine, 640, "rbf", d=d, cov_fp32=cov_fp32)
    Xs = t(candidates(M, d))
    for acq in ("logei", "ucb"):
        kw = dict(best_f=float(y.max()), beta=4.0)
        sc, key = composition(engine, st, Xs, acq, **kw)
        check(engine, topk(engine, 2, st, Xs, 16, acq, **kw), sc, key, 16)


@pytest.mark.parametrize("acq", ACQS)
def test_call_options(engine, acq):
    st, _, y = fitted(engine, 640, "matern52")
    Xs = t(candidates())
    off = 7 * 2 ** 20
    kw = dict(best_f=0.3 + 1.7 * float(y.max()), beta=4.0, y_mean=0.3, y_scale=1.7, index_offset=off)
    sc, key = composition(engine, st, Xs, acq, **kw)
    first = topk(engine, 2, st, Xs, 16, acq, **kw)
    check(engine, first, sc, key, 16, offset=off)
    again = topk(engine, 2, st, Xs, 16, acq, **kw)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        on_stream = topk(engine, 2, st, Xs, 16, acq, **kw)
    stream.synchronize()
    assert np.array_equal(first[0], on_stream[0]) and np.array_equal(first[1], on_stream[1])


def test_fallbacks(engine):
    """n = 200 (the fused small-n sweep) and sweep_prune = 0 compose the full sweep and the sort inside the call."""
    st, _, y = fitted(engine, 200, "rbf")
    Xs = t(candidates())
    kw = dict(best_f=float(y.max()))
    sc, key = composition(engine, st, Xs, "logei", **kw)
    got = topk(engine, 1, st, Xs, 16, "logei", index_offset=11, **kw)
    check(engine, got, sc, key, 16, offset=11)
    assert got[2] == (M, M, 0, 0)  # the fused path has no tiles
    st6, _, y6 = fitted(engine, 640, "rbf")
    sc6, key6 = composition(engine, st6, Xs, "logei", best_f=float(y6.max()))
    got6 = topk(engine, 0, st6, Xs, 16, "logei", best_f=float(y6.max()))
    check(engine, got6, sc6, key6, 16)
    assert got6[2][1] == M and got6[2][2] == got6[2][3] > 0


@pytest.mark.parametrize("acq,oracle_count", [("ucb", 59), ("logei", 120)])
def test_pruning_engaged(engine, acq, oracle_count):
    """RBF, n = 640, beta = 4, k = 16.  The cap m / 4 keeps a silent fall-back to the full sweep from passing; it is a
    condition, not a performance figure.  Oracle: the incumbent after the seed block is the 16th best of the first 1024
    exact scores; the staged candidates whose bound after 512 rows of V still reaches it are computed to the end."""
    n, k = 640, 16
    st, X, y = fitted(engine, n, "rbf")
    Xs = candidates()
    best_f = float(y.max())
    ost = O.fit(X, y, O.KernelParams(O.RBF, np.full(D, botorch_default_lengthscale(D)), noise=1e-4))
    Ks = O.kernel_matrix(X, Xs, ost.params)
    mu = ost.params.const_mean + Ks.T @ ost.alpha
    V = sla.solve_triangular(ost.L, Ks, lower=True, check_finite=False)
    kd = O.kernel_diag(Xs, ost.params)
    exact = O.acquisition(mu, np.maximum(kd - np.einsum("ij,ij->j", V, V), 1e-10), OACQ[acq], best_f, 4.0)
    ub = O.acquisition(mu, np.maximum(kd - np.einsum("ij,ij->j", V[:512], V[:512]), 1e-10), OACQ[acq], best_f, 4.0)
    tau = np.sort(exact[:1024])[::-1][k - 1]
    unprunable = int((ub[1024:] >= tau).sum())
    print(f"oracle ({acq}): {unprunable} staged candidates reach the 16th best seed score after 512 rows "
          f"({1024 + unprunable} computed to the end)")
    assert abs(unprunable - oracle_count) <= 2 and 1024 + unprunable <= M / 4
    kw = dict(best_f=best_f, beta=4.0)
    sc, key = composition(engine, st, t(Xs), acq, **kw)
    got = topk(engine, 2, st, t(Xs), k, acq, **kw)
    check(engine, got, sc, key, k)
    print(f"sweep_stats {got[2]}")
    assert got[2][1] <= M / 4
    assert got[2][2] < got[2][3]


def test_dropin_shared_factor_analytic_sweep(engine, tmp_path, monkeypatch):
    """independent_outputs=False: BayesianOptimizer._analytic_sweep(k) takes acquire_topk and returns the points the
    composition (sweep_objective with scores + topk) returns."""
    from bayesianoptimizer_amd.optimizer import BayesianOptimizer, GPConfig
    from tests.stubs import BOUNDS, StubSimulator

    cfg = GPConfig(fit_hyperparameters=False, independent_outputs=False, raw_samples=4096)
    opt = BayesianOptimizer(StubSimulator(), BOUNDS, str(tmp_path), n_initial_points=300, n_batches=0, batch_size=8,
                            target_total=300, engine=engine, seed=5, gp_config=cfg, acquisition="logei")
    opt.optimize()
    opt.fit_gp_model()
    gp = opt.gp_model
    assert not gp.independent and engine.padded_n(gp.state.n) >= 384
    grid = opt._sobol_grid(4096)
    monkeypatch.setattr(opt, "_sobol_grid", lambda n: grid[:n])
    calls = []
    real = engine.acquire_topk
    monkeypatch.setattr(engine, "acquire_topk", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    got = opt._analytic_sweep(8)
    assert calls == [1]
    w = opt._acq_weights()
    gt = opt._tensor(grid)
    _, _, score = gp.sweep_objective(opt.x_tf(gt), "logei", w.tolist(), best_f=opt._incumbent(w),
                                     beta=opt.config.beta, return_scores=True)
    _, order = engine.topk(score, 8)
    assert torch.equal(got, gt[order.to(gt.device)])
