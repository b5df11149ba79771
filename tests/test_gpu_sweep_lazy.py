"""The lazy form of the pruned sweep: K* head rows for every candidate, full-height columns rebuilt from a
survivor list for the tail.

Two yardsticks, both bit identity.  (1) gpx_debug_kstar_f64: a column the gather build writes has the bytes of the column
the full-store build writes.  (2) (best_val, best_idx) with sweep_prune = 2 against 0, plus the sweep_stats identities
([0] = m, [3] equal in both modes).  Shapes: padded n = 384 and 640 are the smallest with 3 and 5 row tiles; their
chunks (the tail buffer's capacity) hold 349 440 and 209 664 columns; a call's first super-chunk is one chunk long,
the later ones hold 2^20 candidates.
"""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import GPEngine, KernelParams, botorch_default_lengthscale, _capi
from bayesianoptimizer_amd.engine import ACQ_KINDS
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KINDS = ["rbf", "matern52", "scale_linear_matern52"]
SUPER = 1 << 20
CHUNK = {384: 349_440, 640: 209_664}
_fits = {}
_cands = {}


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def fitted(engine, n, kind="rbf", d=4, cov_fp32=False):
    """One fit per configuration for the whole module; never modified."""
    key = (n, kind, d, cov_fp32)
    if key not in _fits:
        X, y = O.synthetic_problem(n, d, 21)
        kp = KernelParams(kind, botorch_default_lengthscale(d), linear_variance=0.3, noise=1e-4, cov_fp32=cov_fp32)
        _fits[key] = (engine.fit(t(X), t(y), kp), X, y)
    return _fits[key]


def candidates(m, d=4):
    if (m, d) not in _cands:
        _cands[(m, d)] = O.sobol_candidates(m, d, 22)
    return _cands[(m, d)]


def acquire(engine, prune, st, Xs, acq="logei", **kw):
    before = engine.get_option("sweep_prune")
    engine.set_option("sweep_prune", prune)
    try:
        bv, bi = engine.acquire(st, Xs, acq, **kw)
        stats = engine.sweep_stats()
    finally:
        engine.set_option("sweep_prune", before)
    return int(bv.view(torch.int64).item()), int(bi.item()), stats


def both(engine, st, Xs, acq="logei", **kw):
    full = acquire(engine, 0, st, Xs, acq, **kw)
    pruned = acquire(engine, 2, st, Xs, acq, **kw)
    print(f"sweep_stats pruned {pruned[2]} full {full[2]}")
    assert pruned[:2] == full[:2], (pruned, full)
    m = Xs.shape[0]
    assert full[2][0] == m and full[2][1] == m and full[2][2] == full[2][3] > 0
    assert pruned[2][0] == m and pruned[2][3] == full[2][3]
    return full, pruned


# ---- (1) recomputed columns have the bits of the full build ---------------------------------------------------------
def debug_kstar(engine, kp, X, Xs, m, list_=None, count=None):
    lib, n, d = engine.lib, X.shape[0], X.shape[1]
    npad = int(lib.gpx_padded_n(n))
    ld = (m + 255) // 256 * 256
    out = torch.full((npad, ld), float("nan"), dtype=torch.float64, device=DEV)
    nbytes = ctypes.c_size_t()
    assert lib.gpx_debug_kstar_workspace_size(n, ld, ctypes.byref(nbytes)) == _capi.GPX_OK
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    pc = kp.to_c(d)
    ptr = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None
    st = lib.gpx_debug_kstar_f64(engine.handle, ctypes.byref(pc), n, ptr(X), X.stride(0), ptr(Xs), m, Xs.stride(0),
                                 ptr(list_), ptr(count), ptr(out), ld, ptr(ws), ws.numel())
    _capi.check(st, engine.handle)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("d", [4, 8, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_gather_build_has_the_bits_of_the_full_build(engine, kind, d):
    n, m, cap, cnt = 300, 3000, 1500, 1061  # padded n = 384 (84 padded rows); the count is no multiple of 128
    rng = np.random.default_rng(5 + d)
    X, _ = O.synthetic_problem(n, d, 21)
    Xs = rng.random((m, d))
    kp = KernelParams(kind, list(0.3 + rng.random(d)), outputscale=1.3, linear_variance=list(0.1 + rng.random(d)))
    idx = rng.permutation(m)[:cap].astype(np.int32)
    idx[10:40] = idx[100:130]  # repeats
    idx[500] = idx[499]
    idx[cnt - 1] = m - 1
    Xd, Xsd = t(X), t(Xs)
    full = debug_kstar(engine, kp, Xd, Xsd, m)
    lst = torch.tensor(idx, dtype=torch.int32, device=DEV)
    count = torch.tensor([cnt], dtype=torch.int32, device=DEV)
    got = debug_kstar(engine, kp, Xd, Xsd, cap, lst, count)
    full_i, got_i = full.view(torch.int64), got.view(torch.int64)
    want = full_i[:, torch.tensor(idx[:cnt].astype(np.int64), device=DEV)]
    assert torch.equal(got_i[:, :cnt], want)
    assert torch.all(full[n:, :m] == 0) and not torch.isnan(full[:, :m]).any()
    # zero up to the end of the last 128-column tile (the product reads whole tiles)
    assert torch.all(got[:, cnt:(cnt + 127) // 128 * 128] == 0)
    # a count of zero writes nothing
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert torch.isnan(debug_kstar(engine, kp, Xd, Xsd, cap, lst, zero)).all()


# ---- (2) equal bits of the argmax --------------------------------------------------------------------------------
def test_two_super_chunks_winner_in_both_and_in_the_second_only(engine):
    """(a) m = 2^20 + 5000 at padded n = 384.  The call's first super-chunk is one chunk long, so the call splits into
    [0, 349 440) and [349 440, m): the winner and its copy sit on opposite sides of that boundary."""
    st, _, y = fitted(engine, 384)
    m, C = SUPER + 5000, CHUNK[384]
    base = candidates(m)
    kw = dict(best_f=float(y.max()))
    i0 = acquire(engine, 0, st, t(base), **kw)[1]
    lo, hi = (i0, C + 1234) if i0 < C else (200_000, i0)
    assert 1024 <= lo < C <= hi < m and lo + 1 != hi
    Xs = base.copy()
    Xs[lo] = Xs[hi] = base[i0]  # the winner in both super-chunks: the lowest index wins
    full, pruned = both(engine, st, t(Xs), **kw)
    assert full[1] == lo
    assert pruned[2][2] < pruned[2][3]
    Xs[lo] = base[lo + 1]  # the winner only in the second super-chunk
    full2, _ = both(engine, st, t(Xs), **kw)
    assert full2[1] == hi and full2[0] == full[0]


def test_three_super_chunks_reach_the_cap(engine):
    """m > C + 2^20 at padded n = 384: a chunk-long first super-chunk, one of the 2^20 cap and a third; the winner only
    in the third, then also in the second, then also in the first."""
    st, _, y = fitted(engine, 384)
    C = CHUNK[384]
    m = C + SUPER + 3000
    base = candidates(m)
    kw = dict(best_f=float(y.max()))
    i0 = acquire(engine, 0, st, t(base), **kw)[1]
    Xs = base.copy()
    Xs[i0] = base[i0 + 1 if i0 + 1 < m else i0 - 1]
    expect = None
    for k in (C + SUPER + 1500, C + 700_000, 100_000):
        assert k != i0
        Xs[k] = base[i0]
        full, pruned = both(engine, st, t(Xs), **kw)
        assert full[1] == k and (expect is None or full[0] == expect)
        expect = full[0]
        assert pruned[2][2] < pruned[2][3]


@pytest.mark.parametrize("extra", [0, 1024])
def test_tail_overflow_identical_candidates(engine, extra):
    """(b) nothing prunable: every candidate after the seed block survives the first tile, so the tail takes more rounds
    than one (two with the issue's m, the seed block taking 1024 of it; three with 1024 more), the last one partial."""
    st, _, y = fitted(engine, 640)
    m = 2 * CHUNK[640] + 300 + extra
    Xs = t(np.repeat(candidates(5000)[17:18], m, axis=0))
    full, pruned = both(engine, st, Xs, best_f=float(y.max()), index_offset=11)
    assert full[1] == 11
    assert pruned[2][1] == m and pruned[2][2] == pruned[2][3]


def test_block_of_copies_of_the_best_larger_than_the_tail(engine):
    """(c) a prunable Sobol set with more than one tail capacity of copies of its best candidate in the middle."""
    st, _, y = fitted(engine, 640)
    base = candidates(150_000)
    kw = dict(best_f=float(y.max()))
    i0 = acquire(engine, 0, st, t(base), **kw)[1]
    ncopy = CHUNK[640] + 1000
    for start in (100_000, 20_000):  # the block after / before a late original
        Xs = np.concatenate([base[:start], np.repeat(base[i0:i0 + 1], ncopy, axis=0), base[start:]])
        where = i0 if i0 < start else i0 + ncopy
        full, pruned = both(engine, st, t(Xs), **kw)
        assert full[1] == min(where, start)
        assert pruned[2][1] >= ncopy and pruned[2][2] < pruned[2][3]


def test_nan_candidates_among_the_survivors_and_all_nan(engine):
    """(d) a NaN bound survives every stage: NaN candidates reach the tail and never win."""
    st, _, y = fitted(engine, 640)
    kw = dict(best_f=float(y.max()))
    base = candidates(5000)
    clean = acquire(engine, 0, st, t(base), **kw)
    Xs = base.copy()
    bad = [i for i in (7, 1500, 1501, 2999, 4999) if i != clean[1]]
    Xs[bad] = np.nan
    full, pruned = both(engine, st, t(Xs), **kw)
    assert full[:2] == clean[:2]
    assert pruned[2][1] >= len(bad) - 1  # (index 7 lies in the seed block)
    both(engine, st, t(np.full_like(Xs, np.nan)), **kw)


@pytest.mark.parametrize("n", [300, 1000])
@pytest.mark.parametrize("acq", ["ei", "logei", "ucb", "variance"])
def test_offset_standardize_stream(engine, acq, n):
    """(e) n no multiple of the tile, index_offset, y standardisation and a non-default stream in one case."""
    st, _, y = fitted(engine, n, "matern52")
    Xs = t(candidates(5000))
    off = 7 * 2 ** 20
    kw = dict(best_f=0.3 + 1.7 * float(y.max()), beta=4.0, y_mean=0.3, y_scale=1.7, index_offset=off)
    _, bi, sc = engine.acquire(st, Xs, acq, return_scores=True, **kw)
    sg = sc.cpu().numpy()
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        full, _ = both(engine, st, Xs, acq, **kw)
    stream.synchronize()
    assert full[1] == off + int(np.flatnonzero(sg == sg.max())[0]) == int(bi.item())


def test_same_call_twice_same_bits(engine):
    """(f) the slot order of the survivor lists may vary from run to run; the result may not."""
    st, _, y = fitted(engine, 640, "scale_linear_matern52")
    Xs = t(candidates(150_000))
    kw = dict(best_f=float(y.max()))
    a = acquire(engine, 2, st, Xs, **kw)
    b = acquire(engine, 2, st, Xs, **kw)
    assert a == b
    assert a[:2] == acquire(engine, 0, st, Xs, **kw)[:2]


@pytest.mark.parametrize("d,cov_fp32", [(16, True), (20, False)])
def test_difference_form_configurations_keep_the_chunked_pruned_path(engine, d, cov_fp32):
    """(g) the fp32 covariance build and d > 16 (kstar_kernel) are not converted: bit-exact as before."""
    st, _, y = fitted(engine, 384, "matern52", d=d, cov_fp32=cov_fp32)
    full, pruned = both(engine, st, t(candidates(5000, d)), best_f=float(y.max()))


def test_workspace_of_exactly_the_reported_size(engine):
    """(h) through the C ABI with a buffer of gpx_sweep_workspace_size bytes, filled with NaN bytes."""
    st, _, y = fitted(engine, 640)
    m = 150_000
    Xs = t(candidates(m))
    lib = engine.lib
    nbytes = ctypes.c_size_t()
    assert lib.gpx_sweep_workspace_size(st.n, 1, m, ctypes.byref(nbytes)) == _capi.GPX_OK
    want = acquire(engine, 0, st, Xs, best_f=float(y.max()))
    ws = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device=DEV)
    ap = _capi.AcqParamsC()
    ap.kind, ap.best_f, ap.beta, ap.y_mean, ap.y_scale = ACQ_KINDS["logei"], float(y.max()), 4.0, 0.0, 1.0
    bv = torch.empty(1, dtype=torch.float64, device=DEV)
    bi = torch.empty(1, dtype=torch.int64, device=DEV)
    engine.inverse(st)
    pc = st.params.to_c(st.X.shape[1])
    alpha = st.alpha[:, 0].contiguous()
    ptr = lambda a: ctypes.c_void_p(a.data_ptr())
    engine.set_option("sweep_prune", 2)
    try:
        torch.cuda.synchronize()
        for size, ok in ((nbytes.value - 1, False), (nbytes.value, True)):
            status = lib.gpx_acquire_argmax_f64(engine.handle, ctypes.byref(pc), st.n, ptr(st.X), st.X.stride(0),
                                                ptr(st.W), st.W.stride(0), ptr(alpha), ptr(Xs), m, Xs.stride(0),
                                                ctypes.byref(ap), 0, ptr(bv), ptr(bi), None, ptr(ws), size)
            assert (status == _capi.GPX_OK) == ok
        torch.cuda.synchronize()
    finally:
        engine.set_option("sweep_prune", 1)
    assert (int(bv.view(torch.int64).item()), int(bi.item())) == want[:2]


@pytest.mark.parametrize("offset", [0, 8])
@pytest.mark.parametrize("call", ["topk", "multi", "posterior", "posterior_fused"])
def test_workspace_of_exactly_the_reported_size_every_sweep_call(engine, monkeypatch, call, offset):
    """(h) for the other calls that carve the sweep's layout: gpx_acquire_topk_f64 (k = 5), gpx_acquire_argmax_multi_f64
    (T = 2) and gpx_posterior_f64 (nrhs = 3; also the fused n = 200), each through the engine's own call with its
    workspace replaced by exactly the reported bytes of 0xFF, 256-aligned or 8 bytes into the allocation, a 4 KiB guard
    of 0xFF behind them.  Padded n = 384: three row tiles, the smallest pruned size.  One byte less is rejected; the
    results have the bits of the engine's call with its own workspace; the guard is intact."""
    n, d, m, guard = (200 if call == "posterior_fused" else 384), 3, 3000, 4096
    X, y = O.synthetic_problem(n, d, 21)
    Y = np.stack([y, np.sin(3 * X).sum(1), np.cos(2 * X).sum(1)], 1)
    kp = KernelParams("rbf", botorch_default_lengthscale(d), noise=1e-4)
    Xs = t(candidates(m, d))
    lib, nbytes = engine.lib, ctypes.c_size_t()
    if call == "topk":
        st = engine.fit(t(X), t(y), kp)
        assert lib.gpx_acquire_topk_workspace_size(n, m, 5, ctypes.byref(nbytes)) == _capi.GPX_OK
        run = lambda: engine.acquire_topk(st, Xs, 5, best_f=float(y.max()))
    elif call == "multi":
        sts = engine.fit_outputs(t(X), t(Y[:, :2]), [kp, kp.replace(outputscale=1.5)])
        assert lib.gpx_sweep_multi_workspace_size(n, m, ctypes.byref(nbytes)) == _capi.GPX_OK
        run = lambda: engine.acquire_multi(sts, Xs, "ucb", weights=[0.5, 1.0])
    else:
        st = engine.fit(t(X), t(Y), kp)
        assert lib.gpx_sweep_workspace_size(n, 3, m, ctypes.byref(nbytes)) == _capi.GPX_OK
        run = lambda: engine.posterior(st, Xs)
    nb = nbytes.value
    want = [a.clone() for a in run()]
    big = torch.empty(offset + nb + guard, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 256 == 0
    asked = []
    for size in (nb - 1, nb):
        big.fill_(0xFF)
        monkeypatch.setattr(engine, "workspace", lambda key, need: (asked.append(need), big[offset:offset + size])[1])
        if size < nb:
            with pytest.raises(_capi.GPXError, match="workspace too small"):
                run()
        else:
            got = run()
    torch.cuda.synchronize()
    assert asked == [nb, nb]  # the engine asks for what the size function reports, and passes on what it is given
    assert bool((big[:offset] == 0xFF).all()) and bool((big[offset + nb:] == 0xFF).all())
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_pruning_engaged_on_the_lazy_path(engine):
    """The n = 640 problem of test_gpu_sweep_prune.test_pruning_engaged, where the oracle rules out over 90 % of the
    candidates after the first row tile: at most a quarter may reach the last tile, and fewer tiles run than in full."""
    st, _, y = fitted(engine, 640)
    m = 5000
    full, pruned = both(engine, st, t(candidates(m)), best_f=float(y.max()))
    assert pruned[2][1] <= m / 4
    assert pruned[2][2] < pruned[2][3]
