"""The mean-first order of the lazy pruned sweep's seeded spans (sweep_order = 1): the columns are ranked and
pruned on the mean's bound with the prior variance, and the head (K* rows 0 .. 127, row tile 0 of the product) runs only
over the columns that pass, through the list-driven instance of head_product_kernel.

Yardstick: bit identity of (best_val, best_idx) and of every top-k pair against sweep_prune = 0, under sweep_order 1 and
0, plus the sweep_stats conditions named at each test.  Shapes: the smallest at which the seeded order runs, those of
tests/test_gpu_sweep_seed.py: padded n = 384 with m = 400 000 (chunk 349 440) and padded n = 640 with m = 250 000 (chunk
209 664); d = 4 (the mean bound's fp64 factorised form) and d = 8 (its fp32 form); one fit per shape for the module.

sweep_stats[2] (product tiles, the head's included) of the logei RBF calls with scalar lengthscales, order 1 / order 0,
read on an MI355X with this file's inputs:
    d = 4: padded n = 384: 33 / 3141;   padded n = 640: 185 / 1986
    d = 8: padded n = 384: 24 / 3141;   padded n = 640: 40 / 1986
UCB and the variance acquisition keep the parent's order under either value (the RBF prior variance is one constant, so
the mean-first bound ranks by the mean alone and gave them a weaker seed: 3422 against 3182 tiles for UCB at padded
n = 384, d = 4), and so does the top-k form above k = 64 (its incumbent is the k-th best of the seed's 1024 scores).
"""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import KernelParams, botorch_default_lengthscale, _capi
from oracle import gp_oracle as O
from tests import ard_util
from tests.abi_util import GuardedWorkspace
from tests.test_gpu_sweep_headfused import KINDS, bits, candidates as head_candidates, case, head_product, ptr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ACQS = ["logei", "ei", "ucb", "variance"]
SEED = 1024
SUPER = 1 << 20
CHUNK = {384: 349_440, 640: 209_664}
CASES = [(384, 400_000), (640, 250_000)]
# gpx_sweep_workspace_size(n, 1, m) of the parent build (commit aa478a3), read through its library
PARENT_WORKSPACE = {(4096, 1 << 20): 3792374096, (384, 400_000): 2351392832, (640, 250_000): 2195630880,
                    (384, SUPER + 5000): 3067494992}
_fits = {}
_cands = {}


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def fitted(engine, n, d, kind="rbf", ard=False):
    """(state, X, y) of one fit per configuration for the whole module; never modified."""
    key = (n, d, kind, ard)
    if key not in _fits:
        X, y = O.synthetic_problem(n, d, 21)
        if ard:
            kp, _ = ard_util.ard_params(kind, d, d, noise=1e-4)
        else:
            kp = KernelParams(kind, botorch_default_lengthscale(d), linear_variance=0.3, noise=1e-4)
        _fits[key] = (engine.fit(t(X), t(y), kp), X, y)
    return _fits[key]


def host_candidates(m, d):
    """The leading m of one Sobol set per d (a host array, shared: copy before writing)."""
    if d not in _cands:
        _cands[d] = O.sobol_candidates(SUPER + 5000 if d == 4 else 400_000, d, 22)
    return _cands[d][:m]


def device_candidates(m, d):
    if ("dev", m, d) not in _cands:
        _cands[("dev", m, d)] = t(host_candidates(m, d))
    return _cands[("dev", m, d)]


def with_options(engine, prune, order, fn):
    before = engine.get_option("sweep_prune"), engine.get_option("sweep_order")
    engine.set_option("sweep_prune", prune)
    engine.set_option("sweep_order", order)
    try:
        out = fn()
        stats = tuple(int(v) for v in engine.sweep_stats())
    finally:
        engine.set_option("sweep_prune", before[0])
        engine.set_option("sweep_order", before[1])
    return out, stats


def acquire(engine, prune, order, st, Xs, acq="logei", **kw):
    (bv, bi), stats = with_options(engine, prune, order, lambda: engine.acquire(st, Xs, acq, **kw))
    return int(bv.view(torch.int64).item()), int(bi.item()), stats


def three(engine, st, Xs, acq="logei", **kw):
    """sweep_prune = 0, then sweep_prune = 2 under sweep_order 1 and 0: equal bits; returns the three results."""
    m = Xs.shape[0]
    full = acquire(engine, 0, 1, st, Xs, acq, **kw)
    assert full[2][0] == m and full[2][1] == m and full[2][2] == full[2][3] > 0
    new = acquire(engine, 2, 1, st, Xs, acq, **kw)
    old = acquire(engine, 2, 0, st, Xs, acq, **kw)
    print(f"sweep_stats order 1 {new[2]} order 0 {old[2]} full {full[2]}")
    for got in (new, old):
        assert got[:2] == full[:2], (got, full)
        assert got[2][0] == m and got[2][3] == full[2][3]
    return full, new, old


# ---- 1. bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("d", [4, 8])
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("acq", ACQS)
def test_equal_bits_under_both_orders(engine, acq, ard, d, n, m):
    st, _, y = fitted(engine, n, d, "rbf", ard)
    Xs = device_candidates(m, d)
    kw = dict(best_f=float(y.max()), beta=4.0)
    _, new, old = three(engine, st, Xs, acq, **kw)
    if acq in ("ucb", "variance"):
        assert new[2] == old[2]
    _, _, sc = engine.acquire(st, Xs, acq, return_scores=True, **kw)
    for k in (1, 16, 1024):
        v_ref, i_ref = engine.topk(sc, k)
        for order in (1, 0):
            (v, i), stats = with_options(engine, 2, order, lambda: engine.acquire_topk(st, Xs, k, acq, **kw))
            print(f"top-{k} order {order}: sweep_stats {stats}")
            assert torch.equal(i, i_ref) and torch.equal(bits(v), bits(v_ref)), (k, order)
            assert stats[0] == m and stats[2] <= stats[3]  # (ei at k = 1024 ran every tile under either order)


@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("kind", ["matern52", "scale_linear_matern52"])
def test_the_matern_kinds_do_not_take_the_order(engine, kind, n, m):
    st, _, y = fitted(engine, n, 4, kind)
    _, new, old = three(engine, st, device_candidates(m, 4), best_f=float(y.max()))
    assert new[2] == old[2]


# ---- 2. the head was skipped -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("d", [4, 8])
def test_product_tiles_of_both_orders(engine, d, n, m):
    """At d = 4 the head did not run over most columns: at most half of the parent order's product tiles (a CPU
    simulation gives 32 against 3141 and 183 against 1986).  d = 8: printed, and never more than the parent order's."""
    st, _, y = fitted(engine, n, d)
    _, new, old = three(engine, st, device_candidates(m, d), best_f=float(y.max()))
    print(f"padded n = {n}, d = {d}, m = {m}: product tiles order 1 {new[2][2]}, order 0 {old[2][2]}")
    assert new[2][2] <= old[2][2]
    if d == 4:
        assert 2 * new[2][2] <= old[2][2]


# ---- 3. nothing prunable ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [384, 640])
def test_identical_candidates(engine, n):
    st, _, y = fitted(engine, n, 4)
    m = CHUNK[n] + 5000
    Xs = t(np.repeat(host_candidates(5000, 4)[17:18], m, axis=0))
    full = acquire(engine, 0, 1, st, Xs, best_f=float(y.max()), index_offset=11)
    new = acquire(engine, 1, 1, st, Xs, best_f=float(y.max()), index_offset=11)
    print(f"sweep_stats order 1 {new[2]} full {full[2]}")
    assert new[:2] == full[:2] and full[1] == 11
    assert new[2][1] == m and new[2][2] == new[2][3] == full[2][3]


# ---- 4. pass 1 keeps, pass 2 or the stages drop ------------------------------------------------------------------------
def test_copies_of_the_best_training_row(engine):
    """50 000 copies of the training row with the largest y: a high mean, so the prior-variance bound keeps them, and a
    posterior variance near zero, so they die once the product's row tiles are in the bound.

    Padded n = 640 only.  With mu = best_f and the prior variance 1 the copies' bound is logEI = log(phi(0)) = -0.92.
    Pass 1 keeps them only where the call's best score lies below that: it is -3.03 on the n = 640 set and -0.87 on the
    n = 384 set (tools/mean_first_sim.py, profiles/r21_meanfirst_sim.jsonl), so at n = 384 pass 1 drops the copies
    (sweep_stats (400000, 1024, 31, 9375) on an MI355X) and the input is not this test's scenario."""
    n, m = CASES[1]
    st, X, y = fitted(engine, n, 4)
    Xs = host_candidates(m, 4).copy()
    Xs[100_000:150_000] = X[int(np.argmax(y))]
    _, new, old = three(engine, st, t(Xs), best_f=float(y.max()))
    assert new[2][1] < SEED + 5000
    assert new[2][2] >= 50_000 // 128


# ---- 5. the list-driven head against the contiguous one ----------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [3, 8, 16])
@pytest.mark.parametrize("n", [100, 300])
def test_list_driven_head_has_the_contiguous_bits(engine, n, d, kind):
    m = 1000
    kp, X, alpha, W = case(engine, kind, n, d)
    Xs_host = head_candidates(X.cpu().numpy(), m, np.random.default_rng(7 * n + d + m))
    Xs = t(Xs_host)
    nan_row, inf_row = 3 * (m // 8) + 5, m - 3
    ss_ref, mu_ref = head_product(engine, kp, X, alpha, Xs, W)
    ld = ss_ref.shape[0]
    perm = np.random.default_rng(n + d).permutation(m)
    perm = perm[(perm != nan_row) & (perm != inf_row)][:700]  # a scrambled subset of 0 .. 999
    perm[0], perm[126] = nan_row, inf_row  # count 1 lists the NaN row, every count >= 127 both
    assert len(set(perm.tolist())) == 700
    lst = torch.tensor(np.stack([perm, np.full_like(perm, -7)], axis=1), dtype=torch.int32, device=DEV).contiguous()
    pc = kp.to_c(d)
    for cnt in (0, 1, 127, 128, 129, 700):
        ss = torch.full((ld,), float("nan"), dtype=torch.float64, device=DEV)
        mu = torch.full((2, ld), float("nan"), dtype=torch.float64, device=DEV)
        poison = bits(ss[:1]).clone()
        count = torch.tensor([cnt], dtype=torch.int32, device=DEV)
        _capi.check(engine.lib.gpx_debug_head_product_list_f64(
            engine.handle, ctypes.byref(pc), n, ptr(X), X.stride(0), ptr(alpha), ptr(Xs), m, Xs.stride(0), ptr(W),
            W.stride(0), ptr(ss), ptr(mu), ld, ptr(lst), ptr(count)), engine.handle)
        torch.cuda.synchronize()
        listed = torch.zeros(ld, dtype=torch.bool, device=DEV)
        listed[torch.tensor(perm[:cnt].astype(np.int64), device=DEV)] = True
        assert int(listed.sum()) == cnt
        assert torch.equal(bits(ss)[listed], bits(ss_ref)[listed]), cnt
        assert torch.equal(bits(mu)[:, listed], bits(mu_ref)[:, listed]), cnt
        assert bool((bits(ss)[~listed] == poison).all()) and bool((bits(mu)[:, ~listed] == poison).all()), cnt
    assert torch.isnan(ss_ref[nan_row])  # the NaN row reaches the sums


def test_list_entry_rejects_null_list_and_count(engine):
    kp, X, alpha, W = case(engine, "rbf", 300, 8)
    Xs = t(np.random.default_rng(1).random((129, 8)))
    out = torch.empty((3, 256), dtype=torch.float64, device=DEV)
    lst = torch.zeros((4, 2), dtype=torch.int32, device=DEV)
    count = torch.ones(1, dtype=torch.int32, device=DEV)
    pc = kp.to_c(8)
    call = lambda l, c: engine.lib.gpx_debug_head_product_list_f64(  # noqa: E731
        engine.handle, ctypes.byref(pc), 300, ptr(X), X.stride(0), ptr(alpha), ptr(Xs), 129, 8, ptr(W), W.stride(0),
        ptr(out[0]), ptr(out[1:]), 256, ptr(l), ptr(c))
    assert call(None, count) == _capi.GPX_INVALID_ARG
    assert call(lst, None) == _capi.GPX_INVALID_ARG
    assert call(lst, count) == _capi.GPX_OK
    torch.cuda.synchronize()


# ---- 6. NaN and infinite candidates ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("d", [4, 8])
def test_nan_and_infinite_candidates(engine, d, n, m):
    """A NaN row and a row with an infinite coordinate among the others, and one slice that holds nothing else (its seed
    is one of them)."""
    st, _, y = fitted(engine, n, d)
    Xs = host_candidates(m, d).copy()
    Xs[12_345] = np.nan
    Xs[m - 77, d - 1] = np.inf
    lo, hi = 500 * m // SEED, 501 * m // SEED
    Xs[lo:hi] = np.nan
    Xs[lo + 1:hi:2, 0] = np.inf
    full, _, _ = three(engine, st, t(Xs), best_f=float(y.max()))
    assert not (lo <= full[1] < hi) and full[1] not in (12_345, m - 77)


# ---- 7. a second span --------------------------------------------------------------------------------------------------
def test_two_spans(engine):
    """m = 2^20 + 5000 at padded n = 384: the seeded span and a second one pruned mean-first against its incumbent; the
    winner moved into the second span comes back from there."""
    st, _, y = fitted(engine, 384, 4)
    m = SUPER + 5000
    kw = dict(best_f=float(y.max()))
    base = host_candidates(m, 4)
    full, new, _ = three(engine, st, t(base), **kw)
    assert new[2][2] < new[2][3]
    i0 = full[1]
    Xs = base.copy()
    Xs[i0] = base[(i0 + 1) % m]
    Xs[SUPER + 1234] = base[i0]
    full2, new2, _ = three(engine, st, t(Xs), **kw)
    assert full2[1] == SUPER + 1234 and new2[2][2] < new2[2][3]


# ---- 8. workspace ------------------------------------------------------------------------------------------------------
def test_workspace_of_exactly_the_reported_size(engine, monkeypatch):
    n, m = CASES[0]
    st, _, y = fitted(engine, n, 4)
    Xs = device_candidates(m, 4)
    run = lambda: acquire(engine, 2, 1, st, Xs, best_f=float(y.max()))  # noqa: E731
    want = run()
    guarded = GuardedWorkspace(0)  # every byte 0xFF on entry: a NaN in every double
    monkeypatch.setattr(engine, "workspace", guarded)
    got = run()
    assert guarded.guards_intact(), "a kernel wrote outside the reported workspace"
    assert guarded.asked == [PARENT_WORKSPACE[(n, m)]]
    assert got == want


def test_workspace_sizes_are_the_parents(engine):
    for (n, m), want in PARENT_WORKSPACE.items():
        b = ctypes.c_size_t()
        assert engine.lib.gpx_sweep_workspace_size(n, 1, m, ctypes.byref(b)) == _capi.GPX_OK
        assert b.value == want, (n, m)


# ---- 9. the option -----------------------------------------------------------------------------------------------------
def test_option_defaults_to_mean_first(engine):
    assert engine.get_option("sweep_order") == 1
    for bad in (2, -1):
        with pytest.raises(Exception):
            engine.set_option("sweep_order", bad)
    assert engine.get_option("sweep_order") == 1
