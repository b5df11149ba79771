"""The seeded order of the lazy pruned sweep: a call longer than one chunk takes its first incumbent from
the head bound's best column in each of 1024 slices of its first span, not from its leading 1024 candidates.

The yardstick is bit identity of (best_val, best_idx), and of every top-k pair, against sweep_prune = 0, plus the
sweep_stats identities.  Shapes: the smallest where the order runs, a call just over one chunk at the two smallest
padded n with an odd and an even number of row tiles beyond the head's: padded n = 384 (3 row tiles, chunk 349 440
columns) with m = 400 000 and padded n = 640 (5 row tiles, chunk 209 664) with m = 250 000; d = 4.
"""
import numpy as np
import pytest
import scipy.linalg as sla
import torch

from bayesianoptimizer_amd import KernelParams, botorch_default_lengthscale
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KINDS = ["rbf", "matern52", "scale_linear_matern52"]
ACQS = ["logei", "ei", "ucb", "variance"]
SEED = 1024
SUPER = 1 << 20
CHUNK = {384: 349_440, 640: 209_664}
CASES = [(384, 400_000), (640, 250_000)]
# sweep_stats[2] (128 x 128 product tiles) of the sweep_prune = 2 logei call on the rbf fit of each case on the parent
# build (commit 923fdd5: the leading 1024 candidates as the seed, a first span of one chunk), read on an MI355X through
# GPX_LIB with this file's inputs.
PARENT_TILES = {(384, 400_000): 3157, (640, 250_000): 2668}
_fits = {}
_cands = {}


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def fitted(engine, n, kind="rbf"):
    """One fit per configuration for the whole module; never modified."""
    if (n, kind) not in _fits:
        X, y = O.synthetic_problem(n, 4, 21)
        kp = KernelParams(kind, botorch_default_lengthscale(4), linear_variance=0.3, noise=1e-4)
        _fits[(n, kind)] = (engine.fit(t(X), t(y), kp), X, y)
    return _fits[(n, kind)]


def candidates(m):
    """The leading m of one Sobol set (a host array, shared: copy before writing)."""
    if "all" not in _cands:
        _cands["all"] = O.sobol_candidates(SUPER + 5000, 4, 22)
    return _cands["all"][:m]


def slice_of(c, m):
    return ((c + 1) * SEED - 1) // m


def slice_range(s, m):
    return s * m // SEED, (s + 1) * m // SEED


def acquire(engine, prune, st, Xs, acq="logei", **kw):
    before = engine.get_option("sweep_prune")
    engine.set_option("sweep_prune", prune)
    try:
        bv, bi = engine.acquire(st, Xs, acq, **kw)
        stats = engine.sweep_stats()
    finally:
        engine.set_option("sweep_prune", before)
    return int(bv.view(torch.int64).item()), int(bi.item()), stats


def both(engine, st, Xs, acq="logei", modes=(2, -2), **kw):
    """sweep_prune = 2 (the mean's bound) and -2 (exact head means) against 0; returns (full, [pruned per mode])."""
    m = Xs.shape[0]
    full = acquire(engine, 0, st, Xs, acq, **kw)
    assert full[2][0] == m and full[2][1] == m and full[2][2] == full[2][3] > 0
    out = []
    for mode in modes:
        pruned = acquire(engine, mode, st, Xs, acq, **kw)
        print(f"sweep_prune {mode}: sweep_stats {pruned[2]} full {full[2]}")
        assert pruned[:2] == full[:2], (mode, pruned, full)
        assert pruned[2][0] == m and pruned[2][3] == full[2][3]
        out.append(pruned)
    return full, out


def winner(engine, st, Xs, acq="logei", **kw):
    return acquire(engine, 0, st, Xs, acq, **kw)[1]


@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("acq", ACQS)
@pytest.mark.parametrize("kind", KINDS)
def test_equal_bits(engine, kind, acq, n, m):
    st, _, y = fitted(engine, n, kind)
    full, pruned = both(engine, st, t(candidates(m)), acq, best_f=float(y.max()), beta=4.0)
    for p in pruned:
        assert p[2][2] < p[2][3]


@pytest.mark.parametrize("mode", [2, -2])
def test_same_call_twice_same_bits_and_counters(engine, mode):
    n, m = CASES[1]
    st, _, y = fitted(engine, n, "scale_linear_matern52")
    Xs = t(candidates(m))
    a = acquire(engine, mode, st, Xs, best_f=float(y.max()))
    b = acquire(engine, mode, st, Xs, best_f=float(y.max()))
    assert a == b


@pytest.mark.parametrize("n,m", [(384, CHUNK[384] + 1), (640, CHUNK[640] + 1), (384, 400_003), (640, 250_101)])
def test_one_past_the_chunk_odd_lengths_and_an_offset(engine, n, m):
    """m = chunk + 1 (the shortest call of the new order; no slice is block-aligned) and an m that is no multiple of
    256, with a non-zero index_offset."""
    st, _, y = fitted(engine, n)
    off = 7 * 2 ** 20 + 3
    full, pruned = both(engine, st, t(candidates(m)), best_f=float(y.max()), index_offset=off)
    assert off <= full[1] < off + m
    for p in pruned:
        assert p[2][2] < p[2][3]


@pytest.mark.parametrize("n,m", CASES)
def test_copies_of_the_winner_lowest_index_wins(engine, n, m):
    st, _, y = fitted(engine, n)
    kw = dict(best_f=float(y.max()))
    base = candidates(m)
    i0 = winner(engine, st, t(base), **kw)
    lo, hi = slice_range(slice_of(i0, m), m)
    assert hi - lo >= 3 and slice_of(lo, m) == slice_of(hi - 1, m) == slice_of(i0, m) and slice_of(hi, m) != slice_of(i0, m)
    # in the same slice: one copy before the original where there is room, else behind it
    Xs = base.copy()
    twin = lo if i0 > lo else hi - 1
    Xs[twin] = base[i0]
    full, _ = both(engine, st, t(Xs), **kw)
    assert full[1] == min(i0, twin)
    # in two other slices, one on each side where the call has room
    Xs = base.copy()
    others = [c for c in (lo - 5 * (hi - lo), hi + 7 * (hi - lo)) if 0 <= c < m]
    assert others and all(slice_of(c, m) != slice_of(i0, m) for c in others)
    Xs[others] = base[i0]
    full2, _ = both(engine, st, t(Xs), **kw)
    assert full2[1] == min([i0] + others) and full2[0] == full[0]


def test_winner_that_is_not_the_best_bound_of_its_slice(engine):
    """A neighbour of the winner in its slice with a larger bound and a smaller score takes the slice's seed; the winner
    must come back through the prune pass and the tail.  The bound is restated here for sweep_prune = -2 (exact mean, the
    variance left after the first 128 rows of the product) to choose the neighbour among small perturbations of the
    winner.  UCB: its bound is loose enough in the variance for the bound and the score to order two neighbours
    differently (logEI's bound of the winner equals its score to 1e-12 on this problem)."""
    n, m = CASES[0]
    st, X, y = fitted(engine, n)
    kw = dict(best_f=float(y.max()), beta=4.0)
    base = candidates(m)
    i0 = winner(engine, st, t(base), acq="ucb", **kw)
    lo, hi = slice_range(slice_of(i0, m), m)
    kp = O.KernelParams(O.RBF, np.full(4, botorch_default_lengthscale(4)), noise=1e-4)
    ost = O.fit(X, y, kp)
    L = np.linalg.cholesky(O.gram(X, kp))
    pool = base[i0] + 0.02 * np.random.default_rng(3).standard_normal((2048, 4))
    pts = np.concatenate([base[lo:hi], pool])
    v0 = sla.solve_triangular(L[:128, :128], O.kernel_matrix(X, pts, kp)[:128], lower=True)
    mu, var = O.posterior(ost, pts)
    bound = O.acquisition(mu, np.maximum(O.kernel_diag(pts, kp) - (v0 * v0).sum(0), 1e-10), O.ACQ_UCB, beta=4.0)
    score = O.acquisition(mu, var, O.ACQ_UCB, beta=4.0)
    ns = hi - lo
    ok = np.flatnonzero((bound[ns:] > bound[:ns].max() + 1e-6) & (score[ns:] < score[i0 - lo] - 1e-6))
    assert ok.size, "no perturbation with a larger bound and a smaller score than the winner"
    Xs = base.copy()
    Xs[i0 + 1 if i0 + 1 < hi else i0 - 1] = pool[ok[0]]
    full, _ = both(engine, st, t(Xs), "ucb", **kw)
    assert full[1] == i0


def test_a_nan_row_and_a_far_point(engine):
    n, m = CASES[1]
    st, _, y = fitted(engine, n)
    kw = dict(best_f=float(y.max()))
    base = candidates(m)
    i0 = winner(engine, st, t(base), **kw)
    lo, hi = slice_range(slice_of(i0, m), m)
    Xs = base.copy()
    Xs[lo if i0 > lo else hi - 1] = np.nan  # in the winner's slice
    Xs[(i0 + m // 2) % m] = 1e3             # far outside the unit cube
    full, _ = both(engine, st, t(Xs), **kw)
    assert full[1] == i0


def test_identical_candidates_every_round_is_live(engine):
    """Nothing can be dropped: every candidate reaches the last row tile exactly once, the seed's included."""
    n = 640
    st, _, y = fitted(engine, n)
    m = CHUNK[n] + 300
    Xs = t(np.repeat(candidates(5000)[17:18], m, axis=0))
    full, (pruned,) = both(engine, st, Xs, modes=(1,), best_f=float(y.max()), index_offset=11)
    assert full[1] == 11
    assert pruned[2][1] == m


def test_two_spans(engine):
    """m = 2^20 + 5000 at padded n = 384: the seeded span of 2^20 and a second one bounded against its best."""
    st, _, y = fitted(engine, 384)
    m = SUPER + 5000
    kw = dict(best_f=float(y.max()))
    base = candidates(m)
    both(engine, st, t(base), **kw)
    i0 = winner(engine, st, t(base), **kw)
    Xs = base.copy()
    Xs[i0] = base[(i0 + 1) % m]
    Xs[SUPER + 1234] = base[i0]  # the winner in the second span only
    full, _ = both(engine, st, t(Xs), **kw)
    assert full[1] == SUPER + 1234


# ---- the top-k form through the same calls ---------------------------------------------------------------------------
def bits(v):
    return v.view(torch.int64).cpu().numpy()


def topk(engine, prune, st, Xs, k, **kw):
    before = engine.get_option("sweep_prune")
    engine.set_option("sweep_prune", prune)
    try:
        v, i = engine.acquire_topk(st, Xs, k, "logei", **kw)
        stats = engine.sweep_stats()
    finally:
        engine.set_option("sweep_prune", before)
    return bits(v), i.cpu().numpy(), stats


@pytest.mark.parametrize("n,m", CASES)
def test_topk_k1_reports_the_argmax_calls_counters(engine, n, m):
    st, _, y = fitted(engine, n)
    Xs = t(candidates(m))
    ref = acquire(engine, 2, st, Xs, best_f=float(y.max()))
    got = topk(engine, 2, st, Xs, 1, best_f=float(y.max()))
    assert (got[0][0], got[1][0]) == ref[:2]
    assert got[2] == ref[2], (got[2], ref[2])


@pytest.mark.parametrize("copies", [False, True])
@pytest.mark.parametrize("n,m", CASES)
def test_topk_equals_the_composition(engine, n, m, copies):
    st, _, y = fitted(engine, n)
    kw = dict(best_f=float(y.max()))
    base = candidates(m)
    if copies:  # the winner again in its own slice and in two others
        i0 = winner(engine, st, t(base), **kw)
        lo, hi = slice_range(slice_of(i0, m), m)
        base = base.copy()
        base[[lo if i0 > lo else hi - 1, (i0 + m // 3) % m, (i0 + 2 * m // 3) % m]] = base[i0]
    Xs = t(base)
    _, _, sc = engine.acquire(st, Xs, "logei", return_scores=True, **kw)
    for k in (16, 1024):
        v_ref, i_ref = engine.topk(sc, k)
        for mode in (2, -2):
            got = topk(engine, mode, st, Xs, k, **kw)
            assert np.array_equal(got[1], i_ref.cpu().numpy()) and np.array_equal(got[0], bits(v_ref)), (k, mode)
            assert len(set(got[1].tolist())) == k
            assert got[2][0] == m and got[2][2] < got[2][3]


@pytest.mark.parametrize("n,m", CASES)
def test_no_more_product_tiles_than_the_parent(engine, n, m):
    st, _, y = fitted(engine, n)
    got = acquire(engine, 2, st, t(candidates(m)), best_f=float(y.max()))
    print(f"padded n = {n}, m = {m}: sweep_stats {got[2]}, the parent's tiles {PARENT_TILES[(n, m)]}")
    assert got[2][2] <= PARENT_TILES[(n, m)]
