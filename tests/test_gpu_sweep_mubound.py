"""The lazy pruned sweep's bound of the posterior mean (gpx_mubound.hip).

The head phase no longer computes every candidate's exact mean: mu_bound_kernel gives mu_approx and mu_slack with
|mu_approx - mu| <= mu_slack, mu being the value the exact path computes, and the survivors get their exact mean
partials from the gather build.  Yardsticks: the bound holds and is not vacuous (gpx_debug_mu_bound_f64 against the
full build's partials from gpx_debug_kstar_mu_f64, summed in sum_partials' order), the fast exponential alone against
the device's fp64 exp, the gathered partials byte for byte, and (best_val, best_idx) bit for bit with sweep_prune = 2
against 0 (full sweep) and -2 (exact head means).
"""
import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import GPEngine, KernelParams, botorch_default_lengthscale
from oracle import gp_oracle as O
from tests.mu_bound_util import DEV, kstar_mu, mu_bound, mu_exact, t

pytestmark = pytest.mark.gpu
EPS1, EPS2 = 2.0 ** -20, 2.0 ** -120  # MUB_EPS1, MUB_EPS2 of gpx_mubound.hip
CHUNK640 = 209_664
_fits = {}
_cands = {}


def fitted(engine, n, d=4):
    """One RBF fit per shape for the whole module; never modified."""
    if (n, d) not in _fits:
        X, y = O.synthetic_problem(n, d, 21)
        kp = KernelParams("rbf", botorch_default_lengthscale(d), noise=1e-4)
        _fits[(n, d)] = (engine.fit(t(X), t(y), kp), X, y, kp)
    return _fits[(n, d)]


def candidates(m, d=4):
    if (m, d) not in _cands:
        _cands[(m, d)] = O.sobol_candidates(m, d, 22)
    return _cands[(m, d)]


# ---- the bound holds and is not vacuous ---------------------------------------------------------------------------
def bound_candidates(X, d, rng):
    """3000 candidates: random, exact copies of training rows (r2 = 0), far points (r2 in the underflow range), one NaN
    and one with an infinite coordinate."""
    Xs = rng.random((3000, d))
    Xs[2000:2300] = X[rng.integers(0, X.shape[0], 300)]
    Xs[2300:2900] *= 50.0
    Xs[2950] = np.nan
    Xs[2960, d - 1] = np.inf
    return Xs


@pytest.mark.parametrize("d", [3, 8, 16])
@pytest.mark.parametrize("n", [300, 640, 1000])
def test_bound_holds_and_is_not_vacuous(engine, n, d):
    st, X, y, kp = fitted(engine, n, d)
    rng = np.random.default_rng(100 * n + d)
    Xs = bound_candidates(X, d, rng)
    m = Xs.shape[0]
    finite = torch.tensor(np.isfinite(Xs).all(axis=1), device=DEV)
    Xd, Xsd = t(X), t(Xs)
    npad = st.npad
    fit_alpha = st.alpha[:, 0].contiguous().clone()
    alt = torch.zeros(npad, dtype=torch.float64, device=DEV)
    alt[:n] = t(1e8 * (1.0 - 2.0 * (np.arange(n) % 2)))
    cases = {"fitted": fit_alpha, "y x 1e6": fit_alpha * 1e6, "alternating 1e8": alt, "zero": torch.zeros_like(alt)}
    okp = O.KernelParams(O.RBF, np.full(d, botorch_default_lengthscale(d)))
    Kh = None
    for name, alpha in cases.items():
        _, part = kstar_mu(engine, kp, Xd, alpha, Xsd, m)
        mu = mu_exact(part, m)
        ma, sl = mu_bound(engine, kp, Xd, alpha, Xsd)[:2]
        err = (ma - mu).abs()
        worst = float((err[finite] / sl[finite].clamp_min(1e-300)).max())
        print(f"n={n} d={d} alpha {name}: max |mu_approx - mu| / mu_slack = {worst:.3g}, "
              f"max slack {float(sl[finite].max()):.3g}, max |mu| {float(mu[finite].abs().max()):.3g}")
        assert bool((err[finite] <= sl[finite]).all())
        assert bool(torch.isnan(ma[2950])) and bool(torch.isnan(mu[2950]))
        if name == "zero":
            assert bool((ma[finite] == 0).all()) and bool((sl[finite] == 0).all())
        if name == "fitted":
            if Kh is None:
                fin = np.isfinite(Xs).all(axis=1)
                Kh = np.zeros((n, m))
                Kh[:, fin] = O.kernel_matrix(X, Xs[fin], okp)
            a = alpha[:n].cpu().numpy()
            cap = 2.0 ** -16 * (np.abs(a) @ Kh) + 2.0 ** -20 * 1.0 * np.abs(a).sum()
            assert bool((sl[finite] <= t(cap)[finite]).all())


def test_fast_exponential_against_the_device_exp(engine):
    """d = 1, one training row at 0, alpha = 1, outputscale 1: K* is the device's fp64 exp(-x^2 / 2), mu_approx the fast
    one of the same r2.  2^21 arguments over [-760, 0], the edges, and every fp32 base-2 argument of three binades
    ([-1, -0.5), [-16, -8), [-128, -64): the last one crosses the flush of results below 2^-126)."""
    kp = KernelParams("rbf", 1.0)
    X = t(np.zeros((1, 1)))
    alpha = torch.zeros(128, dtype=torch.float64, device=DEV)
    alpha[0] = 1.0
    grids = [np.concatenate([np.linspace(-760.0, 0.0, 1 << 21), [-0.0, -745.2, -1e4]])]
    for hi in (0x3F000000, 0x41000000, 0x42800000):  # 0.5, 8, 64: the binade's 2^23 fp32 values, negated
        yf = -(np.arange(hi, hi + (1 << 23), dtype=np.uint32).view(np.float32).astype(np.float64))
        grids.append(yf * np.log(2.0))  # exp's argument whose base-2 form is yf
    args = np.concatenate(grids)
    assert args.size >= 1 << 22
    worst, CH = 0.0, 1 << 20
    for s in range(0, args.size, CH):
        x = t(np.sqrt(-2.0 * args[s:s + CH])).reshape(-1, 1).contiguous()
        m = x.shape[0]
        K, _ = kstar_mu(engine, kp, X, alpha, x, m)
        E = K[0, :m]
        et, sl = mu_bound(engine, kp, X, alpha, x)[:2]
        bound = EPS1 * et + EPS2
        ratio = float(((et - E).abs() / bound).max())
        worst = max(worst, ratio)
        assert bool(((et - E).abs() <= bound / 4).all()), ratio
        assert bool(((et - E).abs() <= sl).all())
    print(f"fast exponential: max |exp~ - exp| / (eps1 exp~ + eps2) = {worst:.4f} over {args.size} arguments")


# ---- the gather build's mean partials ------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 8, 16])
def test_gather_partials_have_the_bits_of_the_full_build(engine, d):
    rng = np.random.default_rng(7 + d)
    kp = KernelParams("rbf", list(0.3 + rng.random(d)), outputscale=1.3)
    check_gather_partials(engine, d, kp, rng)


def check_gather_partials(engine, d, kp, rng):
    n, m, cap, cnt = 300, 3000, 1500, 1061  # padded n = 384; the count is no multiple of 128
    X, _ = O.synthetic_problem(n, d, 21)
    Xs = rng.random((m, d))
    alpha = t(np.concatenate([rng.standard_normal(n) * 50.0, np.zeros(84)]))
    idx = rng.permutation(m)[:cap].astype(np.int32)
    Xd, Xsd = t(X), t(Xs)
    full_k, full_p = kstar_mu(engine, kp, Xd, alpha, Xsd, m)
    lst = torch.tensor(idx, dtype=torch.int32, device=DEV)
    count = torch.tensor([cnt], dtype=torch.int32, device=DEV)
    SENT = -12345.678
    part = torch.full((384 // 64, 3072), SENT, dtype=torch.float64, device=DEV)
    got_k, part = kstar_mu(engine, kp, Xd, alpha, Xsd, cap, lst, count, mu_part=part, ldmu=3072)
    listed = torch.tensor(idx[:cnt].astype(np.int64), device=DEV)
    assert torch.equal(part[:, listed].view(torch.int64), full_p[:, listed].view(torch.int64))
    assert torch.equal(got_k[:, :cnt].view(torch.int64), full_k[:, listed].view(torch.int64))
    mask = torch.ones(3072, dtype=torch.bool, device=DEV)
    mask[listed] = False
    assert bool((part[:, mask] == SENT).all())
    assert not bool((full_p[:, :m] == SENT).any())


# ---- results keep their bits ----------------------------------------------------------------------------------------
def acquire(engine, prune, st, Xs, acq="logei", **kw):
    before = engine.get_option("sweep_prune")
    engine.set_option("sweep_prune", prune)
    try:
        bv, bi = engine.acquire(st, Xs, acq, **kw)
        stats = engine.sweep_stats()
    finally:
        engine.set_option("sweep_prune", before)
    return int(bv.view(torch.int64).item()), int(bi.item()), stats


def three(engine, st, Xs, acq="logei", **kw):
    full = acquire(engine, 0, st, Xs, acq, **kw)
    exact = acquire(engine, -2, st, Xs, acq, **kw)
    bound = acquire(engine, 2, st, Xs, acq, **kw)
    print(f"sweep_stats bound {bound[2]} exact head {exact[2]} full {full[2]}")
    assert bound[:2] == full[:2] and exact[:2] == full[:2], (bound, exact, full)
    assert bound[2][0] == Xs.shape[0] and bound[2][3] == full[2][3]
    return full, exact, bound


@pytest.mark.parametrize("m", [5000, 150_000])
@pytest.mark.parametrize("n", [300, 640, 1000])
@pytest.mark.parametrize("acq", ["ei", "logei", "ucb", "variance"])
def test_argmax_bits(engine, acq, n, m):
    st, _, y, _ = fitted(engine, n)
    off = 7 * 2 ** 20
    kw = dict(best_f=0.3 + 1.7 * float(y.max()), beta=4.0, y_mean=0.3, y_scale=1.7, index_offset=off)
    full, _, _ = three(engine, st, t(candidates(m)), acq, **kw)
    assert off <= full[1] < off + m


def test_identical_candidates_nothing_prunable(engine):
    st, _, y, _ = fitted(engine, 640)
    Xs = t(np.repeat(candidates(5000)[17:18], 4096, axis=0))
    full, _, bound = three(engine, st, Xs, best_f=float(y.max()), index_offset=11)
    assert full[1] == 11 and bound[2][1] == 4096


def test_winner_only_in_the_second_super_chunk_and_equal_scores(engine):
    """The call's first super-chunk is one chunk long.  The best candidate is moved behind that boundary; then a copy of
    it (a bit-equal score) is put at a lower index of the second super-chunk and at one of the first: the lowest wins."""
    st, _, y, _ = fitted(engine, 640)
    m = CHUNK640 + 5000
    base = candidates(m)
    kw = dict(best_f=float(y.max()))
    i0 = acquire(engine, 0, st, t(base), **kw)[1]
    Xs = base.copy()
    hi = CHUNK640 + 3000
    assert i0 != hi and i0 + 1 < m
    Xs[i0] = base[i0 + 1]
    Xs[hi] = base[i0]
    full, _, _ = three(engine, st, t(Xs), **kw)
    assert full[1] == hi
    for lower in (CHUNK640 + 100, 5000):
        assert lower != i0
        Xs[lower] = base[i0]
        again, _, _ = three(engine, st, t(Xs), **kw)
        assert again[1] == lower and again[0] == full[0]


def test_all_nan_candidates(engine):
    st, _, y, _ = fitted(engine, 640)
    three(engine, st, t(np.full((5000, 4), np.nan)), best_f=float(y.max()))


def test_best_f_so_large_that_every_logei_is_tiny(engine):
    st, _, y, _ = fitted(engine, 640)
    full, _, _ = three(engine, st, t(candidates(5000)), best_f=float(y.max()) + 200.0)
    assert np.int64(full[0]).view(np.float64) < -1e4


def test_large_alpha_large_slack(engine):
    """alpha x 1e6: the slack is large against the score's spread and nearly everything survives the head."""
    st, _, y, _ = fitted(engine, 640)
    alpha = (st.alpha[:, 0] * 1e6).contiguous()
    for acq in ("logei", "ucb"):
        three(engine, st, t(candidates(5000)), acq, best_f=float(y.max()) * 1e6, alpha=alpha)


def test_pruning_still_engages(engine):
    """The n = 640 problem of test_gpu_sweep_lazy.test_pruning_engaged_on_the_lazy_path: the slack may let a few more
    candidates through the head than the exact means do, not many."""
    st, _, y, _ = fitted(engine, 640)
    _, exact, bound = three(engine, st, t(candidates(5000)), best_f=float(y.max()))
    assert bound[2][1] <= 1.25 * exact[2][1] + 16


def test_same_call_twice_same_bits(engine):
    st, _, y, _ = fitted(engine, 640)
    Xs = t(candidates(150_000))
    kw = dict(best_f=float(y.max()))
    a = acquire(engine, 2, st, Xs, **kw)
    b = acquire(engine, 2, st, Xs, **kw)
    assert a == b
