"""The factorised form of the pruned sweep's head mean bound (gpx_mubound.hip: mu_fact_kernel).

With one centre for every row block, exp(-r2 / 2) = exp(-|a|^2 / 2) exp(-|b|^2 / 2) exp(a.b): the row factor goes into
alpha, the candidate factor is applied once, and an entry costs one conversion, one v_exp_f32 and two fp32 FMAs.  A
workgroup of 256 candidates takes this form only if Y_c = log2(e) sqrt(max |a|^2 |b|^2) <= 16 for every one of them;
the others keep mu_bound_kernel's loop.  Yardsticks: |mu_approx - mu| <= mu_slack on both paths (mu from
gpx_debug_kstar_mu_f64, summed in sum_partials' order), the slack's size, which path ran (the count of workgroups on
the old path, an int64 at the start of the debug entry's 256-byte-aligned workspace), and (best_val, best_idx) bit for
bit against sweep_prune = 0.
"""
import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import KernelParams, botorch_default_lengthscale
from oracle import gp_oracle as O
from tests.mu_bound_util import DEV, kstar_mu, mu_bound, mu_exact, t

pytestmark = pytest.mark.gpu
Y_LIMIT = 16.0  # MUF_Y_LIMIT of gpx_mubound.hip
LOG2E = 1.4426950408889634
WG = 256
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


def geometry(X, ls):
    """The centre, max |a|^2 and a function Y_c(Xs) of the factorised form, restated in numpy."""
    s = X / ls
    c = s.mean(axis=0)
    m2 = float(((s - c) ** 2).sum(axis=1).max())

    def yc(Xs):
        with np.errstate(invalid="ignore", over="ignore"):
            return LOG2E * np.sqrt(m2 * ((Xs / ls - c) ** 2).sum(axis=1))
    return c, m2, yc


def mixed_candidates(X, ls, rng):
    """3000 candidates in workgroups of 256:  0-3 unit cube, 4 copies of training rows, 5 and 6 hold a block of 300 far
    points (x 50), 7 a single far point among near ones, 8 has every Y_c just under the limit, 9 just over, 10 one
    NaN, 11 (partial) one infinite coordinate.  Returns the candidates and the workgroups expected on the old path."""
    n, d = X.shape
    c, m2, yc = geometry(X, ls)
    Xs = rng.random((3000, d))
    Xs[1024:1280] = X[rng.integers(0, n, 256)]
    Xs[1280:1580] *= 50.0
    Xs[1900] *= 50.0
    for lo, target in ((2048, 0.995 * Y_LIMIT), (2304, 1.005 * Y_LIMIT)):
        u = rng.standard_normal((256, d))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        Xs[lo:lo + 256] = (c + u * (target / (LOG2E * np.sqrt(m2)))) * ls
    Xs[2600] = np.nan
    Xs[2900, d - 1] = np.inf
    y = yc(Xs)
    slow = sorted({i // WG for i in range(3000) if not y[i] <= Y_LIMIT})
    assert slow == [5, 6, 7, 9, 10, 11], slow
    near = np.ones(3000, dtype=bool)
    for g in slow:
        near[g * WG:(g + 1) * WG] = False
    assert float(y[near].max()) <= 0.996 * Y_LIMIT and float(y[2304:2560].min()) >= 1.004 * Y_LIMIT
    return Xs, slow


def alpha_cases(st, n, rng):
    npad = st.npad
    fit_alpha = st.alpha[:, 0].contiguous().clone()
    alt = torch.zeros(npad, dtype=torch.float64, device=DEV)
    alt[:n] = t(1e8 * (1.0 - 2.0 * (np.arange(n) % 2)))
    wide = torch.zeros(npad, dtype=torch.float64, device=DEV)  # 2^200 between the largest and the smallest magnitude
    mag = 2.0 ** (-200.0 * rng.random(n))
    mag[0], mag[1] = 1.0, 2.0 ** -200
    wide[:n] = t(mag * np.where(rng.random(n) < 0.5, -1.0, 1.0))
    return {"fitted": fit_alpha, "fitted x 1e6": fit_alpha * 1e6, "alternating 1e8": alt, "2^200 range": wide,
            "zero": torch.zeros_like(alt)}


def check_bound(engine, kp, Xd, alpha, Xsd, finite, label):
    m = Xsd.shape[0]
    mu = mu_exact(kstar_mu(engine, kp, Xd, alpha, Xsd, m)[1], m)
    ma, sl, fallback, _ = mu_bound(engine, kp, Xd, alpha, Xsd)
    err = (ma - mu).abs()
    worst = float((err[finite] / sl[finite].clamp_min(1e-300)).max())
    print(f"{label}: max |mu_approx - mu| / mu_slack = {worst:.3g}, max slack {float(sl[finite].max()):.3g}, "
          f"max |mu| {float(mu[finite].abs().max()):.3g}, workgroups on the old path {fallback}")
    assert bool((err[finite] <= sl[finite]).all()), label
    assert bool((sl[finite] >= 0).all()), label
    return ma, sl, mu, fallback


@pytest.mark.parametrize("d", [3, 8, 16])
@pytest.mark.parametrize("n", [300, 640, 1000])
def test_bound_holds_on_both_paths(engine, n, d):
    st, X, y, kp = fitted(engine, n, d)
    ls = botorch_default_lengthscale(d)
    rng = np.random.default_rng(1000 * n + d)
    Xs, slow = mixed_candidates(X, ls, rng)
    m = Xs.shape[0]
    fin = np.isfinite(Xs).all(axis=1)
    finite = torch.tensor(fin, device=DEV)
    Xd, Xsd = t(X), t(Xs)
    for name, alpha in alpha_cases(st, n, rng).items():
        ma, sl, mu, fallback = check_bound(engine, kp, Xd, alpha, Xsd, finite, f"n={n} d={d} alpha {name}")
        assert fallback == len(slow)
        assert bool(torch.isnan(ma[2600])) and bool(torch.isnan(mu[2600]))
        if name == "zero":
            assert bool((ma[finite] == 0).all()) and bool((sl[finite] == 0).all())
        if name == "fitted":  # not vacuous: the unit-cube candidates, all on the factorised path
            okp = O.KernelParams(O.RBF, np.full(d, ls))
            a = alpha[:n].cpu().numpy()
            A = np.abs(a) @ O.kernel_matrix(X, Xs[:1024], okp)
            cap = 2.0 ** -18 * A + 2.0 ** -20 * 1.0 * np.abs(a).sum()
            err = (ma - mu).abs()[:1024]
            print(f"n={n} d={d}: unit cube, max mu_slack / cap = {float((sl[:1024] / t(cap)).max()):.3g}, "
                  f"max |mu_approx - mu| / mu_slack = {float((err / sl[:1024]).max()):.3g}, "
                  f"max |mu_approx - mu| / A = 2^{float(torch.log2((err / t(A)).max().clamp_min(1e-300))):.1f}")
            assert bool((sl[:1024] <= t(cap)).all())


def test_the_factorised_path_runs_for_near_candidates_only(engine):
    st, X, y, kp = fitted(engine, 640, 8)
    rng = np.random.default_rng(5)
    alpha = st.alpha[:, 0].contiguous()
    near = rng.random((1024, 8))
    finite = torch.ones(1024, dtype=torch.bool, device=DEV)
    _, _, _, fallback = check_bound(engine, kp, t(X), alpha, t(near), finite, "all near")
    assert fallback == 0
    _, _, _, fallback = check_bound(engine, kp, t(X), alpha, t(near * 50.0 + 10.0), finite, "all far")
    assert fallback == 4


def test_outlier_training_row_sends_everything_to_the_old_path(engine):
    n, d, m = 300, 8, 1000
    rng = np.random.default_rng(6)
    X, _ = O.synthetic_problem(n, d, 21)
    X = X.copy()
    X[137] *= 50.0
    ls = botorch_default_lengthscale(d)
    kp = KernelParams("rbf", ls)
    Xs = rng.random((m, d))
    _, _, yc = geometry(X, ls)
    y = yc(Xs)
    groups = {i // WG for i in range(m) if not y[i] <= Y_LIMIT}
    assert groups == {0, 1, 2, 3}
    npad = int(engine.lib.gpx_padded_n(n))
    alpha = torch.zeros(npad, dtype=torch.float64, device=DEV)
    alpha[:n] = t(rng.standard_normal(n) * 30.0)
    finite = torch.ones(m, dtype=torch.bool, device=DEV)
    _, _, _, fallback = check_bound(engine, kp, t(X), alpha, t(Xs), finite, "outlier row")
    assert fallback == 4


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


@pytest.mark.parametrize("acq", ["logei", "ucb"])
def test_argmax_bits_with_near_and_far_candidates(engine, acq):
    st, _, y, _ = fitted(engine, 640)
    Xs = candidates(5000).copy()
    Xs[1000:1300] *= 50.0
    Xs[3000] *= 50.0
    Xs[4100:4400] = Xs[4100:4400] * 3.0 - 1.0
    Xsd = t(Xs)
    kw = dict(best_f=0.3 + 1.7 * float(y.max()), beta=4.0, y_mean=0.3, y_scale=1.7, index_offset=3 * 2 ** 20)
    full = acquire(engine, 0, st, Xsd, acq, **kw)
    a = acquire(engine, 2, st, Xsd, acq, **kw)
    b = acquire(engine, 2, st, Xsd, acq, **kw)
    print(f"sweep_stats bound {a[2]} full {full[2]}")
    assert a[:2] == full[:2], (a, full)
    assert a == b


def test_pruning_keeps_engaging(engine):
    """Tiles executed with the bound against the exact head means (sweep_prune = -2) of the same build: within 2 %.
    Over 85 % of the tiles are the fixed head, so 2 % is room for about a seventh more tail tiles."""
    st, _, y, _ = fitted(engine, 1000, 8)
    Xs = t(candidates(1 << 15, 8))
    kw = dict(best_f=float(y.max()))
    exact = acquire(engine, -2, st, Xs, **kw)
    bound = acquire(engine, 2, st, Xs, **kw)
    print(f"tiles executed: bound {bound[2][2]} exact head means {exact[2][2]}; "
          f"head survivors (sweep_stats[1]): bound {bound[2][1]} exact {exact[2][1]}")
    assert bound[:2] == exact[:2]
    assert abs(bound[2][2] - exact[2][2]) <= 0.02 * exact[2][2]
