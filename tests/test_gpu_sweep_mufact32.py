"""The fp32 factorised form of the pruned sweep's head mean bound (gpx_mubound.hip: mu_fact32_kernel).

For 4 < d <= 8 the dot product y = log2(e) a.b of the factorised form runs on v_mfma_f32_16x16x4_f32 with fp32 fragments.
Its proven relative slack eps1_32(c) = ((11 + 0.6932 (d + 2) Y_c) 2^-24 + eps64) (1 + 2^-8) grows with Y_c, so a workgroup
of 256 candidates takes it only if every candidate has eps1_32 <= 2^-18 (1 - 2^-12); other workgroups eligible for a
factorised form (Y_c <= 16) take the fp64 one (mu_fact_kernel), the rest mu_bound_kernel.  The debug entry leaves two
int64 counters in its 256-byte-aligned workspace: workgroups on mu_bound_kernel's path at byte 0, workgroups on the
fp64 factorised form at byte 160.  Yardsticks: |mu_approx - mu| <= mu_slack on all three paths (mu from
gpx_debug_kstar_mu_f64, summed in sum_partials' order), both counters, the slack's size, the row order of the fp32
record's alpha" (one-hot alpha), and (best_val, best_idx) bit for bit against sweep_prune = 0.

Measured on MI355X (profiles/r13_gpu_tests_mufact32.log): max |mu_approx - mu| / mu_slack over all shapes and alpha cases
0.136 on the fp32 form (0.029 with the fitted alpha, 0.118 with one-hot alpha), 0.233 on the fp64 form, 0.047 on the
unfactorised one; mu_slack at most 0.28 of its cap on the factorised forms.
"""
import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import KernelParams, botorch_default_lengthscale
from oracle import gp_oracle as O
from tests.ard_util import ard_params
from tests.mu_bound_util import DEV, M, kstar_mu, mixed_candidates, mu_bound, mu_exact, t

pytestmark = pytest.mark.gpu
_fits = {}
_cands = {}
_cases = {}


def fitted(engine, n, d, ard=False):
    """One RBF fit per shape for the whole module; never modified.  ard: a lengthscale per dimension
    (tests/ard_util.py, seed d) in place of the default one."""
    if (n, d, ard) not in _fits:
        X, y = O.synthetic_problem(n, d, 21)
        kp = KernelParams("rbf", botorch_default_lengthscale(d), noise=1e-4)
        if ard:
            kp = ard_params("rbf", d, d, noise=1e-4)[0]
        _fits[(n, d, ard)] = (engine.fit(t(X), t(y), kp), X, y, kp)
    return _fits[(n, d, ard)]


def lengthscale(kp, d, ard):
    """What the numpy restatements divide by: the scalar of the default fits, the vector of the ARD ones."""
    return np.array(kp.lengthscales(d)) if ard else botorch_default_lengthscale(d)


def candidates(m, d):
    if (m, d) not in _cands:
        _cands[(m, d)] = O.sobol_candidates(m, d, 22)
    return _cands[(m, d)]


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


def run_case(engine, n, d, ard=False):
    """One shape's mixed candidates through every alpha case, once per module: name -> (mu_approx, mu_slack, mu,
    fallback, fp64form), and the candidates' layout."""
    if (n, d, ard) not in _cases:
        st, X, y, kp = fitted(engine, n, d, ard)
        ls = lengthscale(kp, d, ard)
        rng = np.random.default_rng(1000 * n + d)
        Xs, slow, fp64, on32, on64 = mixed_candidates(X, ls, rng)
        Xd, Xsd = t(X), t(Xs)
        res = {}
        for name, alpha in alpha_cases(st, n, rng).items():
            mu = mu_exact(kstar_mu(engine, kp, Xd, alpha, Xsd, M)[1], M)
            ma, sl, fallback, fp64form = mu_bound(engine, kp, Xd, alpha, Xsd)
            res[name] = (alpha, ma, sl, mu, fallback, fp64form)
        _cases[(n, d, ard)] = (res, X, Xs, slow, fp64, on32, on64)
    return _cases[(n, d, ard)]


def path_ratios(err, sl, masks):
    out = {}
    for name, mk in masks.items():
        if mk.any():
            mt = torch.tensor(mk, device=DEV)
            out[name] = float((err[mt] / sl[mt].clamp_min(1e-300)).max())
    return out


@pytest.mark.parametrize("n,d", [(300, 5), (300, 8), (640, 5), (640, 8), (300, 3), (300, 16)])
def test_bound_holds_on_all_three_paths(engine, n, d):
    check_bound_on_all_three_paths(engine, n, d)


def check_bound_on_all_three_paths(engine, n, d, ard=False):
    res, X, Xs, slow, fp64, on32, on64 = run_case(engine, n, d, ard)
    fin = np.isfinite(Xs).all(axis=1)
    finite = torch.tensor(fin, device=DEV)
    masks = {"fp32 form": on32, "fp64 form": on64, "unfactorised": fin & ~on32 & ~on64}
    for name, (alpha, ma, sl, mu, fallback, fp64form) in res.items():
        err = (ma - mu).abs()
        print(f"n={n} d={d} alpha {name}: max |mu_approx - mu| / mu_slack per path {path_ratios(err, sl, masks)}, "
              f"workgroups on mu_bound_kernel {fallback}, on the fp64 form {fp64form}")
        assert fallback == len(slow) and fp64form == len(fp64), (name, fallback, fp64form)
        assert bool((err[finite] <= sl[finite]).all()), name
        assert bool((sl[finite] >= 0).all()), name
        assert bool(torch.isnan(ma[1900])) and bool(torch.isnan(mu[1900]))
        if name == "zero":
            assert bool((ma[finite] == 0).all()) and bool((sl[finite] == 0).all())


@pytest.mark.parametrize("d", [5, 8])
@pytest.mark.parametrize("n", [300, 640])
def test_slack_size_on_the_factorised_forms(engine, n, d):
    """mu_slack <= 2^-18 sum |alpha_j| k_j + 2^-20 outputscale |alpha|_1 for every candidate on a factorised form."""
    check_slack_size_on_the_factorised_forms(engine, n, d)


def check_slack_size_on_the_factorised_forms(engine, n, d, ard=False, only=None):
    """only: a boolean mask that narrows the factorised candidates checked (None: all of them)."""
    res, X, Xs, slow, fp64, on32, on64 = run_case(engine, n, d, ard)
    alpha, ma, sl, mu, _, _ = res["fitted"]
    fact = (on32 | on64) if only is None else (on32 | on64) & only
    okp = O.KernelParams(O.RBF, np.array(fitted(engine, n, d, ard)[3].lengthscales(d)))
    a = alpha[:n].cpu().numpy()
    A = np.abs(a) @ O.kernel_matrix(X, Xs[fact], okp)
    cap = t(2.0 ** -18 * A + 2.0 ** -20 * 1.0 * np.abs(a).sum())
    ft = torch.tensor(fact, device=DEV)
    err = (ma - mu).abs()
    print(f"n={n} d={d}: max mu_slack / cap = {float((sl[ft] / cap).max()):.3g}; max |mu_approx - mu| / mu_slack: "
          f"{path_ratios(err, sl, {'fp32 form': on32, 'fp64 form': on64})}; unit cube alone "
          f"{float((err[:256] / sl[:256]).max()):.3g}")
    assert bool((sl[ft] <= cap).all())
    assert bool((err[ft] <= sl[ft]).all())


def test_row_order_of_the_fp32_record(engine):
    """One-hot alpha at each of the 64 rows of row block 1 and at the last valid row: mu_approx must be alpha_j k(x_j,
    x*) within the slack.  The f32 accumulator holds row 4 (lane >> 4) + reg, the f64 one (lane >> 4) + 4 reg; alpha" in
    the other's order multiplies the wrong rows' exponentials, which the summed cases can hide."""
    n, d, m = 300, 8, 256
    st, X, y, kp = fitted(engine, n, d)
    rng = np.random.default_rng(7)
    Xs = rng.random((m, d))
    okp = O.KernelParams(O.RBF, np.full(d, botorch_default_lengthscale(d)))
    K = t(O.kernel_matrix(X, Xs, okp))
    Xd, Xsd = t(X), t(Xs)
    worst = 0.0
    for j in list(range(64, 128)) + [n - 1]:
        alpha = torch.zeros(st.npad, dtype=torch.float64, device=DEV)
        alpha[j] = -1.5 if j % 2 else 2.5
        ma, sl, fallback, fp64form = mu_bound(engine, kp, Xd, alpha, Xsd)
        assert fallback == 0 and fp64form == 0  # every workgroup on the fp32 form
        mu = mu_exact(kstar_mu(engine, kp, Xd, alpha, Xsd, m)[1], m)
        assert bool(((ma - mu).abs() <= sl).all()), j
        ref = alpha[j] * K[j]
        # numpy's k against the exact path's: (e) of the proof, (120 Q_c + 4) 2^-53 < 2^-36 for Q_c < 2^10
        assert bool(((ma - ref).abs() <= sl + 2.0 ** -36 * ref.abs()).all()), j
        assert bool((sl > 0).all()) and bool((sl <= 2.0 ** -17 * ref.abs()).all()), j
        worst = max(worst, float(((ma - mu).abs() / sl).max()))
    print(f"one-hot alpha, 65 rows: max |mu_approx - mu| / mu_slack = {worst:.3g}")


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
@pytest.mark.parametrize("n", [640, 1000])
def test_argmax_bits_and_pruning(engine, n, acq):
    """(value bits, index) with the bound equal those of the unpruned sweep, twice the same, and the tiles executed stay
    within 2 % of the run with exact head means (sweep_prune = -2), the project's tolerance for this comparison."""
    st, _, y, _ = fitted(engine, n, 8)
    Xs = t(candidates(1 << 15, 8))
    kw = dict(best_f=float(y.max()), beta=4.0)
    full = acquire(engine, 0, st, Xs, acq, **kw)
    exact = acquire(engine, -2, st, Xs, acq, **kw)
    a = acquire(engine, 2, st, Xs, acq, **kw)
    b = acquire(engine, 2, st, Xs, acq, **kw)
    print(f"n={n} {acq}: sweep_stats bound {a[2]} exact head means {exact[2]} full {full[2]}")
    assert a[:2] == full[:2], (a, full)
    assert a == b
    assert abs(a[2][2] - exact[2][2]) <= 0.02 * exact[2][2]
