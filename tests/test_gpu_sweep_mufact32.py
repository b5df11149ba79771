"""The fp32 factorised form of the pruned sweep's head mean bound (gpx_sweep.hip 1b: mu_fact32_kernel).

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
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import KernelParams, botorch_default_lengthscale, _capi
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
Y_LIMIT = 16.0  # MUF_Y_LIMIT of gpx_sweep.hip
EPS32_LIMIT = 2.0 ** -18 * (1.0 - 2.0 ** -12)  # MUF32_EPS1_MAX (1 - 2^-12): the fp32 form's eligibility
LOG2E = 1.4426950408889634
RUN_TERMS = 11.0  # MUF32_RUN + 3: a run of 8 fp32 FMAs, v_exp_f32's 2 v and the rounding of alpha"
WG = 256
M = 3000
FP64FORM_BYTE = 160  # the second counter's offset in the aligned workspace (include/gpx.h)
_fits = {}
_cands = {}
_cases = {}


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def ptr(a):
    return ctypes.c_void_p(a.data_ptr()) if a is not None else None


def fitted(engine, n, d):
    """One RBF fit per shape for the whole module; never modified."""
    if (n, d) not in _fits:
        X, y = O.synthetic_problem(n, d, 21)
        kp = KernelParams("rbf", botorch_default_lengthscale(d), noise=1e-4)
        _fits[(n, d)] = (engine.fit(t(X), t(y), kp), X, y, kp)
    return _fits[(n, d)]


def candidates(m, d):
    if (m, d) not in _cands:
        _cands[(m, d)] = O.sobol_candidates(m, d, 22)
    return _cands[(m, d)]


def kstar_mu(engine, kp, X, alpha, Xs, m):
    """gpx_debug_kstar_mu_f64 -> the full build's mean partials."""
    lib, n, d = engine.lib, X.shape[0], X.shape[1]
    npad = int(lib.gpx_padded_n(n))
    ld = (m + 255) // 256 * 256
    out = torch.full((npad, ld), float("nan"), dtype=torch.float64, device=DEV)
    mu_part = torch.full((npad // 64, ld), float("nan"), dtype=torch.float64, device=DEV)
    pc = kp.to_c(d)
    st = lib.gpx_debug_kstar_mu_f64(engine.handle, ctypes.byref(pc), n, ptr(X), X.stride(0), ptr(alpha), ptr(Xs), m,
                                    Xs.stride(0), None, None, ptr(out), ld, ptr(mu_part), 0)
    _capi.check(st, engine.handle)
    torch.cuda.synchronize()
    return mu_part


def mu_exact(mu_part, m):
    """The partials summed as sum_partials does: ascending row block, one accumulator."""
    s = torch.zeros(m, dtype=torch.float64, device=DEV)
    for jb in range(mu_part.shape[0]):
        s = s + mu_part[jb, :m]
    return s


def mu_bound(engine, kp, X, alpha, Xs):
    """gpx_debug_mu_bound_f64 -> (mu_approx, mu_slack, workgroups on mu_bound_kernel, workgroups on mu_fact_kernel)."""
    lib, n, d, m = engine.lib, X.shape[0], X.shape[1], Xs.shape[0]
    nbytes = ctypes.c_size_t()
    assert lib.gpx_debug_mu_bound_workspace_size(n, ctypes.byref(nbytes)) == _capi.GPX_OK
    ws = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device=DEV)
    ma = torch.full((m,), float("nan"), dtype=torch.float64, device=DEV)
    sl = torch.full((m,), float("nan"), dtype=torch.float64, device=DEV)
    pc = kp.to_c(d)
    st = lib.gpx_debug_mu_bound_f64(engine.handle, ctypes.byref(pc), n, ptr(X), X.stride(0), ptr(alpha), ptr(Xs), m,
                                    Xs.stride(0), ptr(ma), ptr(sl), ptr(ws), ws.numel())
    _capi.check(st, engine.handle)
    torch.cuda.synchronize()
    off = (-ws.data_ptr()) % 256
    fallback = int(ws[off:off + 8].view(torch.int64).item())
    fp64form = int(ws[off + FP64FORM_BYTE:off + FP64FORM_BYTE + 8].view(torch.int64).item())
    return ma, sl, fallback, fp64form


class Geometry:
    """The centre, max |a|^2, Y_c and eps1_32(c) of the factorised forms, restated in numpy."""

    def __init__(self, X, ls):
        self.n, self.d = X.shape
        self.ls = ls
        s = X / ls
        self.c = s.mean(axis=0)
        self.m2 = float(((s - self.c) ** 2).sum(axis=1).max())

    def nbq(self, Xs):
        with np.errstate(invalid="ignore", over="ignore"):
            return ((Xs / self.ls - self.c) ** 2).sum(axis=1)

    def yc(self, Xs):
        with np.errstate(invalid="ignore", over="ignore"):
            return LOG2E * np.sqrt(self.m2 * self.nbq(Xs)) * (1.0 + 2.0 ** -40)

    def eps32_of(self, yc, q):
        eps64 = (256.0 * q + 512.0 + 2.0 * (self.n + 64)) * 2.0 ** -53
        return ((RUN_TERMS + 0.6932 * (self.d + 2) * yc) * 2.0 ** -24 + eps64) * (1.0 + 2.0 ** -8)

    def eps32(self, Xs):
        with np.errstate(invalid="ignore", over="ignore"):
            return self.eps32_of(self.yc(Xs), self.m2 + self.nbq(Xs))

    def ring(self, rng, count, yc):
        """Points with Y_c = yc, in random directions from the centre."""
        u = rng.standard_normal((count, self.d))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        return (self.c + u * (yc / (LOG2E * np.sqrt(self.m2)))) * self.ls

    def yc_at_eps32(self, target):
        yc = 1.0
        for _ in range(4):  # (eps64 moves with Y_c through q; it is 2^-15 of the whole)
            q = self.m2 + (yc / LOG2E) ** 2 / self.m2
            eps64 = (256.0 * q + 512.0 + 2.0 * (self.n + 64)) * 2.0 ** -53
            yc = ((target / (1.0 + 2.0 ** -8) - eps64) * 2.0 ** 24 - RUN_TERMS) / (0.6932 * (self.d + 2))
        return yc


def mixed_candidates(X, ls, rng):
    """3000 candidates in workgroups of 256: 0 unit cube, 1 copies of training rows, 2 a ring with every eps1_32 at 0.995
    of the limit, 3 a ring at 1.005 of it, 4 a ring just under Y_c = 16, 5 a far block (x 50), 6 one far point among
    near ones, 7 one NaN, 8-10 unit cube, 11 (partial) one infinite coordinate.  Returns the candidates, the workgroups
    expected on mu_bound_kernel's path and those expected on the fp64 factorised form (4 < d <= 8: over the fp32 limit;
    else every eligible one), from the formulas restated here, with their margins asserted."""
    n, d = X.shape
    g = Geometry(X, ls)
    Xs = rng.random((M, d))
    Xs[256:512] = X[rng.integers(0, n, 256)]
    Xs[512:768] = g.ring(rng, 256, g.yc_at_eps32(0.995 * EPS32_LIMIT))
    Xs[768:1024] = g.ring(rng, 256, g.yc_at_eps32(1.005 * EPS32_LIMIT))
    Xs[1024:1280] = g.ring(rng, 256, 0.995 * Y_LIMIT)
    Xs[1280:1536] *= 50.0
    Xs[1700] *= 50.0
    Xs[1900] = np.nan
    Xs[2900, d - 1] = np.inf
    y, e = g.yc(Xs), g.eps32(Xs)
    groups = range((M + WG - 1) // WG)
    slow = [w for w in groups if not bool((y[w * WG:(w + 1) * WG] <= Y_LIMIT).all())]
    assert slow == [5, 6, 7, 11], slow
    elig = np.ones(M, dtype=bool)
    for w in slow:
        elig[w * WG:(w + 1) * WG] = False
    assert float(y[elig].max()) <= 0.996 * Y_LIMIT
    if 4 < d <= 8:  # the fp32 form is built for DMAX = 8 only
        fp64 = [w for w in groups if w not in slow and not bool((e[w * WG:(w + 1) * WG] <= EPS32_LIMIT).all())]
        assert fp64 == [3, 4], fp64
        on32 = elig.copy()
        for w in fp64:
            on32[w * WG:(w + 1) * WG] = False
        # the margins: nothing within 0.4 % of the limit on either side, the rings where they were put
        assert float(e[on32].max()) <= 0.996 * EPS32_LIMIT and float(e[768:1024].min()) >= 1.004 * EPS32_LIMIT
        assert float(e[512:768].min()) >= 0.994 * EPS32_LIMIT
    else:
        fp64 = [w for w in groups if w not in slow]
        on32 = np.zeros(M, dtype=bool)
    return Xs, slow, fp64, on32, elig & ~on32


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


def run_case(engine, n, d):
    """One shape's mixed candidates through every alpha case, once per module: name -> (mu_approx, mu_slack, mu,
    fallback, fp64form), and the candidates' layout."""
    if (n, d) not in _cases:
        st, X, y, kp = fitted(engine, n, d)
        ls = botorch_default_lengthscale(d)
        rng = np.random.default_rng(1000 * n + d)
        Xs, slow, fp64, on32, on64 = mixed_candidates(X, ls, rng)
        Xd, Xsd = t(X), t(Xs)
        res = {}
        for name, alpha in alpha_cases(st, n, rng).items():
            mu = mu_exact(kstar_mu(engine, kp, Xd, alpha, Xsd, M), M)
            ma, sl, fallback, fp64form = mu_bound(engine, kp, Xd, alpha, Xsd)
            res[name] = (alpha, ma, sl, mu, fallback, fp64form)
        _cases[(n, d)] = (res, X, Xs, slow, fp64, on32, on64)
    return _cases[(n, d)]


def path_ratios(err, sl, masks):
    out = {}
    for name, mk in masks.items():
        if mk.any():
            mt = torch.tensor(mk, device=DEV)
            out[name] = float((err[mt] / sl[mt].clamp_min(1e-300)).max())
    return out


@pytest.mark.parametrize("n,d", [(300, 5), (300, 8), (640, 5), (640, 8), (300, 3), (300, 16)])
def test_bound_holds_on_all_three_paths(engine, n, d):
    res, X, Xs, slow, fp64, on32, on64 = run_case(engine, n, d)
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
    res, X, Xs, slow, fp64, on32, on64 = run_case(engine, n, d)
    alpha, ma, sl, mu, _, _ = res["fitted"]
    fact = on32 | on64
    okp = O.KernelParams(O.RBF, np.full(d, botorch_default_lengthscale(d)))
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
        mu = mu_exact(kstar_mu(engine, kp, Xd, alpha, Xsd, m), m)
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
