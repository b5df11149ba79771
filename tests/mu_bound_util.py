"""Shared helpers of the head mean bound's GPU tests (gpx_mubound.hip): the ctypes wrappers of the debug entries
gpx_debug_kstar_mu_f64 and gpx_debug_mu_bound_f64, the exact mean in sum_partials' order, and the factorised forms'
geometry restated in numpy with the 3000 mixed candidates built from it.  A plain module (no fixtures, no tests)."""
import ctypes

import numpy as np
import torch

from bayesianoptimizer_amd import _capi

DEV = torch.device("cuda", 0)
Y_LIMIT = 16.0  # MUF_Y_LIMIT of gpx_mubound.hip
EPS32_LIMIT = 2.0 ** -18 * (1.0 - 2.0 ** -12)  # MUF32_EPS1_MAX (1 - 2^-12): the fp32 form's eligibility
LOG2E = 1.4426950408889634
RUN_TERMS = 11.0  # MUF32_RUN + 3: a run of 8 fp32 FMAs, v_exp_f32's 2 v and the rounding of alpha"
WG = 256
M = 3000
FP64FORM_BYTE = 160  # the second counter's offset in the aligned workspace (include/gpx.h)


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def ptr(a):
    return ctypes.c_void_p(a.data_ptr()) if a is not None else None


def kstar_mu(engine, kp, X, alpha, Xs, m, list_=None, count=None, mu_part=None, ldmu=0):
    """gpx_debug_kstar_mu_f64 -> (K*, mean partials)."""
    lib, n, d = engine.lib, X.shape[0], X.shape[1]
    npad = int(lib.gpx_padded_n(n))
    ld = (m + 255) // 256 * 256
    out = torch.full((npad, ld), float("nan"), dtype=torch.float64, device=DEV)
    if mu_part is None:
        mu_part = torch.full((npad // 64, ld), float("nan"), dtype=torch.float64, device=DEV)
    pc = kp.to_c(d)
    st = lib.gpx_debug_kstar_mu_f64(engine.handle, ctypes.byref(pc), n, ptr(X), X.stride(0), ptr(alpha), ptr(Xs), m,
                                    Xs.stride(0), ptr(list_), ptr(count), ptr(out), ld, ptr(mu_part), ldmu)
    _capi.check(st, engine.handle)
    torch.cuda.synchronize()
    return out, mu_part


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
    """The centre, max |a|^2, Y_c and eps1_32(c) of the factorised forms, restated in numpy.  ls: one lengthscale, or
    one per dimension (the kernels scale coordinate k by 1 / ls[k]; a scalar divides as it always did)."""

    def __init__(self, X, ls):
        self.n, self.d = X.shape
        self.ls = ls if np.ndim(ls) == 0 else np.asarray(ls, dtype=np.float64)
        assert np.ndim(ls) == 0 or self.ls.shape == (self.d,)
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
        if np.ndim(ls) == 0:
            assert fp64 == [3, 4], fp64
        else:
            # per-dimension lengthscales below the default stretch the unit cube: some of its workgroups leave the
            # fp32 form as well.  The rings stay where they were put, and every workgroup's largest eps1_32 is clear
            # of the limit, so that the device decides as these formulas do.
            assert 2 not in fp64 and 3 in fp64 and 4 in fp64, fp64
            for w in groups:
                if w not in slow:
                    worst = float(e[w * WG:(w + 1) * WG].max())
                    assert not 0.996 * EPS32_LIMIT < worst < 1.004 * EPS32_LIMIT, (w, worst / EPS32_LIMIT)
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
