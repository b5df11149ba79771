"""Arbitrary-precision reference of the acquisition arithmetic, written from the mathematical definitions with mpmath.

Imports nothing from bayesianoptimizer_amd or oracle.  Inputs are taken as the exact doubles they are; results are
mpmath numbers (``float(...)`` rounds them once).

Analytic part: with sigma = sqrt(var), u = (mu - best_f) / sigma,
    ei = sigma (phi(u) + u Phi(u)),  logei = log ei,  ucb = mu + sqrt(beta) sigma,  variance = var.
No erfcx form and no branch: the cancellation of phi(u) + u Phi(u) for u << 0 (the sum is ~ phi(u) / u^2) is paid for in
digits, chosen per point: 2 log10|u| for the cancellation and as many again because exp(-u^2 / 2) carries the rounding
of its argument, u^2 times the working epsilon.  The result is good to far better than 1e-25 relative
(tests/test_acq_ref_host.py re-evaluates a sample at twice the digits).

MC part: the forward definitions of gpx_mc_acq_f64 / gpx_mc_nei_f64 (include/gpx.h; tests/mc_acq_ref.py and
tests/mc_nei_ref.py are their fp64 torch forms) on mpmath numbers, for q <= 3 and S <= 8 (the reference's limit, not the
kernels').  The jitter of a q-batch is the one the fp64 reference selected (``info``): the retry ladder is a property of
fp64 arithmetic and is not redone here.  Gradients with respect to the mean, the covariance (each entry on its own,
through the symmetrisation) and the cross-covariance are mpmath's numerical derivatives of the forward, not a
hand-derived backward.
"""
import math

import mpmath as mp

BASE_DPS = 50  # digits kept beyond the cancellation
JITTERS = (0.0, 1e-8, 1e-7, 1e-6)
MAX_Q, MAX_S = 3, 8


# ---- analytic ---------------------------------------------------------------------------------------------------------
def analytic_dps(mu, var, best_f, extra=0):
    """working digits for one point: BASE_DPS + 4 log10|u| (see the module's docstring) + extra"""
    with mp.workdps(40):
        u = (mp.mpf(mu) - mp.mpf(best_f)) / mp.sqrt(mp.mpf(var))
        lg = int(mp.ceil(mp.log10(abs(u)))) if abs(u) > 1 else 0
    return BASE_DPS + 4 * lg + extra


def u_sigma(mu, var, best_f):
    sigma = mp.sqrt(mp.mpf(var))
    return (mp.mpf(mu) - mp.mpf(best_f)) / sigma, sigma


def ei_helper(u):
    """phi(u) + u Phi(u), at the precision of the context"""
    return mp.npdf(u) + u * mp.ncdf(u)


def analytic(mu, var, best_f, dps=None):
    """dict(u, sigma, phi, Phi, ei, logei) of one point at ``dps`` digits (default: analytic_dps)"""
    with mp.workdps(analytic_dps(mu, var, best_f) if dps is None else dps):
        u, sigma = u_sigma(mu, var, best_f)
        h = ei_helper(u)
        return {"u": u, "sigma": sigma, "phi": mp.npdf(u), "Phi": mp.ncdf(u), "ei": sigma * h,
                "logei": mp.log(h) + mp.log(sigma)}


def ei(mu, var, best_f, dps=None):
    return analytic(mu, var, best_f, dps)["ei"]


def logei(mu, var, best_f, dps=None):
    return analytic(mu, var, best_f, dps)["logei"]


def ucb(mu, var, beta):
    with mp.workdps(BASE_DPS):
        return mp.mpf(mu) + mp.sqrt(mp.mpf(beta)) * mp.sqrt(mp.mpf(var))


def variance(mu, var):
    return mp.mpf(var)


# ---- the one-point RBF model in closed form (n = 1, d = 1, training point x0 with target y0) ----------------------
def one_point_posterior(x, x0, y0, lengthscale, outputscale, noise, const_mean=0.0, floor_std=1e-10, floor=1e-12):
    """(mu, var) at x of the GP with one training point: k = s exp(-(x - x0)^2 / (2 l^2)), mu = m + k (y0 - m) /
    (s + noise), var = max(max(s - k^2 / (s + noise), floor_std), floor); x may be an mpmath number."""
    s, l_ = mp.mpf(outputscale), mp.mpf(lengthscale)
    r = (x - mp.mpf(x0)) / l_
    k = s * mp.exp(-r * r / 2)
    kk = s + mp.mpf(noise)
    mu = mp.mpf(const_mean) + k * (mp.mpf(y0) - mp.mpf(const_mean)) / kk
    var = s - k * k / kk
    var = var if var > floor_std else mp.mpf(floor_std)
    return mu, (var if var > floor else mp.mpf(floor))


def one_point_score(kind, x, best_f, beta, model, dps=None):
    """score of ``kind`` ("ei", "logei", "ucb") at x through the closed-form posterior; ``model``: the keyword
    arguments of one_point_posterior.  Differentiable by mp.diff in x."""
    with mp.workdps(dps or mp.mp.dps):
        mu, var = one_point_posterior(mp.mpf(x), **model)
        sigma = mp.sqrt(var)
        if kind == "ucb":
            return mu + mp.sqrt(mp.mpf(beta)) * sigma
        h = ei_helper((mu - mp.mpf(best_f)) / sigma)
        return sigma * h if kind == "ei" else mp.log(h) + mp.log(sigma)


def one_point_score_and_grad(kind, x, best_f, beta, model):
    """(value, d value / dx) with the digits chosen from u at x"""
    with mp.workdps(BASE_DPS):
        mu, var = one_point_posterior(mp.mpf(x), **model)
    dps = analytic_dps(float(mu), float(var), best_f, extra=20)
    with mp.workdps(dps):
        f = lambda t: one_point_score(kind, t, best_f, beta, model)  # noqa: E731
        return f(mp.mpf(x)), mp.diff(f, mp.mpf(x))


# ---- MC: forward definitions ------------------------------------------------------------------------------------------
def softplus(y):
    return mp.log1p(mp.exp(y))  # log(1 + e^y); log1p keeps e^y where it is far below one ulp of 1


def log_improvement(f, best, tau_relu, fat_relu):
    """log of the smoothed ReLU of f - best (include/gpx.h): with y = (f - best) / tau_relu,
    log tau_relu + log(softplus(y) + 0.1 / (1 + y^2)) (fat) or log tau_relu + log softplus(y), = y for y <= -37"""
    y = (f - best) / tau_relu
    if fat_relu:
        return mp.log(tau_relu) + mp.log(softplus(y) + mp.mpf(1) / 10 / (1 + y * y))
    return mp.log(tau_relu) + (mp.log(softplus(y)) if y > -37 else y)


def q_reduce(li, tau_max, fat_max):
    """fatmax (alpha = 2) or tau_max logsumexp over the q entries"""
    if fat_max:
        M = max(li)
        return M + tau_max * mp.log(mp.fsum((1 + (M - v) / (2 * tau_max)) ** -2 for v in li))
    M = max(li)  # the shift is exact mathematics (log sum exp(v / tau) = M / tau + log sum exp((v - M) / tau))
    return M + tau_max * mp.log(mp.fsum(mp.exp((v - M) / tau_max) for v in li))


def log_mean_exp(r):
    M = max(r)
    return M + mp.log(mp.fsum(mp.exp(v - M) for v in r) / len(r))


def _mat(rows):
    return [[mp.mpf(v) for v in row] for row in rows]


def _chol(A):
    q = len(A)
    L = mp.cholesky(mp.matrix(A))
    return [[L[i, j] for j in range(q)] for i in range(q)]


def _sym_jitter(cov, jitter):
    q = len(cov)
    return [[(cov[i][j] + cov[j][i]) / 2 + (jitter if i == j else 0) for j in range(q)] for i in range(q)]


def mc_acq_forward(mean, cov, z, jitter, best_f, fat_relu, fat_max, tau_relu, tau_max):
    """qLogEI value of one q-batch: mean (q), cov (q x q), z (S x q) as mpmath numbers"""
    q, S = len(mean), len(z)
    L = _chol(_sym_jitter(cov, jitter))
    r = []
    for s in range(S):
        f = [mean[i] + mp.fsum(L[i][j] * z[s][j] for j in range(i + 1)) for i in range(q)]
        r.append(q_reduce([log_improvement(fi, best_f, tau_relu, fat_relu) for fi in f], tau_max, fat_max))
    return log_mean_exp(r)


def mc_nei_forward(mean, cov, cross, Linv, zb, best, zq, jitter, log, fat_relu, fat_max, tau_relu, tau_max):
    """(log) noisy EI value of one q-batch conditioned on the baseline: A = cross Linv^T, D = sym(cov) - A A^T,
    f_s = mean + A zb_s + chol(D + jitter I) zq_s against the per-sample incumbent best_s (tests/mc_nei_ref.py)"""
    q, nb, S = len(mean), len(Linv), len(zq)
    A = [[mp.fsum(cross[i][k] * Linv[j][k] for k in range(nb)) for j in range(nb)] for i in range(q)]
    D = _sym_jitter(cov, 0)
    D = [[D[i][j] - mp.fsum(A[i][k] * A[j][k] for k in range(nb)) + (jitter if i == j else 0) for j in range(q)]
         for i in range(q)]
    L = _chol(D)
    r = []
    for s in range(S):
        f = [mean[i] + mp.fsum(A[i][k] * zb[s][k] for k in range(nb)) +
             mp.fsum(L[i][j] * zq[s][j] for j in range(i + 1)) for i in range(q)]
        if log:
            r.append(q_reduce([log_improvement(fi, best[s], tau_relu, fat_relu) for fi in f], tau_max, fat_max))
        else:
            r.append(max(max(f) - best[s], mp.mpf(0)))
    return log_mean_exp(r) if log else mp.fsum(r) / S


def _partial(fwd, a, idx, mirror=False):
    """d fwd / d a[idx] by mp.diff, the entry put back afterwards; ``mirror``: a[j][i] moves with a[i][j]"""
    i, j = idx if isinstance(idx, tuple) else (idx, None)
    x0 = a[i] if j is None else a[i][j]

    def put(t):
        if j is None:
            a[i] = t
        else:
            a[i][j] = t
            if mirror:
                a[j][i] = t

    def f(t):
        put(t)
        try:
            return fwd()
        finally:
            put(x0)
    return mp.diff(f, x0)


def _partials(fwd, vectors=(), matrices=(), symmetrised=()):
    """Gradients of fwd() with respect to every entry of the given nested lists.  ``symmetrised`` matrices enter fwd
    only through (C + C^T) / 2: the derivative with respect to one entry, the other held, is half the derivative of
    moving the pair together (the whole of it on the diagonal), so each pair is differentiated once."""
    out = [[_partial(fwd, v, i) for i in range(len(v))] for v in vectors]
    for m in matrices:
        out.append([[_partial(fwd, m, (i, j)) for j in range(len(m[i]))] for i in range(len(m))])
    for c in symmetrised:
        q = len(c)
        g = [[None] * q for _ in range(q)]
        for i in range(q):
            for j in range(i + 1):
                d = _partial(fwd, c, (i, j), mirror=True)
                g[i][j] = g[j][i] = d if i == j else d / 2
        out.append(g)
    return out


def _check_limits(q, S):
    if q > MAX_Q or S > MAX_S:
        raise ValueError(f"the mp reference is kept to q <= {MAX_Q}, S <= {MAX_S}")


def mc_acq(mean, cov, z, info, best_f, fat_relu, fat_max, tau_relu=1e-6, tau_max=1e-2, need_grad=True, dps=BASE_DPS):
    """Per q-batch of mean (B x q), cov (B x q x q) (nested lists / arrays of doubles), z (S x q): lists of the value,
    and with ``need_grad`` of d value / d mean (q) and d value / d cov (q x q); None for a batch with info < 0."""
    B, q, S = len(mean), len(mean[0]), len(z)
    _check_limits(q, S)
    values, gmeans, gcovs = [], [], []
    with mp.workdps(dps):
        zz = _mat(z)
        par = (mp.mpf(best_f), bool(fat_relu), bool(fat_max), mp.mpf(tau_relu), mp.mpf(tau_max))
        for b in range(B):
            if int(info[b]) < 0:
                values.append(None), gmeans.append(None), gcovs.append(None)
                continue
            m, c, jit = [mp.mpf(v) for v in mean[b]], _mat(cov[b]), mp.mpf(JITTERS[int(info[b])])
            fwd = lambda: mc_acq_forward(m, c, zz, jit, *par)  # noqa: E731
            values.append(fwd())
            if need_grad:
                gm, gc = _partials(fwd, vectors=[m], symmetrised=[c])
                gmeans.append(gm), gcovs.append(gc)
    return (values, gmeans, gcovs) if need_grad else values


def mc_nei(mean, cov, cross, Linv, zb, best, zq, info, log, fat_relu=True, fat_max=True, tau_relu=1e-6, tau_max=1e-2,
           need_grad=True, dps=BASE_DPS):
    """As mc_acq for the noisy form: cross (B x q x nb), Linv (nb x nb), zb (S x nb), best (S), zq (S x q); gradients
    d value / d mean, d cov, d cross."""
    B, q, S = len(mean), len(mean[0]), len(zq)
    _check_limits(q, S)
    values, gmeans, gcovs, gcross = [], [], [], []
    with mp.workdps(dps):
        Li, zbm, zqm, bs = _mat(Linv), _mat(zb), _mat(zq), [mp.mpf(v) for v in best]
        par = (bool(log), bool(fat_relu), bool(fat_max), mp.mpf(tau_relu), mp.mpf(tau_max))
        for b in range(B):
            if int(info[b]) < 0:
                values.append(None), gmeans.append(None), gcovs.append(None), gcross.append(None)
                continue
            m, c, x = [mp.mpf(v) for v in mean[b]], _mat(cov[b]), _mat(cross[b])
            jit = mp.mpf(JITTERS[int(info[b])])
            fwd = lambda: mc_nei_forward(m, c, x, Li, zbm, bs, zqm, jit, *par)  # noqa: E731
            values.append(fwd())
            if need_grad:
                gm, gx, gc = _partials(fwd, vectors=[m], matrices=[x], symmetrised=[c])
                gmeans.append(gm), gcovs.append(gc), gcross.append(gx)
    return (values, gmeans, gcovs, gcross) if need_grad else values


def to_float(x):
    """nested lists of mpmath numbers -> nested lists of doubles (None -> nan)"""
    if x is None:
        return math.nan
    if isinstance(x, list):
        return [to_float(v) for v in x]
    return float(x)
