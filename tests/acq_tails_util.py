"""Input ladders, metrics and the recorded fp64 baselines of the acquisition-arithmetic tests against the mpmath reference
(tests/mp_acq_ref.py): shared by tests/test_acq_ref_host.py, which measures the CPU forms on them, and
tests/test_gpu_acq_tails.py, which holds the device to four times those measurements on the same ladders.

Analytic ladder.  One RBF training point at 0 (lengthscale 1, target 0.7), 2048 candidates on [0, 6]: 1024 evenly spaced
(k* from 1 down to 1.5e-8; the first one is the training point, where the noise-free model's variance lands on the
1e-10 floor) and 1024 in [2, 2.05], where the moments move by ~1e-5 of themselves per candidate.  A call's best_f is
set from the moments themselves so that a chosen candidate sits at a target u = (mu - best_f) / sigma: the candidate in
the middle of the dense stretch for the targets whose neighbourhood matters (0, the joins of log_ei_helper's branches
-1 and -1024, and -1/sqrt(eps) = -67108864, BoTorch's hand-over to the asymptotic form, are crossed with steps far below
1e-3 of |u|), the candidate of smallest sigma for the deepest ones, so that no other
candidate lies deeper.  The other candidates of the call spread over the ratio of the sigmas, a factor 1e2 (noise 1e-4)
to 1e5 (noise 0), which fills the decades between the targets.

MC ladder.  One q-batch per call from the generators of tests/mc_acq_ref.py / tests/mc_nei_ref.py, the incumbent placed
from the fp64 samples themselves: at the median, above every sample by 1e-5 .. 1e3 and below by the same, the
covariance scaled by 1e-12 and 1e6, tau_max 1e-2 and 1e-4, one batch that needs the 1e-8 jitter, one whose y all lie in
(-31, -30) and one whose y straddle -37 (the plain form's branch), both with mean 0 so that y is known to ~30 eps.
"""
import math

import mpmath as mp
import numpy as np
import torch

from bayesianoptimizer_amd import acqf
from bayesianoptimizer_amd.engine import KernelParams
from bayesianoptimizer_amd.models import ExactGP
from oracle import gp_oracle as O
from tests import mc_acq_ref as R
from tests import mc_nei_ref as N
from tests import mp_acq_ref as M

EPS = 2.0 ** -52
DENORM = 5e-324  # one quantum of the denormal range
TINY = 2.0 ** -1022  # smallest normal double

# ---- recorded baselines: largest deviation of the fp64 CPU forms from mp on these ladders, in units of EPS ----------
# Measured by tests/test_acq_ref_host.py (which prints them and asserts them against these caps: the measurement plus
# one or two eps of slack); repeated in DESIGN.md §4.  The device bounds are 4 x these, never below FLOOR_EPS.
FLOOR_EPS = 16.0
CAP_ANALYTIC_EPS = {"logei": 8.0, "ucb": 2.0, "ei": 29.0, "logei_join": 46.0}  # measured 6.50, 0.97, 27.38, 44.20
# "logei_join": the absolute error of LogEI over every candidate with u in [-3, -1) (analytic_baseline).  There the
# score is ~ -2 .. -8, so the ladder's metric |err| / (1 + |ref|) with its floor of 16 eps would pass a form that loses
# three times the digits of the erfcx form (the log of the sum taken further down than -1: its two terms each carry
# u^2 / 2 eps from the rounding of their arguments before they cancel; 102 eps against the erfcx form's 30 near -3).
# The cancellation 1 - e^w multiplies the device's and the oracle's errors by the same factor and is already in the
# measured figure, so the device is allowed twice it, not four times: the factor covers only the difference between
# two libms' erfcx, log and expm1, a few ulp each, and has to stay below the factor three that it is there to resolve.
JOIN_FACTOR = 2.0
# acqf's analytic classes on the oracle engine (measured values 3.98, 11.61, 0.61; gradients 209348, 702033, 363.1: the
# derivative of the one-point posterior variance 1 - k^2 / (1 + noise) cancels, and d logEI / du carries u^2 eps)
CAP_TORCH_EPS = {"value": {"logei": 5.0, "ei": 13.0, "ucb": 2.0},
                 "grad": {"logei": 209350.0, "ei": 702035.0, "ucb": 365.0}}
# per call of the MC ladders, largest over q, S and the four qLogEI modes (over q, nb, S for the noisy form).  The
# largest over the shapes and not each shape's own figure: on the ill-conditioned calls the error is the rounding of f
# magnified, a draw from one distribution for the reference and the device alike, and a draw exceeds four times another
# draw about one time in six; it does not exceed four times the largest of a dozen.  The large
# entries are conditioning, not arithmetic: y = (f - best_f) / tau_relu turns the rounding of f, eps |f|, into
# eps |f| / tau_relu, and a small tau_max or a nearly singular covariance multiplies the gradients' once more.
CAP_MC_EPS = {
    "above 0.001": {"gcov": 480, "gmean": 480, "value": 460},
    "above 1": {"gcov": 540, "gmean": 460, "value": 3},
    "above 1000": {"gcov": 8700, "gmean": 830, "value": 3},
    "above 1e-05": {"gcov": 91000, "gmean": 91000, "value": 18000},
    "below 0.001": {"gcov": 33, "gmean": 16, "value": 5},
    "below 1": {"gcov": 81, "gmean": 21, "value": 5},
    "below 1000": {"gcov": 6000, "gmean": 320, "value": 3},
    "below 1e-05": {"gcov": 220, "gmean": 15, "value": 7},
    "cov 1e-12 above 1": {"gcov": 1.1e+06, "gmean": 260000, "value": 3},
    "cov 1e-12 above 1e-5": {"gcov": 1.5e+06, "gmean": 38000, "value": 8300},
    "cov 1e-12 below 1e-3": {"gcov": 50, "gmean": 17, "value": 6},
    "cov 1e-12 median": {"gcov": 1.6e+06, "gmean": 7400, "value": 500},
    "cov 1e6 above 1e-5": {"gcov": 5.6e+07, "gmean": 5.6e+07, "value": 1.1e+07},
    "cov 1e6 above 1e3": {"gcov": 320, "gmean": 230, "value": 3},
    "cov 1e6 below 1e3": {"gcov": 910, "gmean": 230, "value": 3},
    "cov 1e6 median": {"gcov": 52, "gmean": 44, "value": 4},
    "jitter 1e-8": {"gcov": 7.1e+06, "gmean": 3400, "value": 320},
    "mean 0 cov 1e-12 y across -37 q=1": {"gcov": 350, "gmean": 16, "value": 3},
    "mean 0 cov 1e-14 y in (-31, -30) q=1": {"gcov": 960, "gmean": 16, "value": 3},
    "median": {"gcov": 6, "gmean": 4, "value": 5},
    "tau_max 1e-4 above 1": {"gcov": 18, "gmean": 14, "value": 3},
    "tau_max 1e-4 above 1e-3": {"gcov": 470, "gmean": 470, "value": 460},
    "tau_max 1e-4 below 1e-3": {"gcov": 24, "gmean": 5, "value": 4},
    "tau_max 1e-4 median": {"gcov": 6, "gmean": 4, "value": 5},
    "mean 0 cov 1e-12 y across -37 q=2": {"gcov": 1100, "gmean": 350, "value": 3},
    "mean 0 cov 1e-14 y in (-31, -30) q=2": {"gcov": 5100, "gmean": 860, "value": 3},
    "mean 0 cov 1e-12 y across -37 q=3": {"gcov": 1200, "gmean": 2000, "value": 3},
    "mean 0 cov 1e-14 y in (-31, -30) q=3": {"gcov": 5200, "gmean": 1600, "value": 3},
}
CAP_NEI_EPS = {
    "best above 0.001": {"lognei gcov": 1100, "lognei gcross": 1100, "lognei gmean": 1100, "lognei value": 65, "nei gcov": 2, "nei gcross": 2, "nei gmean": 2, "nei value": 2},
    "best above 1": {"lognei gcov": 18, "lognei gcross": 21, "lognei gmean": 20, "lognei value": 3, "nei gcov": 2, "nei gcross": 2, "nei gmean": 2, "nei value": 2},
    "best above 1000": {"lognei gcov": 5200, "lognei gcross": 3000, "lognei gmean": 990, "lognei value": 3, "nei gcov": 2, "nei gcross": 2, "nei gmean": 2, "nei value": 2},
    "best above 1e-05": {"lognei gcov": 210000, "lognei gcross": 210000, "lognei gmean": 210000, "lognei value": 11000, "nei gcov": 2, "nei gcross": 2, "nei gmean": 2, "nei value": 2},
    "best below 0.001": {"lognei gcov": 23, "lognei gcross": 22, "lognei gmean": 7, "lognei value": 6, "nei gcov": 8, "nei gcross": 11, "nei gmean": 3, "nei value": 3},
    "best below 1": {"lognei gcov": 40, "lognei gcross": 15, "lognei gmean": 11, "lognei value": 5, "nei gcov": 8, "nei gcross": 11, "nei gmean": 3, "nei value": 3},
    "best below 1000": {"lognei gcov": 4200, "lognei gcross": 2500, "lognei gmean": 300, "lognei value": 3, "nei gcov": 8, "nei gcross": 11, "nei gmean": 3, "nei value": 3},
    "best below 1e-05": {"lognei gcov": 1700, "lognei gcross": 120, "lognei gmean": 35, "lognei value": 5, "nei gcov": 8, "nei gcross": 11, "nei gmean": 3, "nei value": 3},
    "cov 1e-12 best above 1e-5": {"lognei gcov": 4.7e+06, "lognei gcross": 390000, "lognei gmean": 46000, "lognei value": 2400, "nei gcov": 2, "nei gcross": 2, "nei gmean": 2, "nei value": 2},
    "cov 1e-12 best below 1e-3": {"lognei gcov": 230, "lognei gcross": 230, "lognei gmean": 230, "lognei value": 31, "nei gcov": 6, "nei gcross": 7, "nei gmean": 2, "nei value": 3},
    "cov 1e-12 natural": {"lognei gcov": 250, "lognei gcross": 88, "lognei gmean": 7, "lognei value": 6, "nei gcov": 6, "nei gcross": 7, "nei gmean": 2, "nei value": 3},
    "cov 1e6 best above 1e3": {"lognei gcov": 140, "lognei gcross": 67, "lognei gmean": 30, "lognei value": 3, "nei gcov": 2, "nei gcross": 2, "nei gmean": 2, "nei value": 2},
    "cov 1e6 natural": {"lognei gcov": 110, "lognei gcross": 200, "lognei gmean": 89, "lognei value": 4, "nei gcov": 7, "nei gcross": 8, "nei gmean": 3, "nei value": 6},
    "jitter 1e-8": {"lognei gcov": 7.1e+06, "lognei gcross": 760, "lognei gmean": 760, "lognei value": 720, "nei gcov": 7.1e+06, "nei gcross": 3, "nei gmean": 3, "nei value": 370},
    "natural": {"lognei gcov": 18, "lognei gcross": 18, "lognei gmean": 18, "lognei value": 7, "nei gcov": 8, "nei gcross": 11, "nei gmean": 3, "nei value": 3},
    "tau_max 1e-4 best above 1e-3": {"lognei gcov": 1100, "lognei gcross": 1100, "lognei gmean": 1100, "lognei value": 64, "nei gcov": 2, "nei gcross": 2, "nei gmean": 2, "nei value": 2},
    "tau_max 1e-4 natural": {"lognei gcov": 18, "lognei gcross": 18, "lognei gmean": 18, "lognei value": 7, "nei gcov": 8, "nei gcross": 11, "nei gmean": 3, "nei value": 3},
}


def device_bound_eps(cap_eps):
    """four times the CPU baseline, never below 16 eps: the device's libm functions each carry a few ulp of their own
    and compose three deep"""
    return max(4.0 * cap_eps, FLOOR_EPS)


# ---- analytic ladder --------------------------------------------------------------------------------------------------
X0, Y0, LENGTHSCALE = 0.0, 0.7, 1.0
NOISES = (1e-4, 0.0)
Y_SCALES = (1e-6, 1.0, 1e6)
Y_MEAN = 0.25
M_CAND = 2048
BETAS = (3.0, 4.0)
U_OVERFLOW = -1e160  # u * u overflows: LogEI is -inf by design


def candidates():
    x = np.concatenate([np.linspace(0.0, 6.0, M_CAND // 2), np.linspace(2.0, 2.05, M_CAND // 2)])
    return np.sort(x).reshape(-1, 1)


def anchors(var):
    """(index in the middle of the dense stretch, index of the smallest variance)"""
    x = candidates()[:, 0]
    dense = np.flatnonzero((x >= 2.0) & (x <= 2.05))
    return int(dense[len(dense) // 2]), int(np.argmin(var))


# (target u, anchor: 0 dense middle / 1 smallest sigma)
U_TARGETS = [(1e8, 0), (1e7, 0), (1e6, 0), (1e4, 0), (30.0, 0), (1.0, 0), (0.1, 0), (1e-2, 0), (1e-3, 0), (0.0, 0), (-0.5, 0), (-1.0, 0), (-3.0, 0), (-10.0, 0),
             (-30.0, 0), (-37.0, 0), (-38.5, 0), (-1e3, 0), (-1024.0, 0), (-1e5, 0), (-67108864.0, 0), (-1e10, 1), (-1e30, 1),
             (-1e100, 1), (-1e150, 1)]


def analytic_calls(mu, var):
    """[(target u, anchor index, best_f)] for one configuration's moments (arrays of M_CAND doubles)"""
    a = anchors(var)
    out = []
    for u_t, which in U_TARGETS:
        j = a[which]
        out.append((u_t, j, float(mu[j] - u_t * math.sqrt(var[j]))))
    return out


def mp_subset(u_t, j):
    """the candidates evaluated in mp for a call: the anchor, its neighbours, both ends and an even spread; fewer for
    the deepest targets, whose points cost hundreds of digits each"""
    if abs(u_t) > 1e9:
        idx = {0, 1, j - 1, j, j + 1, M_CAND // 4, M_CAND - 1}
    else:
        idx = set(range(j - 6, j + 7)) | set(range(0, M_CAND, 64)) | {1, 2, M_CAND - 1}
    return np.array(sorted(i for i in idx if 0 <= i < M_CAND))


_points = {}


def mp_point(mu, var, best_f):
    """mp quantities of one point, cached by the bits of its inputs (entry points that return the same moments share
    the evaluation)"""
    key = (float(mu), float(var), float(best_f))
    if key not in _points:
        _points[key] = M.analytic(*key)
    return _points[key]


def in_denormal_tail(p):
    """Phi(u) below the smallest normal double: EI's terms are denormal there and only the documented bounds hold
    (include/gpx.h, GPX_ACQ_EI)"""
    return p["Phi"] < TINY


def analytic_dev_eps(kind, got, mu, var, best_f, beta=4.0):
    """deviation of one score from mp in units of eps.
    logei, ucb: |got - ref| / (1 + |ref|).
    ei: |got - ref| / scale with scale = sigma phi(u) (1 + |u|), the size of the two terms that cancel for u < 0; for
    u > 0 nothing cancels, phi(u) vanishes and a correctly rounded sigma u is already off that scale, so the scale is
    never taken below |ref| (for u <= 0 this changes nothing: |ref| < sigma phi(u) there).  Below u = -30 four denormal
    quanta (times sigma where sigma > 1) are taken off the difference first."""
    got = float(got)
    if kind == "ucb":
        ref = M.ucb(mu, var, beta)
        return float(abs(mp.mpf(got) - ref) / (1 + abs(ref))) / EPS
    p = mp_point(mu, var, best_f)
    if kind == "logei":
        return float(abs(mp.mpf(got) - p["logei"]) / (1 + abs(p["logei"]))) / EPS
    diff = abs(mp.mpf(got) - p["ei"])
    if p["u"] < -30:
        diff = max(diff - 4 * DENORM * max(float(p["sigma"]), 1.0), mp.mpf(0))
    scale = max(p["sigma"] * p["phi"] * (1 + abs(p["u"])), abs(p["ei"]))
    if scale == 0:
        return 0.0 if diff == 0 else math.inf
    return float(diff / scale) / EPS


# ---- MC ladder --------------------------------------------------------------------------------------------------------
MODES = {"fatplus_fatmax": (True, True), "fatplus_lse": (True, False), "softplus_fatmax": (False, True),
         "softplus_lse": (False, False)}  # (fat_relu, fat_max), as tests/test_gpu_mc_acq.py
TAU_RELU = 1e-6
OFFSETS = (1e-5, 1e-3, 1.0, 1e3)


def _jitter_cov(q):
    """needs the 1e-8 jitter: q = 1 a variance of -1e-9; else a second pivot of 1 - (1 + 1e-9)^2 = -2e-9"""
    if q == 1:
        return torch.tensor([[[-1e-9]]], dtype=torch.float64)
    c = torch.eye(q, dtype=torch.float64)
    c[0, 1] = c[1, 0] = 1.0 + 1e-9
    return c.unsqueeze(0)


def _samples(mean, cov, z):
    L = torch.linalg.cholesky(0.5 * (cov + cov.transpose(1, 2)))
    return mean.unsqueeze(0) + torch.einsum("bij,sj->sbi", L, z)


_mc = {}


def mc_calls(q, S):
    """[dict(label, mean (1, q), cov (1, q, q), z (S, q), best_f, tau_max)] of the qLogEI ladder; never modified"""
    if (q, S) in _mc:
        return _mc[(q, S)]
    mean, cov = R.synthetic_moments(1, q, seed=40 + q)
    z = R.base_samples(S, q, seed=50 + S)
    calls = []

    def add(label, mean_, cov_, best_f, tau_max=1e-2):
        calls.append(dict(label=label, mean=mean_, cov=cov_, z=z, best_f=float(best_f), tau_max=tau_max))

    f = _samples(mean, cov, z)
    add("median", mean, cov, mean.median())
    for o in OFFSETS:
        add(f"above {o:g}", mean, cov, f.max() + o)
        add(f"below {o:g}", mean, cov, f.min() - o)
    add("tau_max 1e-4 median", mean, cov, mean.median(), 1e-4)
    add("tau_max 1e-4 above 1e-3", mean, cov, f.max() + 1e-3, 1e-4)
    add("tau_max 1e-4 below 1e-3", mean, cov, f.min() - 1e-3, 1e-4)
    add("tau_max 1e-4 above 1", mean, cov, f.max() + 1.0, 1e-4)
    small = cov * 1e-12
    fs = _samples(mean, small, z)
    add("cov 1e-12 median", mean, small, mean.median())
    add("cov 1e-12 above 1e-5", mean, small, fs.max() + 1e-5)
    add("cov 1e-12 below 1e-3", mean, small, fs.min() - 1e-3)
    add("cov 1e-12 above 1", mean, small, fs.max() + 1.0)
    # mean 0: f and best_f are a few 1e-5 at most, so y = (f - best_f) / tau_relu carries ~30 eps and not eps / tau_relu;
    # the q-reduction multiplies that by 1 / tau_max from q = 2 on, so these two carry q in their label (and their cap)
    zero = torch.zeros_like(mean)
    ff = _samples(zero, cov * 1e-14, z)
    add(f"mean 0 cov 1e-14 y in (-31, -30) q={q}", zero, cov * 1e-14, ff.max() + 30.05e-6)
    ff = _samples(zero, small, z)
    add(f"mean 0 cov 1e-12 y across -37 q={q}", zero, small, ff.median() + 37e-6)
    big = cov * 1e6
    fb = _samples(mean, big, z)
    add("cov 1e6 median", mean, big, mean.median())
    add("cov 1e6 above 1e3", mean, big, fb.max() + 1e3)
    add("cov 1e6 below 1e3", mean, big, fb.min() - 1e3)
    add("cov 1e6 above 1e-5", mean, big, fb.max() + 1e-5)
    add("jitter 1e-8", mean, _jitter_cov(q), mean.median())
    _mc[(q, S)] = calls
    return calls


def call_y(call):
    """y = (f - best_f) / tau_relu of a qLogEI call's fp64 samples (jitter-free batches)"""
    return (_samples(call["mean"], call["cov"], call["z"]) - call["best_f"]) / TAU_RELU


NEI_MODES = {"nei": dict(log=False), "lognei": dict(log=True, fat_relu=True, fat_max=True)}
_nei = {}


def nei_calls(q, nb, S):
    """[dict(label, args = (mean, cov, cross, Linv, zb, best, zq), tau_max)] of the noisy ladder: the per-sample
    incumbent plays best_f's part, so the baseline's mean is shifted instead (best_s moves with it)"""
    if (q, nb, S) in _nei:
        return _nei[(q, nb, S)]
    mu_b, cov_bb, mean, cov, cross = N.synthetic(1, q, nb)
    zb, zq = N.base_samples(S, nb, q)
    calls = []

    def gap(c):
        """(largest, smallest) f_si - best_s over the samples with the joint covariance scaled by c"""
        Linv, best = N.setup(mu_b, cov_bb * c, zb)
        A, D = N.conditional(cov * c, cross * c, Linv)
        f = mean.unsqueeze(0) + torch.einsum("bij,sj->sbi", A, zb) + torch.einsum(
            "bij,sj->sbi", torch.linalg.cholesky(D), zq)
        d = f - best.view(-1, 1, 1)
        return float(d.max()), float(d.min())

    def add(label, c, shift, tau_max=1e-2, cov_=None, cross_=None):
        Linv, best = N.setup(mu_b + shift, cov_bb * c, zb)
        calls.append(dict(label=label, tau_max=tau_max, args=(
            mean, cov * c if cov_ is None else cov_, cross * c if cross_ is None else cross_, Linv, zb, best, zq)))

    hi, lo = gap(1.0)
    add("natural", 1.0, 0.0)
    for o in OFFSETS:
        add(f"best above {o:g}", 1.0, hi + o)
        add(f"best below {o:g}", 1.0, lo - o)
    add("tau_max 1e-4 natural", 1.0, 0.0, 1e-4)
    add("tau_max 1e-4 best above 1e-3", 1.0, hi + 1e-3, 1e-4)
    hi_s, lo_s = gap(1e-12)
    add("cov 1e-12 natural", 1e-12, 0.0)
    add("cov 1e-12 best above 1e-5", 1e-12, hi_s + 1e-5)
    add("cov 1e-12 best below 1e-3", 1e-12, lo_s - 1e-3)
    hi_b, lo_b = gap(1e6)
    add("cov 1e6 natural", 1e6, 0.0)
    add("cov 1e6 best above 1e3", 1e6, hi_b + 1e3)
    add("jitter 1e-8", 1.0, 0.0, cov_=_jitter_cov(q), cross_=torch.zeros_like(cross))
    _nei[(q, nb, S)] = calls
    return calls


# ---- MC metrics (tests/test_gpu_mc_acq.py's) against mp --------------------------------------------------------------
def value_dev_eps(got, ref):
    """|got - ref| / (1 + |ref|) in eps; got a double, ref an mpmath number"""
    return float(abs(mp.mpf(float(got)) - ref) / (1 + abs(ref))) / EPS


def grad_dev_eps(got, ref):
    """norm-wise deviation of one q-batch's gradient max|g - ref| / max|ref| in eps; got an array, ref nested lists of
    mpmath numbers.  A gradient that is zero throughout (no sample improves: plain NEI) must be returned as zeros."""
    g = np.asarray(got, dtype=np.float64).reshape(-1)
    r = [v for row in ref for v in (row if isinstance(row, list) else [row])]
    num = max(abs(mp.mpf(float(a)) - b) for a, b in zip(g, r))
    den = max(abs(b) for b in r)
    if den == 0:
        return 0.0 if num == 0 else math.inf
    return float(num / den) / EPS


def mc_ref(call, mode, info):
    """(value, gmean, gcov) of one qLogEI call in mp (lists over its single batch)"""
    fat_relu, fat_max = MODES[mode]
    return M.mc_acq(call["mean"].tolist(), call["cov"].tolist(), call["z"].tolist(), info, call["best_f"], fat_relu,
                    fat_max, TAU_RELU, call["tau_max"])


def nei_ref(call, mode, info):
    """(value, gmean, gcov, gcross) of one noisy call in mp"""
    kw = dict(fat_relu=True, fat_max=True)
    kw.update(NEI_MODES[mode])
    return M.mc_nei(*(a.tolist() for a in call["args"]), info, tau_relu=TAU_RELU, tau_max=call["tau_max"], **kw)


# ---- torch side: a dozen points of the one-point model over the u ladder ---------------------------------------------
TORCH_X = (0.05, 0.3, 0.8, 1.3, 2.0, 2.7, 3.5, 4.5)
TORCH_U = (1e4, 1.0, 0.0, -0.999, -1.001, -10.0, -37.0, -1e3, -1e5, -67108863.0, -67108865.0, -1e10)
TORCH_NOISE = 1e-4


def torch_model_kwargs():
    return dict(x0=X0, y0=Y0, lengthscale=LENGTHSCALE, outputscale=1.0, noise=TORCH_NOISE)


def torch_points():
    """[(x, best_f)]: point k of the ladder sits at u = TORCH_U[k] under the closed-form posterior"""
    out = []
    for k, u in enumerate(TORCH_U):
        x = TORCH_X[k % len(TORCH_X)]
        with mp.workdps(40):
            mu, var = M.one_point_posterior(mp.mpf(x), **torch_model_kwargs())
            out.append((x, float(mu - mp.mpf(u) * mp.sqrt(var))))
    return out

# ---- shared checks ------------------------------------------------------------------------------------------------------
ORACLE_KINDS = {"ei": O.ACQ_EI, "logei": O.ACQ_LOGEI, "ucb": O.ACQ_UCB}


def check_ei_tail(got, p):
    """the documented behaviour where EI's terms are denormal (include/gpx.h): 0 <= EI <= sigma phi(u), to rounding"""
    sigma, bound = float(p["sigma"]), float(p["sigma"] * p["phi"])
    assert 0.0 <= got <= bound * (1 + 4 * EPS) + 4 * DENORM * max(sigma, 1.0), (got, bound, float(p["u"]))


JOIN_TARGETS = (-1.0, -3.0)


def analytic_baseline(mu, var, score):
    """largest deviation in eps per kind over a configuration's ladder; ``score(kind, best_f, beta)``: all M_CAND
    scores.  Every score is finite or the documented -inf / 0, EI is non-negative.  "logei_join": the largest absolute
    error of LogEI in eps over EVERY candidate with u in [-3, -1) of the calls aimed at -1 and -3, the stretch below
    the join of log_ei_helper's first two branches (see JOIN_FACTOR).  Returns (worst, u of the points compared)."""
    worst = {"ei": 0.0, "logei": 0.0, "ucb": 0.0, "logei_join": 0.0}
    us = []
    for u_t, j, best_f in analytic_calls(mu, var):
        idx = mp_subset(u_t, j)
        for kind in ("ei", "logei"):
            s = score(kind, best_f, 4.0)
            assert not np.isnan(s).any(), (kind, u_t)
            if kind == "ei":
                assert (s >= 0).all(), u_t
            for i in idx:
                p = mp_point(mu[i], var[i], best_f)
                if kind == "ei" and in_denormal_tail(p):
                    check_ei_tail(float(s[i]), p)
                    continue
                d = analytic_dev_eps(kind, s[i], mu[i], var[i], best_f)
                worst[kind] = max(worst[kind], d)
            if kind == "logei" and u_t in JOIN_TARGETS:
                uu = (mu - best_f) / np.sqrt(var)
                for i in np.flatnonzero((uu >= -3.0) & (uu < -1.0)):
                    d = float(abs(mp.mpf(float(s[i])) - mp_point(mu[i], var[i], best_f)["logei"])) / EPS
                    worst["logei_join"] = max(worst["logei_join"], d)
        us += [float(mp_point(mu[i], var[i], best_f)["u"]) for i in idx]
    for beta in BETAS:
        s = score("ucb", 0.0, beta)
        for i in range(0, M_CAND, 16):
            worst["ucb"] = max(worst["ucb"], analytic_dev_eps("ucb", s[i], mu[i], var[i], 0.0, beta))
    return worst, np.array(us)


def ladder_u(mu, var):
    """u in fp64 of the points analytic_baseline compares with mp for these moments"""
    sigma = np.sqrt(var)
    return np.concatenate([(mu[idx] - best_f) / sigma[idx] for u_t, j, best_f in analytic_calls(mu, var)
                           for idx in (mp_subset(u_t, j),)])


def check_u_coverage(us):
    """what the ladder promises, on the u of the points evaluated in mp (pooled over the configurations)"""
    us = np.sort(us)
    assert us.max() >= 1e8 and us.min() <= -0.99e150 and us.min() > -1.01e150
    assert ((us > 0) & (us < 2e-3)).any() and ((us < 0) & (us > -1e-3)).any()  # 0 crossed
    for b in (-1.0, -1024.0, -67108864.0):  # crossed with steps of at most 1e-3 |b|
        near = us[(us > b * (1 + 1e-3)) & (us < b * (1 - 1e-3))]
        assert (near > b).any() and (near < b).any() and np.diff(near).max() <= 1e-3 * abs(b)
    lg = np.log10(-us[(us < -1) & (us > -6.7e7)])  # log-spaced in between: no gap of a decade
    assert np.diff(lg).max() < 1.0
    assert ((us < -37.6) & (us > -39)).any() and ((us < -30) & (us > -37.4)).any()
    pos = us[(us >= 0.99e-3) & (us <= 1.01e8)]  # [1e-3, 1e8]: both ends and no gap of a decade
    assert pos.min() <= 1.01e-3 and pos.max() >= 0.99e8 and np.diff(np.log10(pos)).max() < 1.0


# ---- the acqf classes on an engine against the closed-form one-point model ---------------------------------------
def torch_side_devs(engine, device):
    """(largest value deviation, largest gradient deviation) in eps of acqf's analytic classes on the one-point model
    over the torch ladder.  Values: against mp at the engine's own moments (the special functions alone).  Gradients:
    d value / dx through autograd against mp.diff of the mp score composed with the closed-form mp posterior,
    relative to that derivative (this one includes the engine's posterior and its derivative)."""
    kp = KernelParams("rbf", LENGTHSCALE, noise=TORCH_NOISE)
    gp = ExactGP(np.array([[X0]]), np.array([[Y0]]), kp, engine=engine).fit()
    classes = {"logei": acqf.LogExpectedImprovement, "ei": acqf.ExpectedImprovement, "ucb": acqf.UpperConfidenceBound}
    model = torch_model_kwargs()
    worst_v, worst_g = {}, {}
    for kind, cls in classes.items():
        for x, best_f in torch_points():
            a = cls(gp, best_f=best_f, beta=3.0)
            X = torch.tensor([[[x]]], dtype=torch.float64, device=device, requires_grad=True)
            val = a(X)
            (g,) = torch.autograd.grad(val.sum(), X)
            assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(g).all()), (kind, x, best_f)
            with torch.no_grad():
                mu, cov = acqf.posterior_moments(gp, X.detach(), a.objective, floor_terms=True)
            mu_d, var_d = float(mu[0, 0]), float(cov[0, 0, 0])
            p = mp_point(mu_d, var_d, best_f)
            if kind == "ei" and in_denormal_tail(p):
                check_ei_tail(float(val.detach()), p)
            else:
                d = analytic_dev_eps(kind, float(val.detach()), mu_d, var_d, best_f, 3.0)
                worst_v[kind] = max(worst_v.get(kind, 0.0), d)
            ref_v, ref_g = M.one_point_score_and_grad(kind, x, best_f, 3.0, model)
            if kind == "ei" and in_denormal_tail(p):
                continue
            if ref_g == 0:
                assert float(g) == 0.0
                continue
            dg = float(abs(mp.mpf(float(g)) - ref_g) / abs(ref_g)) / EPS
            worst_g[kind] = max(worst_g.get(kind, 0.0), dg)
    return worst_v, worst_g
