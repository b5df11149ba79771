"""Host checks of the ARD recipe of tests/ard_util.py, which the GPU tests of the d-ladder use.

(1) Preconditions.  With the recipe's parameters and noise 1e-4 the oracle fits (positive definite, cond(K) <= 1e6) at
n = 100, 200 and 300 for every ladder d and kind, and over the tests' Sobol candidates the best oracle score is clear of
the runner-up by more than 1e3 times the argmax check's 1e-9 max(1, |best|), for all four acquisitions: an argmax
compared bit for bit is decided by the model, not by rounding.

(2) Sensitivity.  The yardsticks of the GPU tests reject an index mix-up.  A model built with two lengthscales (or two
linear variances) exchanged, consistently in every place they enter, is compared with the true one by each yardstick:
check_posterior of tests/test_gpu_parity.py, the q-batch gradient tolerances of tests/test_acqf.py, the SVGP
hyperparameter gradient's entry_ratio against TAU and the inducing-location gradient's ratio against TAUZ.  The swapped
pairs are (0, 1), (d - 2, d - 1) and, above 16 dimensions, (15, 16), which straddles the two 16-dimension sweeps of the
DMAX = 32 kernels.  Every disagreement must exceed its tolerance at least 100 times; the ratios are printed.
"""
import dataclasses

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import sgpr_grad_ref as G
from tests import sgpr_zgrad_ref as ZR
from tests.ard_util import ACQS, BETA, KINDS, LADDER, NOISE, ard_params, swap_pairs, swapped, sweep_problem
from tests.oracle_engine import to_oracle_params
from tests.test_gpu_parity import RTOL, check_posterior

MARGIN = 100.0
# the SVGP problem of every ladder d: sgpr_ref's shapes 3 (d = 5) and 4 (d = 8), sgpr_grad_ref.DSHAPES for the others
SVGP_SHAPE = {4: 104, 5: 3, 8: 4, 9: 109, 16: 116, 17: 117, 32: 132}


# ---- (1) the recipe's preconditions ---------------------------------------------------------------------------------
def test_recipe_values_are_pairwise_distinct():
    for d in (1,) + LADDER:
        for seed in (d, d + 1, d + 2):
            kp, op = ard_params("scale_linear_matern52", d, seed)
            ls, lv = np.sort(op.lengthscale), np.sort(op.linear_variance)
            assert len(ls) == len(lv) == d
            if d > 1:
                assert np.diff(ls).min() >= 0.99 / (d - 1) * O.botorch_default_lengthscale(d)
                assert np.diff(lv).min() >= 0.99 * 0.4 / (d - 1)
            assert kp.lengthscales(d) == list(op.lengthscale) and kp.linear_variances(d) == list(op.linear_variance)


@pytest.mark.parametrize("d", LADDER)
def test_oracle_fits_and_the_winner_is_clear(d):
    worst_cond, worst_gap = 0.0, np.inf
    for n, m in ((300, 5000), (200, 1500), (100, 1500)):  # the pruned sweeps' shape, the fused small-n sweeps' shapes
        X, y, Xs = sweep_problem(n, d, m)
        for kind in KINDS:
            _, op = ard_params(kind, d, d, noise=NOISE)
            K = O.gram(X, op)
            ost = O.fit(X, y, op)  # raises NotPDError if the Gram matrix is not positive definite
            worst_cond = max(worst_cond, float(np.linalg.cond(K)))
            mu, var = O.posterior(ost, Xs)
            for acq, kid in ACQS.items():
                s = np.sort(O.acquisition(mu, var, kid, float(y.max()), BETA))[::-1]
                gap = (s[0] - s[1]) / max(1.0, abs(s[0]))
                worst_gap = min(worst_gap, gap)
                assert gap > 1e3 * 1e-9, (n, kind, acq, gap)
    print(f"d = {d}: cond(K) <= {worst_cond:.2e}, smallest relative gap of the best score {worst_gap:.2e}")
    assert worst_cond <= 1e6


# ---- (2) the yardsticks reject two exchanged parameters -----------------------------------------------------------------
def posterior_ratios(mu_g, var_g, mu_r, var_r, kdiag):
    """check_posterior's two disagreements over their tolerances."""
    scale = max(np.abs(mu_r).max(), 1e-300)
    return np.abs(mu_g - mu_r).max() / (RTOL * scale), (np.abs(var_g - var_r) / (RTOL * kdiag + 1e-15)).max()


def moments_ratios(got, ref, outputscale):
    """The four disagreements of test_acqf.test_moments_grad_matches_oracle over their tolerances."""
    (mean, dmean, cov, dcov), (rm, rdm, rc, rdc) = got, ref
    return (np.abs(mean - rm).max() / (1e-9 * np.abs(rm).max()), np.abs(dmean - rdm).max() / (1e-8 * np.abs(rdm).max()),
            np.abs(cov - rc).max() / (1e-9 * outputscale), np.abs(dcov - rdc).max() / (1e-8 * np.abs(rdc).max()))


def swaps(kind, d):
    """(what, i, j) of every exchange that changes a kernel of this kind."""
    whats = ["lengthscale"] + (["linear_variance"] if kind == "scale_linear_matern52" else [])
    return [(w, i, j) for w in whats for i, j in swap_pairs(d)]


@pytest.mark.parametrize("d", LADDER)
def test_exact_gp_yardsticks_reject_exchanged_parameters(d):
    n, q = 200, 3
    X, y, Xs = sweep_problem(n, d, 1500)
    Xs = Xs[:300]
    for kind in KINDS:
        kp, op = ard_params(kind, d, d, noise=NOISE)
        ost = O.fit(X, y, op)
        mu_r, var_r = O.posterior(ost, Xs)
        kdiag = O.kernel_diag(Xs, op)
        mom_r = O.moments_grad(ost, Xs[:4 * q], q)
        for what, i, j in swaps(kind, d):
            wrong = to_oracle_params(swapped(kp, i, j, what), d)
            wst = O.fit(X, y, wrong)
            mu_w, var_w = O.posterior(wst, Xs)
            rp = posterior_ratios(mu_w, var_w, mu_r, var_r, kdiag)
            rm = moments_ratios(O.moments_grad(wst, Xs[:4 * q], q), mom_r, op.outputscale)
            print(f"d = {d} {kind} {what} ({i}, {j}): disagreement / tolerance: posterior mean {rp[0]:.1e} variance "
                  f"{rp[1]:.1e}; moments mean {rm[0]:.1e} dmean {rm[1]:.1e} cov {rm[2]:.1e} dcov {rm[3]:.1e}")
            assert min(rp) >= MARGIN and min(rm) >= MARGIN, (kind, what, i, j)
            with pytest.raises(AssertionError):
                check_posterior(mu_w, var_w, mu_r, var_r, kdiag)


@pytest.mark.parametrize("d", LADDER)
def test_svgp_gradient_yardsticks_reject_exchanged_parameters(d):
    pb = G.problem(SVGP_SHAPE[d])
    assert pb.X.shape[1] == d
    Z, X, y = pb.Z[0], pb.X, pb.Y[:, 0]
    for kind in KINDS:
        kp = G.with_kind(pb.kps[0], kind)
        g_r = G.formula_task(Z, X, y, kp)
        dz_r, scale = ZR.formula_dz(Z, X, y, kp)
        for what, i, j in swaps(kind, d):
            wrong = swapped(kp, i, j, what)
            rg = G.entry_ratio(G.formula_task(Z, X, y, wrong), g_r) / G.TAU
            rz = ZR.ratio(ZR.formula_dz(Z, X, y, wrong)[0], dz_r, scale) / ZR.TAUZ
            print(f"d = {d} {kind} {what} ({i}, {j}): disagreement / tolerance: hyperparameter gradient {rg:.1e}, "
                  f"dZ {rz:.1e}")
            assert rg >= MARGIN and rz >= MARGIN, (kind, what, i, j)


def test_svgp_problems_have_distinct_parameters():
    """The SVGP problems draw their own parameters (0.8 + U lengthscales, 0.05 + 0.1 U linear variances): distinct too."""
    for d, shape in SVGP_SHAPE.items():
        for p in G.problem(shape).kps:
            for v in (p.lengthscales(d), p.linear_variances(d)):
                assert len(set(v)) == d
    assert dataclasses.is_dataclass(G.problem(104).ops[0]) and len(G.problem(104).ops) == 1
