"""CPU tests of the arbitrary-precision acquisition reference (tests/mp_acq_ref.py) and the measurement of the fp64 CPU
forms against it on the ladders of tests/acq_tails_util.py: the oracle's analytic scores on the oracle's moments, the
torch MC references, the acqf classes on the oracle engine.  The measured deviations are printed and asserted against
the caps recorded in tests/acq_tails_util.py; tests/test_gpu_acq_tails.py holds the device to four times those."""
import math

import mpmath as mp
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import acq_tails_util as U
from tests import mc_acq_ref as R
from tests import mc_nei_ref as N
from tests import mp_acq_ref as M
from tests.oracle_engine import OracleEngine

KINDS = U.ORACLE_KINDS


# ---- the reference against the existing ones, mid-range ---------------------------------------------------------------
def test_mp_analytic_agrees_with_oracle_midrange():
    rng = np.random.default_rng(0)
    mu, var = rng.standard_normal(200), rng.uniform(0.01, 2.0, 200)
    best_f, beta = 0.3, 3.0
    ref = {k: O.acquisition(mu, var, v, best_f, beta) for k, v in KINDS.items()}
    for i in range(200):
        p = M.analytic(mu[i], var[i], best_f)
        assert abs(float(p["u"])) < 40
        assert float(p["ei"]) == pytest.approx(ref["ei"][i], rel=1e-12, abs=1e-300)
        assert float(p["logei"]) == pytest.approx(ref["logei"][i], rel=1e-12, abs=1e-12)
        assert float(M.ucb(mu[i], var[i], beta)) == pytest.approx(ref["ucb"][i], rel=1e-14)
        assert float(M.variance(mu[i], var[i])) == var[i]


@pytest.mark.parametrize("mode", list(U.MODES))
def test_mp_qlogei_agrees_with_torch_reference_midrange(mode):
    fat_relu, fat_max = U.MODES[mode]
    mean, cov = R.synthetic_moments(2, 3, seed=1)
    z = R.base_samples(8, 3, seed=2)
    best_f = float(mean.median())
    rv, rgm, rgc, info = R.mc_acq(mean, cov, z, "qlogei", best_f=best_f, fat_relu=fat_relu, fat_max=fat_max)
    v, gm, gc = M.mc_acq(mean.tolist(), cov.tolist(), z.tolist(), info.tolist(), best_f, fat_relu, fat_max)
    np.testing.assert_allclose(M.to_float(v), rv.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(M.to_float(gm), rgm.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(M.to_float(gc), rgc.numpy(), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("mode", list(U.NEI_MODES))
def test_mp_nei_agrees_with_torch_reference_midrange(mode):
    mu_b, cov_bb, mean, cov, cross = N.synthetic(2, 3, 2)
    zb, zq = N.base_samples(8, 2, 3)
    Linv, best = N.setup(mu_b, cov_bb, zb)
    args = (mean, cov, cross, Linv, zb, best, zq)
    ref = N.mc_nei(*args, **U.NEI_MODES[mode])
    kw = dict(fat_relu=True, fat_max=True)
    kw.update(U.NEI_MODES[mode])
    got = M.mc_nei(*(a.tolist() for a in args), ref[4].tolist(), **kw)
    for g, r in zip(got, ref[:4]):
        np.testing.assert_allclose(M.to_float(g), r.numpy(), rtol=1e-10, atol=1e-12)


def test_mp_rejects_shapes_beyond_its_limit():
    mean, cov = R.synthetic_moments(1, 4, seed=1)
    with pytest.raises(ValueError):
        M.mc_acq(mean.tolist(), cov.tolist(), R.base_samples(3, 4, seed=1).tolist(), [0], 0.0, True, True)


# ---- the reference's own accuracy: twice the digits ---------------------------------------------------------------
def test_mp_analytic_is_good_to_1e25_at_twice_the_digits():
    worst = mp.mpf(0)
    for u in (1e8, 30.0, 1e-3, 0.0, -0.5, -1.0, -3.0, -37.0, -38.5, -1e3, -1e5, -67108864.0, -1e10, -1e30, -1e100, -1e150):
        for var in (1e-12, 1e-4, 1.0, 1e12):
            mu = 0.25
            best_f = mu - u * math.sqrt(var)
            a = M.analytic(mu, var, best_f)
            b = M.analytic(mu, var, best_f, dps=2 * M.analytic_dps(mu, var, best_f))
            for k in ("ei", "logei"):
                worst = max(worst, abs(a[k] - b[k]) / abs(b[k]) if b[k] != 0 else abs(a[k]))
    print(f"mp analytic: largest relative change at twice the digits {mp.nstr(worst, 3)}")
    assert worst < 1e-25


def test_mp_mc_is_good_to_1e25_at_twice_the_digits():
    worst = mp.mpf(0)
    for label in ("median", "above 1000", "below 1000", "tau_max 1e-4 above 1", "mean 0 cov 1e-12 y across -37 q=2"):
        call = next(c for c in U.mc_calls(2, 3) if c["label"] == label)
        for mode in ("fatplus_fatmax", "softplus_lse"):
            fat_relu, fat_max = U.MODES[mode]
            a, b = (M.mc_acq(call["mean"].tolist(), call["cov"].tolist(), call["z"].tolist(), [0], call["best_f"],
                             fat_relu, fat_max, U.TAU_RELU, call["tau_max"], dps=d) for d in (M.BASE_DPS, 2 * M.BASE_DPS))
            flat = lambda t: [t[0][0]] + t[1][0] + [v for row in t[2][0] for v in row]  # noqa: E731
            scale = max(abs(v) for v in flat(b)[1:])
            worst = max(worst, abs(flat(a)[0] - flat(b)[0]) / (1 + abs(flat(b)[0])),
                        max(abs(x - y) for x, y in zip(flat(a)[1:], flat(b)[1:])) / scale)
    print(f"mp MC: largest change at twice the digits {mp.nstr(worst, 3)}")
    assert worst < 1e-25


# ---- the baseline: oracle.acquisition on oracle.posterior's moments --------------------------------------------------
def oracle_moments(noise, y_scale):
    p = O.KernelParams(O.RBF, np.array([U.LENGTHSCALE]), noise=noise)
    st = O.fit(np.array([[U.X0]]), np.array([U.Y0]), p)
    return O.posterior(st, U.candidates(), U.Y_MEAN, y_scale)


def test_baseline_analytic_oracle_against_mp():
    worst = {"ei": 0.0, "logei": 0.0, "ucb": 0.0, "logei_join": 0.0}
    us = []
    for noise in U.NOISES:
        for y_scale in U.Y_SCALES:
            mu, var = oracle_moments(noise, y_scale)
            if noise == 0.0:
                assert var[0] == max(1e-10 * y_scale ** 2, 1e-12)  # the training point: on the floor
            if y_scale == 1e-6:
                assert (var == 1e-12).all()
            w, u = U.analytic_baseline(mu, var, lambda kind, best_f, beta: O.acquisition(mu, var, KINDS[kind], best_f, beta))
            print(f"baseline oracle analytic noise={noise:g} y_scale={y_scale:g}: " +
                  " ".join(f"{k} {v:.2f} eps" for k, v in w.items()))
            worst = {k: max(worst[k], w[k]) for k in w}
            us.append(u)
    U.check_u_coverage(np.concatenate(us))
    print("baseline oracle analytic, all configurations: " + " ".join(f"{k} {v:.2f} eps" for k, v in worst.items()),
          "caps", U.CAP_ANALYTIC_EPS)
    for k in worst:
        assert worst[k] <= U.CAP_ANALYTIC_EPS[k], (k, worst[k])


def test_oracle_logei_is_minus_infinity_where_u_squared_overflows():
    s = O.acquisition(np.array([0.0]), np.array([1.0]), O.ACQ_LOGEI, -U.U_OVERFLOW)
    assert s[0] == -math.inf
    assert O.acquisition(np.array([0.0]), np.array([1.0]), O.ACQ_EI, -U.U_OVERFLOW)[0] == 0.0


# ---- the baseline: the torch MC references -----------------------------------------------------------------------------
def _label_max(store, label, kind, d):
    store[(label, kind)] = max(store.get((label, kind), 0.0), d)


def _report(name, worst, caps):
    for (label, kind), d in sorted(worst.items()):
        print(f"baseline {name} [{label}] {kind}: {d:.2f} eps (cap {caps.get(label, {}).get(kind)})")
    for (label, kind), d in worst.items():
        assert d <= caps[label][kind], (label, kind, d)


@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("S", [3, 8])
def test_baseline_mc_acq_ref_against_mp(q, S):
    worst = {}
    for call in U.mc_calls(q, S):
        if call["label"].startswith("mean 0 cov 1e-12 y across -37"):
            y = U.call_y(call)
            assert float(y.min()) < -37.0 < float(y.max())
        if call["label"].startswith("mean 0 cov 1e-14 y in (-31, -30)"):
            y = U.call_y(call)
            assert -31.0 < float(y.min()) and float(y.max()) < -30.0
        for mode, (fat_relu, fat_max) in U.MODES.items():
            rv, rgm, rgc, info = R.mc_acq(call["mean"], call["cov"], call["z"], "qlogei", best_f=call["best_f"],
                                          fat_relu=fat_relu, fat_max=fat_max, tau_relu=U.TAU_RELU,
                                          tau_max=call["tau_max"])
            assert info.tolist() == [1 if call["label"].startswith("jitter") else 0]
            assert not (rv.isnan().any() or rgm.isnan().any() or rgc.isnan().any())
            v, gm, gc = U.mc_ref(call, mode, info.tolist())
            _label_max(worst, call["label"], "value", U.value_dev_eps(rv[0], v[0]))
            _label_max(worst, call["label"], "gmean", U.grad_dev_eps(rgm[0], gm[0]))
            _label_max(worst, call["label"], "gcov", U.grad_dev_eps(rgc[0], gc[0]))
    _report(f"mc_acq_ref q={q} S={S}", worst, U.CAP_MC_EPS)


@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("S", [3, 8])
def test_baseline_mc_nei_ref_against_mp(q, nb, S):
    worst = {}
    for call in U.nei_calls(q, nb, S):
        for mode, kw in U.NEI_MODES.items():
            ref = N.mc_nei(*call["args"], tau_relu=U.TAU_RELU, tau_max=call["tau_max"], **kw)
            assert ref[4].tolist() == [1 if call["label"].startswith("jitter") else 0]
            assert not any(bool(t.isnan().any()) for t in ref[:4])
            v, gm, gc, gx = U.nei_ref(call, mode, ref[4].tolist())
            _label_max(worst, call["label"], f"{mode} value", U.value_dev_eps(ref[0][0], v[0]))
            for name, g, r in (("gmean", ref[1], gm), ("gcov", ref[2], gc), ("gcross", ref[3], gx)):
                _label_max(worst, call["label"], f"{mode} {name}", U.grad_dev_eps(g[0], r[0]))
    _report(f"mc_nei_ref q={q} nb={nb} S={S}", worst, U.CAP_NEI_EPS)


# ---- the baseline: the acqf classes on the oracle engine against the closed-form one-point model --------------------
def test_baseline_acqf_on_oracle_engine_against_mp():
    worst_v, worst_g = U.torch_side_devs(OracleEngine(), torch.device("cpu"))
    print(f"baseline acqf analytic on the oracle engine: values {worst_v} eps, gradients {worst_g} eps; caps "
          f"{U.CAP_TORCH_EPS}")
    for kind in worst_v:
        assert worst_v[kind] <= U.CAP_TORCH_EPS["value"][kind], (kind, worst_v[kind])
        assert worst_g[kind] <= U.CAP_TORCH_EPS["grad"][kind], (kind, worst_g[kind])
