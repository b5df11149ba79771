"""The device's acquisition arithmetic against the arbitrary-precision reference (tests/mp_acq_ref.py) in the tails of
its argument range: the analytic scores of the sweep (finalize_kernel, gpx_sweep.hip) on the device's own moments, the
pruned sweep far from the incumbent, the MC kernels (gpx_mcacq.hip) and acqf's analytic classes on device tensors.

Ladders, metrics and the measured fp64 CPU baselines are those of tests/acq_tails_util.py (tests/test_acq_ref_host.py
measures the baselines on the same ladders).  Bounds: four times the CPU baseline, never below 16 eps; LogEI just below
the join at -1 is also held to twice its baseline in absolute terms (JOIN_FACTOR).  The MC tests print the torch
reference's deviation from mp on the same call beside the device's.  The largest
deviations seen on the device are printed per group and recorded in DESIGN.md §4."""
import math

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import KernelParams
from oracle import gp_oracle as O
from tests import acq_tails_util as U
from tests import mc_acq_ref as R
from tests import mc_nei_ref as N
from tests import test_gpu_sweep_prune as P
from tests import test_gpu_topk_sweep as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ENTRIES = ["fused", "unfused", "multi"]
_states = {}


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


# ---- analytic scores --------------------------------------------------------------------------------------------------
def one_point_state(engine, noise):
    if ("single", noise) not in _states:
        kp = KernelParams("rbf", U.LENGTHSCALE, noise=noise)
        _states[("single", noise)] = engine.fit(t([[U.X0]]), t([U.Y0]), kp)
    return _states[("single", noise)]


MULTI = dict(weights=(0.7, -1.3), y_mean=(U.Y_MEAN, -0.1), targets=(U.Y0, -0.4), lengthscales=(U.LENGTHSCALE, 1.3))


def two_output_states(engine, noise):
    if ("multi", noise) not in _states:
        kps = [KernelParams("rbf", ls, noise=noise) for ls in MULTI["lengthscales"]]
        _states[("multi", noise)] = engine.fit_outputs(t([[U.X0]]), t([list(MULTI["targets"])]), kps)
    return _states[("multi", noise)]


def scorer(engine, entry, noise, y_scale, alpha=None):
    """score(kind, best_f, beta) -> (scores as numpy, best value tensor, best index tensor) of one entry point"""
    Xs = t(U.candidates())
    if entry == "multi":
        states = two_output_states(engine, noise)
        kw = dict(weights=MULTI["weights"], y_mean=MULTI["y_mean"], y_scale=(y_scale, 0.5 * y_scale))

        def call(kind, best_f, beta):
            return engine.acquire_multi(states, Xs, kind, best_f=best_f, beta=beta, return_scores=True, **kw)
    else:
        st = one_point_state(engine, noise)

        def call(kind, best_f, beta):
            return engine.acquire(st, Xs, kind, best_f=best_f, beta=beta, y_mean=U.Y_MEAN, y_scale=y_scale,
                                  alpha=alpha, return_scores=True)

    def score(kind, best_f, beta):
        before = engine.get_option("sweep_fused")
        engine.set_option("sweep_fused", 0 if entry == "unfused" else before)
        try:
            bv, bi, sc = call(kind, best_f, beta)
            torch.cuda.synchronize()
        finally:
            engine.set_option("sweep_fused", before)
        return sc.cpu().numpy(), bv, bi
    return score


def device_moments(score):
    """the kernel's own (mu, var): UCB with beta = 0 and the variance scores"""
    return score("ucb", 0.0, 0.0)[0], score("variance", 0.0, 0.0)[0]


def oracle_dev_eps(kind, got, mu, var, best_f, beta):
    """deviation in eps of every candidate's score from the fp64 oracle on the same moments (metrics of
    tests/acq_tails_util.py with the oracle as the reference); EI only where its terms are normal numbers"""
    ref = O.acquisition(mu, var, U.ORACLE_KINDS[kind], best_f, beta)
    if kind != "ei":
        with np.errstate(invalid="ignore"):
            d = np.abs(got - ref) / (1.0 + np.abs(ref))
        return np.where(got == ref, 0.0, d) / U.EPS
    sigma = np.sqrt(var)
    u = (mu - best_f) / sigma
    with np.errstate(over="ignore", under="ignore"):
        phi = np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    scale = np.maximum(sigma * phi * (1.0 + np.abs(u)), np.abs(ref))
    ok = (u > -37.0) & (scale > 0)
    return np.where(ok, np.abs(got - ref) / np.where(ok, scale, 1.0), 0.0) / U.EPS


@pytest.mark.parametrize("y_scale", U.Y_SCALES)
@pytest.mark.parametrize("noise", U.NOISES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_analytic_scores_against_mp(engine, entry, noise, y_scale):
    score = scorer(engine, entry, noise, y_scale)
    mu, var = device_moments(score)
    assert np.isfinite(mu).all() and (var >= 1e-12).all()
    if y_scale == 1e-6:
        assert (var == 1e-12).all()  # the scored variance on BoTorch's floor
    worst_oracle = {}

    def checked(kind, best_f, beta):
        s, bv, bi = score(kind, best_f, beta)
        assert not np.isnan(s).any(), (kind, best_f, int(np.flatnonzero(np.isnan(s))[0]))
        i_ref = int(np.flatnonzero(s == s.max())[0])  # the lowest-index argmax of the returned scores
        assert int(bi.item()) == i_ref and bv.view(torch.int64).item() == s[i_ref:i_ref + 1].view(np.int64)[0]
        d = float(oracle_dev_eps(kind, s, mu, var, best_f, beta).max())
        worst_oracle[kind] = max(worst_oracle.get(kind, 0.0), d)
        return s

    worst, _ = U.analytic_baseline(mu, var, checked)
    print(f"device analytic {entry} noise={noise:g} y_scale={y_scale:g}: vs mp " +
          " ".join(f"{k} {v:.2f} eps" for k, v in worst.items()) + "; all candidates vs oracle " +
          " ".join(f"{k} {v:.2f} eps" for k, v in worst_oracle.items()))
    join = worst.pop("logei_join")
    assert join <= U.JOIN_FACTOR * U.CAP_ANALYTIC_EPS["logei_join"], ("logei on [-3, -1), absolute", join)
    for kind, d in worst.items():
        bound = U.device_bound_eps(U.CAP_ANALYTIC_EPS[kind])
        assert d <= bound, (kind, d, bound)
        # both within their bound of mp: the device and the oracle are within the sum of each other
        assert worst_oracle[kind] <= bound + U.CAP_ANALYTIC_EPS[kind], (kind, worst_oracle[kind])


@pytest.mark.parametrize("entry", ENTRIES)
def test_ladder_covers_every_branch_on_the_device_moments(engine, entry):
    """the u of the points compared with mp, from the moments each entry point returns, pooled over its configurations"""
    us = [U.ladder_u(*device_moments(scorer(engine, entry, noise, y_scale))) for noise in U.NOISES
          for y_scale in U.Y_SCALES]
    U.check_u_coverage(np.concatenate(us))


@pytest.mark.parametrize("y_scale", U.Y_SCALES)
@pytest.mark.parametrize("noise", U.NOISES)
def test_sweep_moments_equal_posterior_bits(engine, noise, y_scale):
    st = one_point_state(engine, noise)
    pm, pv = engine.posterior(st, t(U.candidates()), y_mean=[U.Y_MEAN], y_scale=[y_scale])
    for entry in ("fused", "unfused"):
        mu, var = device_moments(scorer(engine, entry, noise, y_scale))
        assert np.array_equal(mu.view(np.int64), pm[:, 0].cpu().numpy().view(np.int64)), entry
        assert np.array_equal(var.view(np.int64), pv.cpu().numpy().view(np.int64)), entry
    if noise == 0.0:
        assert float(pv[0]) == max(1e-10 * y_scale ** 2, 1e-12)  # the training point: on GPyTorch's floor


@pytest.mark.parametrize("entry", ENTRIES)
def test_logei_is_minus_infinity_where_u_squared_overflows(engine, entry):
    score = scorer(engine, entry, 1e-4, 1.0)
    mu, var = device_moments(score)
    j = U.anchors(var)[0]
    best_f = float(mu[j] - U.U_OVERFLOW * math.sqrt(var[j]))
    assert score("logei", best_f, 4.0)[0][j] == -math.inf
    e = score("ei", best_f, 4.0)[0]
    assert (e == 0.0).all()


MONO_U = (1.0, 0.0, -1.0, -10.0, -38.0, -1e3, -1024.0, -1e5, -67108864.0, -1e10)
MONO_ALPHA = (1.0, 1.0 + 2.0 ** -50, 1.0 + 1e-12, 1.0 + 1e-9, 1.0 + 1e-6, 1.001, 1.5)


def assert_monotone(lo, hi, what):
    """score(larger moment) >= score(smaller) - 1e-9 (|score| + 1) / 4: a violation stays four times inside the margin
    PRUNE_EPS gives the bound test (gpx_sweep.hip)"""
    with np.errstate(invalid="ignore"):
        ok = hi >= lo - 1e-9 * (np.abs(hi) + 1.0) / 4.0
    ok |= (hi == lo)  # -inf against -inf
    assert ok.all(), (what, int(np.flatnonzero(~ok)[0]), lo[~ok][:3], hi[~ok][:3])


@pytest.mark.parametrize("noise", U.NOISES)
@pytest.mark.parametrize("entry", ["fused", "unfused"])
def test_scores_are_monotone_in_each_moment(engine, entry, noise):
    st = one_point_state(engine, noise)
    a0 = float(st.alpha[0, 0])

    def alpha(c):
        a = torch.zeros(st.npad, dtype=torch.float64, device=DEV)
        a[0] = a0 * c
        return a

    # var only: alpha = 0 holds the mean at y_mean for every candidate, the variance grows with the distance
    score = scorer(engine, entry, noise, 1.0, alpha=alpha(0.0))
    mu, var = device_moments(score)
    assert (mu == U.Y_MEAN).all()
    up, down = np.flatnonzero(var[1:] > var[:-1]), np.flatnonzero(var[1:] < var[:-1])
    same = np.flatnonzero(var[1:] == var[:-1])
    assert len(up) > 1500
    j = U.anchors(var)[0]
    for kind in ("ei", "logei", "ucb", "variance"):
        for u_t in (MONO_U if kind in ("ei", "logei") else (0.0,)):
            s = score(kind, float(mu[j] - u_t * math.sqrt(var[j])), 3.0)[0]
            assert_monotone(s[up], s[up + 1], (kind, u_t, "var up"))
            assert_monotone(s[down + 1], s[down], (kind, u_t, "var down"))
            assert np.array_equal(s[same].view(np.int64), s[same + 1].view(np.int64))
    # mu only: the same candidates under a growing alpha keep their variance, their mean moves by k* alpha
    base = scorer(engine, entry, noise, 1.0, alpha=alpha(1.0))
    mu1, var1 = device_moments(base)
    j = U.anchors(var1)[0]
    best_fs = [float(mu1[j] - u_t * math.sqrt(var1[j])) for u_t in MONO_U]
    prev = None
    for c in MONO_ALPHA:
        score = scorer(engine, entry, noise, 1.0, alpha=alpha(c))
        mu_c, var_c = device_moments(score)
        assert np.array_equal(var_c.view(np.int64), var1.view(np.int64))
        cur = {(kind, b): score(kind, b, 3.0)[0] for kind in ("ei", "logei") for b in best_fs}
        cur[("ucb", 0.0)] = score("ucb", 0.0, 3.0)[0]
        if prev is not None:
            mu_p, sc_p = prev
            up, down = mu_c > mu_p, mu_c < mu_p
            assert up.sum() + down.sum() > 1000 or c < 1.0 + 1e-11
            for key, s in cur.items():
                assert_monotone(sc_p[key][up], s[up], (key, c, "mu up"))
                assert_monotone(s[down], sc_p[key][down], (key, c, "mu down"))
        prev = (mu_c, cur)


# ---- the pruned sweep in the tails -----------------------------------------------------------------------------------
PRUNE_N, PRUNE_M, TOPK = 384, 2048, 16


def prune_cases(y):
    cases = [(acq, best_f, y_scale) for acq in ("ei", "logei")
             for best_f in (float(y.max()) + 1e3, 1e8, 1e100, -1e3) for y_scale in (1e-6, 1e6)]
    return cases + [(acq, 0.0, y_scale) for acq in ("ucb", "variance") for y_scale in (1e-6, 1e6)]


def test_pruning_engages_at_the_shape_of_the_tail_cases(engine):
    st, _, y = P.fitted(engine, PRUNE_N, "rbf")
    full, pruned = P.both(engine, st, t(P.candidates(PRUNE_M)), "logei", best_f=float(y.max()))
    print(f"n = {PRUNE_N}, m = {PRUNE_M}: sweep_stats pruned {pruned[2]} full {full[2]}")
    assert pruned[2][2] < pruned[2][3]  # product tiles were dropped


def test_pruned_sweep_returns_the_full_sweeps_bits_in_the_tails(engine):
    st, _, y = P.fitted(engine, PRUNE_N, "rbf")
    Xs = t(P.candidates(PRUNE_M))
    for acq, best_f, y_scale in prune_cases(y):
        kw = dict(best_f=best_f, beta=4.0, y_mean=0.3, y_scale=y_scale)
        full, pruned = P.both(engine, st, Xs, acq, **kw)  # asserts equal (value bits, index)
        sc, key = K.composition(engine, st, Xs, acq, **kw)
        assert not np.isnan(sc.cpu().numpy()).any(), (acq, best_f, y_scale)
        i_ref = int(np.flatnonzero(key == key.max())[0])
        assert full[1] == i_ref, (acq, best_f, y_scale)
        for prune in (0, 2):
            K.check(engine, K.topk(engine, prune, st, Xs, TOPK, acq, **kw), sc, key, TOPK)


@pytest.mark.parametrize("y_scale", [1e-6, 1e6])
def test_ei_that_underflows_everywhere_answers_index_zero(engine, y_scale):
    st, _, y = P.fitted(engine, PRUNE_N, "rbf")
    Xs = t(P.candidates(PRUNE_M))
    kw = dict(best_f=1e100, y_mean=0.3, y_scale=y_scale)
    full, pruned = P.both(engine, st, Xs, "ei", **kw)
    assert full[1] == 0 and full[0] in (0, -2 ** 63)  # zero, all ties: the lowest index
    sc, key = K.composition(engine, st, Xs, "ei", **kw)
    assert (key == 0.0).all()
    got = K.topk(engine, 2, st, Xs, TOPK, "ei", **kw)
    assert np.array_equal(got[1], np.arange(TOPK))


# ---- MC kernels ---------------------------------------------------------------------------------------------------------
def _expected_info(call):
    return [1 if call["label"].startswith("jitter") else 0]


@pytest.mark.parametrize("mode", list(U.MODES))
@pytest.mark.parametrize("S", [3, 8])
@pytest.mark.parametrize("q", [1, 2, 3])
def test_mc_acq_against_mp(engine, q, S, mode):
    fat_relu, fat_max = U.MODES[mode]
    worst, failed = {}, []
    for call in U.mc_calls(q, S):
        value, gmean, gcov, info = (o.cpu() for o in engine.mc_acq(
            call["mean"].to(DEV), call["cov"].to(DEV), call["z"].to(DEV), "qlogei", best_f=call["best_f"],
            fat_relu=fat_relu, fat_max=fat_max, tau_max=call["tau_max"], tau_relu=U.TAU_RELU))
        assert info.tolist() == _expected_info(call), call["label"]
        assert not (value.isnan().any() or gmean.isnan().any() or gcov.isnan().any()), call["label"]
        v, gm, gc = U.mc_ref(call, mode, info.tolist())
        devs = (("value", U.value_dev_eps(value[0], v[0])), ("gmean", U.grad_dev_eps(gmean[0].numpy(), gm[0])),
                ("gcov", U.grad_dev_eps(gcov[0].numpy(), gc[0])))
        # the torch reference against mp on this very call, printed beside the device's figure
        rv, rgm, rgc, _ = R.mc_acq(call["mean"], call["cov"], call["z"], "qlogei", best_f=call["best_f"],
                                   fat_relu=fat_relu, fat_max=fat_max, tau_relu=U.TAU_RELU, tau_max=call["tau_max"])
        base = {"value": U.value_dev_eps(rv[0], v[0]), "gmean": U.grad_dev_eps(rgm[0].numpy(), gm[0]),
                "gcov": U.grad_dev_eps(rgc[0].numpy(), gc[0])}
        cap = U.CAP_MC_EPS[call["label"]]
        for kind, d in devs:
            worst[kind] = max(worst.get(kind, (0.0, "", 0.0)), (d, call["label"], base[kind]))
            if d > U.device_bound_eps(cap[kind]):
                failed.append((call["label"], kind, d, U.device_bound_eps(cap[kind])))
    print(f"device mc_acq {mode} q={q} S={S}: " +
          " ".join(f"{k} {d:.2f} eps [{lab}, torch {b:.2f}]" for k, (d, lab, b) in worst.items()))
    assert not failed, failed


@pytest.mark.parametrize("S", [3, 8])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("q", [1, 2, 3])
def test_mc_nei_against_mp(engine, q, nb, S):
    worst, failed = {}, []
    for call in U.nei_calls(q, nb, S):
        for mode, kw in U.NEI_MODES.items():
            out = engine.mc_nei(*(a.to(DEV) for a in call["args"]), tau_max=call["tau_max"], tau_relu=U.TAU_RELU, **kw)
            value, gmean, gcov, gcross, info = (o.cpu() for o in out)
            assert info.tolist() == _expected_info(call), call["label"]
            assert not any(bool(x.isnan().any()) for x in (value, gmean, gcov, gcross)), call["label"]
            v, gm, gc, gx = U.nei_ref(call, mode, info.tolist())
            devs = ((f"{mode} value", U.value_dev_eps(value[0], v[0])),
                    (f"{mode} gmean", U.grad_dev_eps(gmean[0].numpy(), gm[0])),
                    (f"{mode} gcov", U.grad_dev_eps(gcov[0].numpy(), gc[0])),
                    (f"{mode} gcross", U.grad_dev_eps(gcross[0].numpy(), gx[0])))
            ref = N.mc_nei(*call["args"], tau_relu=U.TAU_RELU, tau_max=call["tau_max"], **kw)  # printed beside
            base = (U.value_dev_eps(ref[0][0], v[0]), U.grad_dev_eps(ref[1][0].numpy(), gm[0]),
                    U.grad_dev_eps(ref[2][0].numpy(), gc[0]), U.grad_dev_eps(ref[3][0].numpy(), gx[0]))
            cap = U.CAP_NEI_EPS[call["label"]]
            for (kind, d), b in zip(devs, base):
                worst[kind] = max(worst.get(kind, (0.0, "", 0.0)), (d, call["label"], b))
                if d > U.device_bound_eps(cap[kind]):
                    failed.append((call["label"], kind, d, U.device_bound_eps(cap[kind])))
    print(f"device mc_nei q={q} nb={nb} S={S}: " +
          " ".join(f"{k} {d:.2f} eps [{lab}, torch {b:.2f}]" for k, (d, lab, b) in worst.items()))
    assert not failed, failed


# ---- torch side ---------------------------------------------------------------------------------------------------------
def test_acqf_analytic_classes_on_device_tensors_against_mp(engine):
    worst_v, worst_g = U.torch_side_devs(engine, DEV)
    print(f"device acqf analytic: values {worst_v} eps, gradients {worst_g} eps")
    for kind in worst_v:
        assert worst_v[kind] <= U.device_bound_eps(U.CAP_TORCH_EPS["value"][kind]), (kind, worst_v[kind])
        assert worst_g[kind] <= U.device_bound_eps(U.CAP_TORCH_EPS["grad"][kind]), (kind, worst_g[kind])
