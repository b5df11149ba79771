"""The acquisition sweep family with ARD parameters: a different lengthscale and a different linear variance in every
dimension (tests/ard_util.py), along the dimension ladder 4, 5, 8, 9, 16, 17, 32 (each DMAX instance of the d-dispatched
kernels at its widest d, the next at its narrowest).

The other sweep modules build their models from one scalar lengthscale and one scalar linear variance, under which a
kernel that reads parameter k where it should read parameter col, on both operands alike, computes the right numbers.
Here every path of the family runs with parameters that tell the dimensions apart, by the yardsticks of the modules
whose helpers are imported (not copied) below:

  full sweep        posterior and argmax against the CPU oracle (test_gpu_parity.check_posterior / check_argmax, the
                    oracle's own margin guarded first)
  pruned sweep      (value bits, index) of sweep_prune = 2 and of the default against sweep_prune = 0, with the
                    sweep_stats identities of test_gpu_sweep_lazy.py; d <= 16 runs the lazy MFMA K* build, d = 17 and 32
                    launch_sweep_chunk_pruned (read from the stage descriptors, as test_gpu_sweep_tail.py does)
  top-k             test_gpu_topk_sweep.check; the multi-output form by test_gpu_topk_multi.check
  fused small-n     against the oracle and against the unfused path (test_gpu_small_n.py)
  head mean bound   |mu - mu_approx| <= mu_slack on all three paths, the slack's size, the gathered partials' bits
  append            test_append.py's check, one case

Shapes are the suite's smallest at which each path exists: n = 300 (padded 384: three row tiles, the minimum for
pruning), m = 5000 (the 1024-candidate seed block, then 3976 staged candidates with a partial last tile), noise 1e-4.
tests/test_ard_host.py checks on the CPU that the oracle fits these problems, that every best score is clear of its
runner-up, and that these yardsticks reject two exchanged parameters.
"""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import multi_sweep_util as U
from tests import test_append as AP
from tests import test_gpu_small_n as SN
from tests import test_gpu_sweep_lazy as LZ
from tests import test_gpu_sweep_mubound as MB
from tests import test_gpu_sweep_mufact32 as MF
from tests import test_gpu_sweep_tail as TL
from tests import test_gpu_topk_multi as TM
from tests import test_gpu_topk_sweep as TK
from tests.ard_util import ACQS, BETA, KINDS, LADDER, NOISE, ard_params, sweep_problem
from tests.oracle_engine import to_oracle_params
from tests.test_gpu_outputs import margin_guard
from tests.test_gpu_parity import check_argmax, check_posterior, t

pytestmark = pytest.mark.gpu
N, M, SEED_BLOCK = 300, 5000, 1024
NPAD = 384
_fits = {}


def fitted(engine, d, kind):
    """One fit per (d, kind) for the whole module, on the device and in the oracle, with the oracle's posterior at
    the candidates; never modified."""
    if (d, kind) not in _fits:
        X, y, Xs = sweep_problem(N, d, M)
        kp, op = ard_params(kind, d, d, noise=NOISE)
        assert len(set(kp.lengthscale)) == d and len(set(kp.linear_variance)) == d
        ost = O.fit(X, y, op)
        mu_r, var_r = O.posterior(ost, Xs)
        _fits[(d, kind)] = dict(st=engine.fit(t(X), t(y), kp), Xs=t(Xs), mu_r=mu_r, var_r=var_r,
                                kdiag=O.kernel_diag(Xs, op), kw=dict(best_f=float(y.max()), beta=BETA))
    return _fits[(d, kind)]


def tiles(stats):
    """The sweep_stats of a call in words: a path that silently fell back to the full sweep shows as 1.000."""
    return (f"{stats[2]} of {stats[3]} tiles executed ({stats[2] / stats[3]:.3f}), {stats[1]} of {stats[0]} columns "
            f"computed to the last row tile")


# ---- the full sweep against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("d", LADDER)
@pytest.mark.parametrize("kind", KINDS)
def test_full_sweep_matches_oracle(engine, kind, d):
    f = fitted(engine, d, kind)
    mu, var = engine.posterior(f["st"], f["Xs"])
    check_posterior(mu.cpu().numpy(), var.cpu().numpy(), f["mu_r"], f["var_r"], f["kdiag"])
    for acq, kid in ACQS.items():
        sref = O.acquisition(f["mu_r"], f["var_r"], kid, f["kw"]["best_f"], BETA)
        margin_guard(sref, 1e-9 * max(1.0, abs(float(np.nanmax(sref)))), f"d = {d} {kind} {acq}")  # check_argmax's bound
        _, bi, sc = engine.acquire(f["st"], f["Xs"], acq, return_scores=True, **f["kw"])
        check_argmax(int(bi.item()), sref, sc.cpu().numpy(), f"d = {d} {kind} {acq}")


# ---- pruned against full -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", LADDER)
@pytest.mark.parametrize("acq", list(ACQS))
@pytest.mark.parametrize("kind", KINDS)
def test_pruned_sweep_has_the_bits_of_the_full_sweep(engine, kind, acq, d):
    f = fitted(engine, d, kind)
    st, Xs, kw = f["st"], f["Xs"], f["kw"]
    full, pruned = LZ.both(engine, st, Xs, acq, **kw)  # sweep_prune = 0, then 2, with the stats identities
    desc, count = TL.stage_descriptors(engine, NPAD, M)
    staged = M - SEED_BLOCK
    assert desc[0] == [0, SEED_BLOCK, staged, (staged + 127) // 128, -1]  # the staged columns behind the seed block
    if d <= 16:  # the lazy form: slot 1 is the gather's set, rebuilt into the round's buffer from survivor list 2
        assert desc[1][0] == 0 and desc[1][4] == 2, desc[:2]
    else:        # no MFMA K* build above d = 16: launch_sweep_chunk_pruned compacts the chunk's K* into buffer 1
        assert desc[1] == [1, 0, count[0], (count[0] + 127) // 128, 0], (desc[:2], count[:2])
    default = LZ.acquire(engine, 1, st, Xs, acq, **kw)
    for name, got in (("sweep_prune = 2", pruned), ("default", default)):
        print(f"d = {d} {kind} {acq} {name}: {tiles(got[2])}")
        assert got[:2] == full[:2], (name, got, full)
        assert got[2][0] == M and got[2][3] == full[2][3]
        assert got[2][2] < got[2][3], f"{name}: the staged path did not run"
        assert got[2][1] <= M / 4  # (the cap of test_gpu_sweep_lazy.test_pruning_engaged_on_the_lazy_path)
    if kind == "rbf" and d <= 16:  # the head mean bound against exact head means (sweep_prune = -2)
        MB.three(engine, st, Xs, acq, **kw)


# ---- top-k -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", LADDER)
@pytest.mark.parametrize("acq", list(ACQS))
@pytest.mark.parametrize("kind", KINDS)
def test_topk_has_the_bits_of_the_composition(engine, kind, acq, d):
    f = fitted(engine, d, kind)
    st, Xs, kw = f["st"], f["Xs"], f["kw"]
    sc, key = TK.composition(engine, st, Xs, acq, **kw)
    for k in (1, 16, 300):
        for prune in (2, 0):
            got = TK.topk(engine, prune, st, Xs, k, acq, **kw)
            TK.check(engine, got, sc, key, k)
            assert got[2][0] == M and got[2][3] > 0
            if prune == 0:
                assert got[2][1] == M and got[2][2] == got[2][3]
            else:
                print(f"d = {d} {kind} {acq} k = {k}: {tiles(got[2])}")
                assert k > 16 or got[2][2] < got[2][3]  # (k = 300: the 300th best of the seed block prunes little)


# ---- the multi-output pruned sweep -------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 8, 16, 17])
@pytest.mark.parametrize("acq", U.ACQS)
def test_multi_output_sweeps(engine, acq, d):
    """T = 3 outputs with three kernel kinds and three different ARD parameter sets.  The composition (the full
    multi-output sweep's scores) against the oracle, then acquire_topk_multi and acquire_multi against the composition
    bit for bit.  d = 17: one output without the lazy build sends the whole call to the full sweep."""
    states, pr = TM.fitted(engine, N, 3, d=d, ard=True)
    for p in pr["params"]:
        assert len(set(p.lengthscale)) == d and len(set(p.linear_variance)) == d
    assert len({tuple(p.lengthscale) for p in pr["params"]}) == 3
    Xn = U.candidates(M, d)
    Xs = t(Xn)
    kw = TM.objective(pr)
    sc, key = TM.composition(engine, states, Xs, acq, **kw)
    osts = O.fit_outputs(pr["X"], pr["Y"], [to_oracle_params(p, d) for p in pr["params"]])
    mu_o, var_o = O.objective_posterior(osts, Xn, pr["w"], pr["ym"], pr["ys"])
    sref = O.acquisition(mu_o, var_o, U.OACQ[acq], pr["best_f"], U.BETA)
    sg = sc.cpu().numpy()
    err = np.abs(sg - sref).max()
    assert err <= 1e-9 * max(1.0, np.abs(sref).max()), err
    margin_guard(sref, err, f"multi d = {d} {acq}")
    check_argmax(int(np.argmax(key)), sref, sg, f"multi d = {d} {acq}")
    full_tiles = 3 * ((M + 127) // 128) * (NPAD // 128)
    for k in (1, 16, 300):
        for prune in (2, 0):
            got = TM.topk(engine, prune, states, Xs, k, acq, **kw)
            TM.check(engine, got, sc, key, k)
            assert got[2][0] == M and got[2][3] == full_tiles
            if prune == 0 or d > 16:
                assert got[2][1] == M and got[2][2] == got[2][3]
            else:
                print(f"multi d = {d} {acq} k = {k}: {tiles(got[2])}")
                assert k > 16 or got[2][2] < got[2][3]
    bv, bi = engine.acquire_multi(states, Xs, acq, **kw)  # (the default sweep_prune: pruned for d <= 16)
    print(f"multi d = {d} {acq} argmax: {tiles(engine.sweep_stats())}")
    order = int(np.argsort(-key, kind="stable")[0])
    ref = torch.where(torch.isnan(bv), torch.full_like(bv, -np.inf), bv) + 0.0
    assert int(bi.item()) == order and int(TM.bits(ref)[0]) == int(key[order:order + 1].view(np.int64)[0])


# ---- the fused small-n sweep -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("d", [4, 5, 8, 9, 16])
@pytest.mark.parametrize("n", [100, 200])
def test_fused_small_n_matches_oracle_and_unfused(engine, n, d, nrhs):
    """Padded n = 128 and 256, the kinds and acquisitions cycled.  One output: posterior and argmax, fused against the
    oracle and against the unfused path.  Three outputs: the posterior of every output, both ways."""
    m = 1500
    X, y, Xn = sweep_problem(n, d, m)
    case = LADDER.index(d) + (n == 200) + nrhs
    kind, acq = KINDS[case % 3], list(ACQS)[case % 4]
    kp, op = ard_params(kind, d, d, noise=NOISE)
    Y = np.stack([y * (r + 1) - 0.3 * r for r in range(nrhs)], axis=1)
    ost = O.fit(X, Y if nrhs > 1 else y, op)
    st = engine.fit(t(X), t(Y if nrhs > 1 else y), kp)
    mu_r, var_r = O.posterior(ost, Xn)
    kdiag = O.kernel_diag(Xn, op)
    if nrhs > 1:
        out = {}
        for fused in (True, False):
            engine.set_option("sweep_fused", 1 if fused else 0)
            try:
                mu, var = engine.posterior(st, t(Xn))
            finally:
                engine.set_option("sweep_fused", 1)
            out[fused] = (mu.cpu().numpy(), var.cpu().numpy())
        check_posterior(out[True][0], out[True][1], mu_r.reshape(m, nrhs), var_r, kdiag)
        check_posterior(out[True][0], out[True][1], out[False][0], out[False][1], kdiag)
        return
    best_f = float(y.max())
    mu_f, var_f, bi_f, sg_f = SN._run(engine, st, Xn, acq, best_f, True)
    mu_u, var_u, bi_u, sg_u = SN._run(engine, st, Xn, acq, best_f, False)
    check_posterior(mu_f, var_f, mu_r.reshape(m, 1), var_r, kdiag)
    check_posterior(mu_f, var_f, mu_u, var_u, kdiag)
    _, _, sref = O.acquire_argmax(ost, Xn, ACQS[acq], best_f=best_f)
    margin_guard(sref, 1e-9 * max(1.0, abs(float(np.nanmax(sref)))), f"fused n = {n} d = {d} {kind} {acq}")
    check_argmax(bi_f, sref, sg_f, f"fused n = {n} d = {d} {kind} {acq}")
    check_argmax(bi_f, sg_u, sg_f, f"fused vs unfused n = {n} d = {d} {kind} {acq}")


# ---- the head mean bound (RBF) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 4, 5, 8, 9, 16])
def test_head_mean_bound_holds_on_all_three_paths(engine, d):
    """test_gpu_sweep_mufact32.test_bound_holds_on_all_three_paths with a lengthscale per dimension: the bound, both
    path counters, and the slack's size (the bound is not vacuous) on the unit-cube workgroup.  The small lengthscales
    stretch the unit cube, so at d = 5 and 8 its workgroups take the fp64 form and the ring at 0.995 of the limit runs the
    fp32 MFMA form; tests/mu_bound_util.py asserts that layout from its formulas."""
    MF.check_bound_on_all_three_paths(engine, N, d, ard=True)
    unit_cube = np.zeros(MF.M, dtype=bool)
    unit_cube[:256] = True
    MF.check_slack_size_on_the_factorised_forms(engine, N, d, ard=True, only=unit_cube)


@pytest.mark.parametrize("d", [5, 8])
def test_head_mean_bound_slack_size(engine, d):
    MF.check_slack_size_on_the_factorised_forms(engine, N, d, ard=True)


@pytest.mark.parametrize("d", [4, 8, 16])
def test_gather_partials_have_the_bits_of_the_full_build(engine, d):
    kp, _ = ard_params("rbf", d, d, outputscale=1.3)
    MB.check_gather_partials(engine, d, kp, np.random.default_rng(7 + d))


# ---- append ------------------------------------------------------------------------------------------------------------
def test_append_matches_refit_and_oracle(engine):
    """n_old = 300, q = 64 (the appended rows cross a 64-row block), d = 9, the linear kind: test_append.py's check of
    the appended state against a refit and against the oracle."""
    d = 9
    kp, op = ard_params("scale_linear_matern52", d, d, noise=2e-4, outputscale=1.3)
    AP.check_append_matches_refit_and_oracle(engine, kp, op, 300, 64, d, "ard d = 9")
