"""Every workspace-taking call in exactly the bytes its size query reports, poisoned (include/gpx.h, Conventions: a
workspace's contents on entry are arbitrary and its address needs only 8-byte alignment).

test_gpu_sweep_lazy.py (h) does this for the posterior, the single top-k sweep and the multi-output argmax; this module
repeats it for every other call.  Each runs through the engine's own method with ``engine.workspace`` replaced
(tests/abi_util.py GuardedWorkspace): every request is served from a fresh allocation of offset + asked + 4096 bytes of
0xFF, the workspace 0 or 8 bytes in.  Asserted: the results have the bits of the engine's call with its own workspace,
the bytes in front of the workspace and the 4 KiB behind it are still 0xFF, the engine asks for exactly what the size
query reports, and one byte less is rejected with GPX_INVALID_ARG.  gpx_alpha_f64 has no engine method of its own and is
called through ``engine.lib``.  Shapes as tests/test_gpu_abi_strides.py; the Monte-Carlo calls take B = 4, q = 3, nb = 5,
S = 64.
"""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import _capi
from tests import abi_util as A
from tests import svgp_moments_ref as SR
from tests.abi_util import GuardedWorkspace, ptr, same_bits, t
from tests.test_gpu_abi_strides import BATCH, M, MB, N, NB, NF, NRHS, Q, batch_inputs, prob, tight_fit
from tests.test_svgp import svgp_problem

pytestmark = pytest.mark.gpu
KIND, D = "rbf", 3
S, B = 64, 4
CALLS = ["fit", "fit_factor", "trtri", "trtri_batched", "potrs", "fit_batched", "fit_factor_batched", "fit_batched_params",
         "append", "argmax_full", "argmax_pruned", "argmax_fused", "topk_multi", "moments_grad", "joint_moments", "mll",
         "mll_batched", "svgp_prepare", "svgp_predict", "svgp_moments_grad", "mc_acq", "mc_nei", "topk"]


def mc_inputs():
    rng = np.random.default_rng(3)
    mean = rng.standard_normal((B, Q))
    G = rng.standard_normal((B, Q, Q))
    cov = G @ G.transpose(0, 2, 1) + np.eye(Q)
    cross = 0.1 * rng.standard_normal((B, Q, NB))
    H = rng.standard_normal((NB, NB))
    Linv = np.linalg.inv(np.linalg.cholesky(H @ H.T + NB * np.eye(NB)))
    zb, zq = rng.standard_normal((S, NB)), rng.standard_normal((S, Q))
    return tuple(t(a) for a in (mean, cov, cross, Linv, zb, rng.standard_normal(S), zq))


def clones(*tensors):
    return tuple(None if a is None else a.clone() for a in tensors)


def state_arrays(st, inverse=True):
    return clones(torch.tril(st.L), st.Dinv[:st.Dinv.shape[0] // 2], st.W if inverse else None, st.alpha, st.info)


def build(engine, call):
    """(run, sizes): ``run()`` makes the engine's call and returns its results as new tensors; ``sizes`` are the bytes the
    size queries report for the workspaces it asks for, in order."""
    lib, size = engine.lib, A.ws_size
    p = prob(KIND, D, NF if call == "argmax_fused" else N)
    X, Y, kp, Xs, Xq = t(p.X), t(p.Y), p.kp, t(p.Xs), t(p.Xq)
    kps = [kp, kp.replace(outputscale=1.7, const_mean=-0.1), kp.replace(noise=3e-4)]
    if call in ("fit", "fit_factor"):
        inv = call == "fit"
        q = lib.gpx_fit_workspace_size if inv else lib.gpx_fit_factor_workspace_size
        return (lambda: state_arrays(engine.fit(X, Y, kp, inverse=inv), inv)), [size(q, N, NRHS)]
    if call == "trtri":
        st = engine.fit(X, Y, kp)

        def run():
            st.W_ready = False
            return clones(engine.inverse(st).W)
        return run, [size(lib.gpx_trtri_workspace_size, N)]
    if call == "trtri_batched":
        sts = engine.fit_batched(*batch_inputs(p), kp)

        def run():
            for st in sts:
                st.W_ready = False
            engine.inverse_batched(sts)
            return clones(sts[0]._batch[1])
        return run, [size(lib.gpx_trtri_batched_workspace_size, N, BATCH)]
    if call == "potrs":
        st = tight_fit(engine, KIND, D)
        return (lambda: (engine.potrs(st, Y),)), [size(lib.gpx_potrs_workspace_size, N, NRHS)]
    if call in ("fit_batched", "fit_factor_batched", "fit_batched_params"):
        inv = "factor" not in call
        Xd, Yd = batch_inputs(p)
        q = lib.gpx_fit_batched_workspace_size if inv else lib.gpx_fit_factor_batched_workspace_size

        def run():
            Lb, Wb, Db, Ab, Ib = engine.fit_batched(Xd, Yd, kps if "params" in call else kp, inverse=inv)[0]._batch
            return clones(torch.tril(Lb), Db[:, :Db.shape[1] // 2], Wb if inv else None, Ab, Ib)
        return run, [size(q, N, NRHS, BATCH)]
    if call == "append":
        def run():
            st = engine.fit(X[:NF], Y[:NF], kp, capacity=N, inverse=True)
            return state_arrays(engine.append(st, X, Y))
        return run, [size(lib.gpx_fit_workspace_size, NF, NRHS), size(lib.gpx_append_workspace_size, NF, N, NRHS)]
    if call.startswith("argmax"):
        st = tight_fit(engine, KIND, D, p.n)
        engine.inverse(st)
        prune = 2 if call == "argmax_pruned" else 0

        def run():
            before = engine.get_option("sweep_prune")
            engine.set_option("sweep_prune", prune)
            try:
                return engine.acquire(st, Xs, "logei", best_f=float(p.Y[:, 0].max()))
            finally:
                engine.set_option("sweep_prune", before)
        return run, [size(lib.gpx_sweep_workspace_size, p.n, 1, M)]
    if call == "topk_multi":
        sts = engine.fit_outputs(X, Y[:, :2], kps[:2], inverse=True)
        return (lambda: engine.acquire_topk_multi(sts, Xs, 5, "ucb", weights=[0.5, 1.0])), \
            [size(lib.gpx_acquire_topk_multi_workspace_size, N, M, 5)]
    if call == "moments_grad":
        st = tight_fit(engine, KIND, D)
        return (lambda: engine.moments_grad(st, Xq, Q)), [size(lib.gpx_moments_grad_workspace_size, N, 4 * Q)]
    if call == "joint_moments":
        st = tight_fit(engine, KIND, D)

        def run():
            mean_b, cov_bb, Sb = engine.joint_moments(st, t(p.Xb))
            return mean_b, cov_bb, Sb[:, :MB]
        return run, [size(lib.gpx_joint_moments_workspace_size, N, MB)]
    if call == "mll":
        st = tight_fit(engine, KIND, D)
        return (lambda: (engine.mll_grad(st, Y),)), [size(lib.gpx_mll_workspace_size, N)]
    if call == "mll_batched":
        sts = engine.fit_outputs(X, Y, kps, inverse=True)
        return (lambda: (engine.mll_grad_outputs(sts, Y),)), [size(lib.gpx_mll_workspace_size, N)]
    if call.startswith("svgp"):
        T, Mi = 2, 200
        Z, vmean, vchol, skp, _ = svgp_problem(T, Mi, D, seed=T + Mi, kind=KIND)
        if call == "svgp_prepare":
            def run():
                prep = engine.svgp_prepare(skp, Z, vmean, vchol, jitter=SR.JITTER)
                return prep["W"], prep["W2"], prep["alpha"]
            return run, [size(lib.gpx_svgp_prepare_workspace_size, Mi, T)]
        prep = engine.svgp_prepare(skp, Z, vmean, vchol, jitter=SR.JITTER)
        Xn = t(np.random.default_rng(9).standard_normal((M, D)))
        if call == "svgp_predict":
            return (lambda: engine.svgp_predict(prep, Xn)), [size(lib.gpx_svgp_predict_workspace_size, Mi, M)]
        return (lambda: engine.svgp_moments_grad(prep, 1, Xq, Q)), \
            [size(lib.gpx_svgp_moments_grad_workspace_size, Mi, 4 * Q)]
    mean, cov, cross, Linv, zb, best, zq = mc_inputs()
    if call == "mc_acq":
        return (lambda: engine.mc_acq(mean, cov, zq, "qlogei", best_f=0.2)), [size(lib.gpx_mc_acq_workspace_size, B, Q, S)]
    if call == "mc_nei":
        return (lambda: engine.mc_nei(mean, cov, cross, Linv, zb, best, zq, log=True)), \
            [size(lib.gpx_mc_nei_workspace_size, B, Q, NB, S)]
    assert call == "topk"
    scores = t(np.random.default_rng(4).standard_normal(M))
    return (lambda: engine.topk(scores, 20)), [size(lib.gpx_topk_workspace_size, M)]


@pytest.mark.parametrize("offset", [0, 8])
@pytest.mark.parametrize("call", CALLS)
def test_workspace_of_exactly_the_reported_size(engine, monkeypatch, call, offset):
    run, sizes = build(engine, call)
    want = run()
    torch.cuda.synchronize()
    # one byte less for the call's own (last) request: rejected
    short = GuardedWorkspace(offset, short_at=len(sizes) - 1)
    monkeypatch.setattr(engine, "workspace", short)
    with pytest.raises(_capi.GPXError, match="workspace too small") as e:
        run()
    assert e.value.status == _capi.GPX_INVALID_ARG
    assert short.guards_intact()
    guarded = GuardedWorkspace(offset)
    monkeypatch.setattr(engine, "workspace", guarded)
    got = run()
    assert guarded.guards_intact(), "a kernel wrote outside the reported workspace"
    assert guarded.asked == sizes  # the engine asks for what the size queries report, each request served separately
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert (a is None and b is None) or same_bits(a, b), f"{call}: differs from the run in the engine's workspace"


@pytest.mark.parametrize("offset", [0, 8])
def test_alpha_workspace_of_exactly_the_reported_size(engine, offset):
    """gpx_alpha_f64 through the C ABI (the engine reaches it only inside gpx_fit_f64): alpha has the fit's bits."""
    p, st = prob(KIND, D), tight_fit(engine, KIND, D)
    Y, nb = t(p.Y), A.ws_size(engine.lib.gpx_alpha_workspace_size, N, NRHS)
    big = torch.full((offset + nb + A.GUARD,), 0xFF, dtype=torch.uint8, device=A.DEV)
    alpha = torch.full_like(st.alpha, A.SENT)
    engine._bind_stream()
    for size, status in ((nb - 1, _capi.GPX_INVALID_ARG), (nb, _capi.GPX_OK)):
        assert engine.lib.gpx_alpha_f64(engine.handle, N, ptr(st.W), st.W.stride(0), ptr(Y), NRHS, NRHS, p.kp.const_mean,
                                        ptr(alpha), ctypes.c_void_p(big.data_ptr() + offset), size) == status
        torch.cuda.synchronize()
        assert bool((alpha == A.SENT).all()) == (status != _capi.GPX_OK)
    assert same_bits(alpha, st.alpha)
    assert bool((big[:offset] == 0xFF).all()) and bool((big[offset + nb:] == 0xFF).all())
