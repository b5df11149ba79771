"""gpx_svgp_acquire_f64 held to its storage contract, as tests/test_gpu_abi_strides.py holds the other calls (include/gpx.h,
Conventions): Z with rows ldz apart and tasks stride_z apart and Xs with rows ldxs apart, each a window of a wider
NaN-filled allocation, give the bits of tight storage; val_out[k], idx_out[k] and scores_out[m] are written in full and
nothing around them is; the const arguments are left as they were.  T = 2, M = 200, m = 700, k = 5."""
import ctypes

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd._capi import AcqParamsC, KernelParamsC
from bayesianoptimizer_amd.engine import ACQ_KINDS
from tests import abi_util as A
from tests import svgp_acquire_ref as AR
from tests import svgp_moments_ref as SR
from tests.abi_util import NAN, Win, ptr, same_bits, t
from tests.test_gpu_abi_strides import CASES, M, call, sync, unchanged
from tests.test_svgp import svgp_problem

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scores", [True, False], ids=["scores_out", "no_scores"])
@pytest.mark.parametrize("kind,d", CASES)
def test_svgp_acquire(engine, kind, d, scores):
    T, Mi, k, lib = 2, 200, 5, engine.lib
    Zn, vmean, vchol, kps, ops = svgp_problem(T, Mi, d, seed=T + Mi, kind=kind)
    Xn = np.random.default_rng(9).standard_normal((M, d))
    prep = engine.svgp_prepare(kps, Zn, vmean, vchol, jitter=SR.JITTER)
    w, ym, ys, best_f = [0.75, -0.5], [0.2, -0.1], [1.5, 0.5], 0.3
    tight = engine.svgp_acquire(prep, t(Xn), k, "logei", best_f=best_f, weights=w, y_mean=ym, y_scale=ys, index_offset=11,
                                return_scores=True)
    pcs = (KernelParamsC * T)(*[q.to_c(d) for q in kps])
    ldz, ldxs = d + 3, d + 5
    Z, sz = A.stack(T, (Mi, d), (ldz, 1), 7, NAN, t(Zn), lead=1)
    Z.freeze()
    Xs = A.rows(t(Xn), ldxs)
    W, W2, alpha = (Win(a.shape, None, NAN, a, lead=1).freeze() for a in (prep["W"], prep["W2"], prep["alpha"]))
    val, idx, sc = A.out_f64(k), A.out_i64(k), A.out_f64(M)
    ap = AcqParamsC()
    ap.kind, ap.best_f, ap.beta, ap.y_mean, ap.y_scale = ACQ_KINDS["logei"], best_f, 4.0, 0.0, 1.0
    dbl = lambda v: (ctypes.c_double * T)(*v)  # noqa: E731
    ws = A.plain_ws(A.ws_size(lib.gpx_svgp_acquire_workspace_size, Mi, M, k))
    call(engine, "gpx_svgp_acquire_f64", pcs, T, Mi, ptr(Z), ldz, sz, ptr(W), ptr(W2), ptr(alpha), dbl(w), dbl(ym),
         dbl(ys), ptr(Xs), M, ldxs, ctypes.byref(ap), 11, k, ptr(val), ptr(idx), ptr(sc) if scores else None, ptr(ws),
         ws.numel())
    sync()
    assert same_bits(val.view, tight[0]) and val.outside_intact() and val.sentinels() == 0
    assert torch.equal(idx.view, tight[1]) and idx.outside_intact() and idx.sentinels() == 0
    if scores:
        assert same_bits(sc.view, tight[2]) and sc.outside_intact() and sc.sentinels() == 0
    else:
        assert sc.sentinels() == M and sc.outside_intact()
    assert unchanged(Z, W, W2, alpha, Xs)
    mean, var = AR.latent_moments(Zn, vmean, vchol, ops, Xn)
    ref = AR.objective_scores(mean, var, "logei", w, ym, ys, best_f=best_f)
    assert np.abs(tight[2].cpu().numpy() - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
