"""gpx_svgp_condition_f64 held to its storage contract, as tests/test_gpu_abi_strides.py holds the other calls
(include/gpx.h, Conventions): Z with rows ldz apart and tasks stride_z apart, Xn with rows ldx apart, Yn with rows ldy
apart, vmean with tasks stride_m apart and vchol with rows ldc apart and tasks stride_c apart, each a window of a wider
NaN-filled allocation (and vchol's strict upper triangle NaN: only the lower one is read), give the bits of tight storage;
W2_out, alpha_out, vmean_out and vchol_out are written in full, the latter two with the inputs' strides, and nothing
around them is; the const arguments are left as they were.  T = 2, M = 200, n_new = 150."""
import numpy as np
import pytest
import torch

from bayesianoptimizer_amd.engine import KernelParamsC
from tests import abi_util as A
from tests import svgp_moments_ref as SR
from tests.abi_util import NAN, SENT, Win, ptr, same_bits, t
from tests.test_gpu_abi_strides import CASES, call, sync, unchanged
from tests.test_svgp import svgp_problem

pytestmark = pytest.mark.gpu
T, MI, K = 2, 200, 150


@pytest.mark.parametrize("pair", [True, False], ids=["pair", "no_pair"])
@pytest.mark.parametrize("kind,d", CASES)
def test_svgp_condition(engine, kind, d, pair):
    lib = engine.lib
    Zn, vmean, vchol, kps, _ = svgp_problem(T, MI, d, seed=T + MI, kind=kind)
    vmean, vchol = t(vmean), torch.tril(t(vchol))
    rng = np.random.default_rng(13)
    Xn, Yn = rng.standard_normal((K, d)), rng.standard_normal((K, T))
    prep = engine.svgp_prepare(kps, Zn, vmean, vchol, jitter=SR.JITTER)
    Mpad = prep["W2"].shape[1]
    tight = engine.svgp_condition(prep, t(Xn), t(Yn), vmean=vmean if pair else None, vchol=vchol if pair else None)
    pcs = (KernelParamsC * T)(*[q.to_c(d) for q in kps])
    ldz, ldx, ldy, ldc = d + 3, d + 5, T + 4, MI + 7
    Z, sz = A.stack(T, (MI, d), (ldz, 1), 7, NAN, t(Zn), lead=1)
    Z.freeze()
    X, Y = A.rows(t(Xn), ldx), A.rows(t(Yn), ldy, col0=2)
    W, W2, alpha = (Win(a.shape, None, NAN, a, lead=1).freeze() for a in (prep["W"], prep["W2"], prep["alpha"]))
    W2o, ao = A.out_f64(T, Mpad, Mpad), A.out_f64(T, Mpad)
    vm, sm = A.stack(T, (MI,), (1,), 5, NAN, vmean, lead=1)
    upper_nan = vchol + torch.triu(torch.full((MI, MI), NAN, dtype=torch.float64, device=A.DEV), 1)
    vc, sc = A.stack(T, (MI, MI), (ldc, 1), 11, NAN, upper_nan, lead=1)
    vm.freeze()
    vc.freeze()
    vmo, _ = A.stack(T, (MI,), (1,), 5, SENT, lead=1)
    vco, _ = A.stack(T, (MI, MI), (ldc, 1), 11, SENT, lead=1)
    info = A.out_i32(T)
    ws = A.plain_ws(A.ws_size(lib.gpx_svgp_condition_workspace_size, MI, K, T, 0))
    call(engine, "gpx_svgp_condition_f64", pcs, T, MI, ptr(Z), ldz, sz, ptr(W), ptr(W2), ptr(alpha), ptr(X), K, ldx,
         ptr(Y), ldy, ptr(W2o), ptr(ao), ptr(vm) if pair else None, sm, ptr(vc) if pair else None, ldc, sc,
         ptr(vmo) if pair else None, ptr(vco) if pair else None, ptr(info), ptr(ws), ws.numel())
    sync()
    assert info.view.tolist() == [0] * T and info.outside_intact()
    assert same_bits(W2o.view, tight[0]["W2"]) and W2o.outside_intact() and W2o.sentinels() == 0
    assert same_bits(ao.view, tight[0]["alpha"]) and ao.outside_intact() and ao.sentinels() == 0
    if pair:
        assert same_bits(vmo.view, tight[1]) and vmo.outside_intact() and vmo.sentinels() == 0
        assert same_bits(vco.view, tight[2]) and vco.outside_intact() and vco.sentinels() == 0
        assert not bool(torch.triu(vco.view, 1).any()) and bool((torch.diagonal(vco.view, dim1=1, dim2=2) > 0).all())
    else:
        assert vmo.sentinels() == T * MI and vco.sentinels() == T * MI * MI
        assert vmo.outside_intact() and vco.outside_intact()
    assert unchanged(Z, W, W2, alpha, X, Y, vm, vc)
    pad = tight[0]["W2"]
    assert not bool(pad[:, MI:, :].any()) and not bool(pad[:, :, MI:].any()) and not bool(tight[0]["alpha"][:, MI:].any())
