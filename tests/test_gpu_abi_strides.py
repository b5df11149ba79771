"""Strided and offset storage through the C ABI gives the bits of tight storage (include/gpx.h, Conventions).

Every entry point runs twice: through GPEngine (tight: ldx = d, ldy = nrhs, matrix pitches npad or a multiple of 128) and
through ``engine.lib`` with every leading dimension and stride loosened: ldx = d + 3, ldxs = d + 5, ldxb = d + 1, Y a
column window (ldy = nrhs + 4 from column 2), matrix pitches even but no multiple of 64 (npad + 2, npad + 6), ldmean =
nrhs + 1, gaps between the problems of a batch.  Input gaps hold NaN, outputs are pre-filled with a sentinel over their
whole allocation (tests/abi_util.py).  Asserted for every call: (1) the defined region has the tight result's bits,
(2) it agrees with the oracle at the tolerance of the call's parity test, (3) nothing outside the defined region is
written, (4) no sentinel survives inside it, (5) the const inputs are unchanged.

Shapes: n = 300 (padded 384: three row tiles, the smallest pruned / lazy size), n = 200 for the fused sweep, d = 3 (the
DMAX = 4 instances) and 17 (the DMAX = 32 ones at their narrowest), nrhs = 3, m = 700, q-batches 4 x 3, mb = 70, nb = 5,
SVGP T = 2, M = 200.  One more size, padded n = 8192, for gpx_trtri_f64 alone: the smallest at which the inverse takes its
128 x 128 tile kernels.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bayesianoptimizer_amd import _capi
from bayesianoptimizer_amd._capi import AcqParamsC, KernelParamsC
from bayesianoptimizer_amd.engine import ACQ_KINDS
from oracle import gp_oracle as O
from tests import abi_util as A
from tests import svgp_moments_ref as SR
from tests.abi_util import NAN, SENT, Win, ok, ptr, same_bits, t
from tests.test_gpu_parity import RTOL, check_argmax, check_posterior, pair
from tests.test_mll import to_oracle
from tests.test_svgp import svgp_problem

pytestmark = pytest.mark.gpu
CASES = [("rbf", 3), ("rbf", 17), ("scale_linear_matern52", 3)]
N, NF, M, NRHS, Q, NB, MB, BATCH = 300, 200, 700, 3, 3, 5, 70, 3
_tight = {}


@functools.lru_cache(maxsize=None)
def prob(kind, d, n=N):
    X, y = O.synthetic_problem(n, d, 21)
    Y = np.stack([y, np.sin(3 * X).sum(1), np.cos(2 * X).sum(1)], 1)
    kp, op = pair(kind, d, noise=1e-4, outputscale=1.3, const_mean=0.15)
    rng = np.random.default_rng(d)
    return SimpleNamespace(X=X, Y=Y, kp=kp, op=op, d=d, n=n, Xs=O.sobol_candidates(M, d, 22), Xq=rng.random((4 * Q, d)),
                           Xb=rng.random((MB, d)))


def tight_fit(engine, kind, d, n=N):
    """The engine's fit with W (gpx_fit_f64, tight storage), once per configuration and never modified."""
    key = (kind, d, n)
    if key not in _tight:
        p = prob(kind, d, n)
        _tight[key] = engine.fit(t(p.X), t(p.Y), p.kp, inverse=True)
    return _tight[key]


def loose_state(p, st):
    """The fitted state's const arrays as a loose caller holds them."""
    npad = st.npad
    return SimpleNamespace(X=A.rows(t(p.X), p.d + 3), Y=A.rows(t(p.Y), NRHS + 4, col0=2),
                           L=A.matrix(npad, npad + 2, NAN, st.L).freeze(), W=A.matrix(npad, npad + 6, NAN, st.W).freeze(),
                           Dinv=Win(st.Dinv.shape, None, NAN, st.Dinv).freeze(),
                           alpha=Win(st.alpha.shape, None, NAN, st.alpha, lead=1).freeze(),
                           a0=Win((npad,), None, NAN, st.alpha[:, 0], lead=1).freeze(),
                           Xs=A.rows(t(p.Xs), p.d + 5), Xq=A.rows(t(p.Xq), p.d + 5), Xb=A.rows(t(p.Xb), p.d + 1))


def unchanged(*wins):
    return all(w.unchanged() for w in wins)


def call(engine, name, *args):
    engine._bind_stream()
    ok(engine, getattr(engine.lib, name)(engine.handle, *args))


def sync():
    torch.cuda.synchronize()


def half(Dinv):
    return Dinv.reshape(-1)[:Dinv.numel() // 2]


def check_factor(K, Dinv, info, tight, p, n, what, oracle=True):
    """K (in/out: L in its lower triangle), the first half of Dinv and info of one problem against the tight state."""
    assert same_bits(torch.tril(K), torch.tril(tight.L)), f"{what}: L differs from the tight run"
    assert same_bits(half(Dinv), half(tight.Dinv)), f"{what}: Dinv differs from the tight run"
    assert int(info.item()) == 0
    assert not bool((torch.tril(K) == SENT).any()) and not bool(torch.isnan(torch.tril(K)).any()), what
    assert not bool((half(Dinv) == SENT).any()), what
    if oracle:
        Lr = O.cholesky(O.gram(p.X[:n], p.op))
        L = np.tril(K.cpu().numpy())
        assert np.abs(L[:n, :n] - Lr).max() <= RTOL * np.abs(Lr).max()
        np.testing.assert_array_equal(L[n:, n:], np.eye(L.shape[0] - n))


def check_inverse(W, L, tight, what):
    assert same_bits(W, tight.W), f"{what}: W differs from the tight run"
    assert not bool((W == SENT).any()) and A.lower_zero(W), what
    Wn, Ln = np.triu(W.cpu().numpy()), np.tril(L.cpu().numpy())
    np.testing.assert_allclose(Wn.T @ Ln, np.eye(Ln.shape[0]), atol=1e-9)


def check_alpha(alpha, tight_alpha, alpha_ref, n, what, rtol=1e-8):
    assert same_bits(alpha, tight_alpha), f"{what}: alpha differs from the tight run"
    assert not bool((alpha == SENT).any()) and not bool(alpha[n:].any()), what
    a = alpha[:n].cpu().numpy()
    assert np.abs(a - alpha_ref.reshape(a.shape)).max() <= rtol * np.abs(alpha_ref).max()


def dinv_win(npad, fill=SENT, data=None):
    return Win((2 * (npad // 64) * 64 * 64,), None, fill, None if data is None else data.reshape(-1))


# ---- the stages of the fit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", CASES)
def test_gram(engine, kind, d):
    p = prob(kind, d)
    tight = engine.gram(t(p.X), p.kp)
    npad = tight.shape[0]
    X, K, pc = A.rows(t(p.X), d + 3), A.matrix(npad, npad + 2), p.kp.to_c(d)
    call(engine, "gpx_gram_f64", ctypes.byref(pc), N, ptr(X), d + 3, ptr(K), npad + 2)
    sync()
    low = torch.tril(K.view)
    assert same_bits(low, torch.tril(tight))
    Kr, Kg = O.gram(p.X, p.op), low.cpu().numpy()
    assert np.abs(Kg[:N, :N] - np.tril(Kr)).max() <= 1e-14 * np.abs(Kr).max()
    np.testing.assert_array_equal(Kg[N:, N:], np.eye(npad - N))
    assert not np.any(Kg[N:, :N])
    assert K.outside_intact() and not bool((low == SENT).any()) and X.unchanged()


@pytest.mark.parametrize("kind,d", CASES[1:])
def test_potrf_trtri_alpha_potrs(engine, kind, d):
    """gpx_potrf_f64 (lda), gpx_trtri_f64 (ldl, ldw), gpx_alpha_f64 (ldw, ldy) and gpx_potrs_f64 (ldl, ldy), each on
    loose copies of the tight stage before it."""
    p, st = prob(kind, d), tight_fit(engine, kind, d)
    npad, lib = st.npad, engine.lib
    K0 = engine.gram(t(p.X), p.kp)
    Kt = K0.clone()
    Dt, it = engine.potrf(Kt, N)
    tight = SimpleNamespace(L=Kt, Dinv=Dt, W=engine.trtri(Kt, Dt, N))
    assert same_bits(torch.tril(Kt), torch.tril(st.L))  # the stages are the fit's
    # potrf
    Aw, Dinv, info = A.matrix(npad, npad + 2, NAN, K0), dinv_win(npad), A.out_i32()
    call(engine, "gpx_potrf_f64", N, ptr(Aw), npad + 2, ptr(Dinv), ptr(info))
    sync()
    check_factor(Aw.view, Dinv.view, info.view, tight, p, N, "potrf")
    D, Ln = Dinv.view.reshape(-1, 64, 64).cpu().numpy(), np.tril(Aw.view.cpu().numpy())
    for b in range(npad // 64):
        np.testing.assert_allclose(D[b] @ Ln[64 * b:64 * b + 64, 64 * b:64 * b + 64], np.eye(64), atol=1e-10)
    assert Aw.outside_intact() and Dinv.outside_intact() and info.outside_intact()
    # trtri
    s = loose_state(p, SimpleNamespace(npad=npad, L=Kt, W=tight.W, Dinv=Dt, alpha=st.alpha))
    W = A.matrix(npad, npad + 6)
    ws = A.plain_ws(A.ws_size(lib.gpx_trtri_workspace_size, N))
    call(engine, "gpx_trtri_f64", N, ptr(s.L), npad + 2, ptr(s.Dinv), ptr(W), npad + 6, ptr(ws), ws.numel())
    sync()
    check_inverse(W.view, Kt, tight, "trtri")
    assert W.outside_intact() and unchanged(s.L, s.Dinv)
    # alpha = W W^T (Y - m)
    ar = O.fit(p.X, p.Y, p.op).alpha
    alpha = A.out_f64(npad, NRHS)
    ws = A.plain_ws(A.ws_size(lib.gpx_alpha_workspace_size, N, NRHS))
    call(engine, "gpx_alpha_f64", N, ptr(s.W), npad + 6, ptr(s.Y), NRHS + 4, NRHS, p.kp.const_mean, ptr(alpha), ptr(ws),
         ws.numel())
    sync()
    check_alpha(alpha.view, st.alpha, ar, N, "alpha")
    assert alpha.outside_intact() and unchanged(s.W, s.Y)
    # potrs: the triangular solves on L
    alpha, info = A.out_f64(npad, NRHS), Win((1,), None, A.ISENT, torch.zeros(1), dtype=torch.int32, lead=1, tail=3)
    ws = A.plain_ws(A.ws_size(lib.gpx_potrs_workspace_size, N, NRHS))
    call(engine, "gpx_potrs_f64", N, ptr(s.L), npad + 2, ptr(s.Dinv), ptr(s.Y), NRHS + 4, NRHS, p.kp.const_mean,
         ptr(alpha), ptr(info), ptr(ws), ws.numel())
    sync()
    check_alpha(alpha.view, engine.potrs(st, t(p.Y)), ar, N, "potrs")
    assert int(info.view.item()) == 0 and info.outside_intact() and alpha.outside_intact()
    assert unchanged(s.L, s.Dinv, s.Y)


@pytest.mark.parametrize("inverse", [True, False], ids=["fit", "fit_factor"])
@pytest.mark.parametrize("kind,d", CASES)
def test_fit(engine, kind, d, inverse):
    """gpx_fit_f64 (ldx, ldy, ldk, ldw) and gpx_fit_factor_f64 (ldx, ldy, ldk)."""
    p = prob(kind, d)
    tight = tight_fit(engine, kind, d) if inverse else engine.fit(t(p.X), t(p.Y), p.kp)
    npad, lib, pc = tight.npad, engine.lib, p.kp.to_c(d)
    X, Y = A.rows(t(p.X), d + 3), A.rows(t(p.Y), NRHS + 4, col0=2)
    K, W, Dinv, alpha, info = A.matrix(npad, npad + 2), A.matrix(npad, npad + 6), dinv_win(npad), \
        A.out_f64(npad, NRHS), A.out_i32()
    if inverse:
        ws = A.plain_ws(A.ws_size(lib.gpx_fit_workspace_size, N, NRHS))
        call(engine, "gpx_fit_f64", ctypes.byref(pc), N, ptr(X), d + 3, ptr(Y), NRHS + 4, NRHS, ptr(K), npad + 2,
             ptr(Dinv), ptr(W), npad + 6, ptr(alpha), ptr(info), ptr(ws), ws.numel())
    else:
        ws = A.plain_ws(A.ws_size(lib.gpx_fit_factor_workspace_size, N, NRHS))
        call(engine, "gpx_fit_factor_f64", ctypes.byref(pc), N, ptr(X), d + 3, ptr(Y), NRHS + 4, NRHS, ptr(K), npad + 2,
             ptr(Dinv), ptr(alpha), ptr(info), ptr(ws), ws.numel())
    sync()
    check_factor(K.view, Dinv.view, info.view, tight, p, N, "fit")
    check_alpha(alpha.view, tight.alpha, O.fit(p.X, p.Y, p.op).alpha, N, "fit")
    if inverse:
        check_inverse(W.view, K.view, tight, "fit")
    else:
        assert W.sentinels() == W.view.numel()
    assert all(w.outside_intact() for w in (K, W, Dinv, alpha, info)) and unchanged(X, Y)


def run_batched_fit(engine, entry, params, p, Xd, Yd, nrhs, shared_x, tights, what):
    """One batched fit through the C ABI with gaps on every stride.  Xd: BATCH x n x d, or n x d with ``shared_x``
    (stride_x = 0); then Yd is the n x BATCH target matrix read column by column (stride_y = 1, ldy = BATCH, nrhs = 1),
    else BATCH x n x nrhs.  tights: the engine's state of every problem."""
    d, npad, lib = p.d, tights[0].npad, engine.lib
    ldk, ldw = npad + 2, npad + 6
    if shared_x:
        X, ldx, sx = A.rows(Xd, d + 3), d + 3, 0
        Y, ldy, sy = Win(Yd.shape, None, NAN, Yd, lead=1).freeze(), BATCH, 1
    else:
        ldx, ldy = d + 3, nrhs + 4
        X, sx = A.stack(BATCH, (N, d), (ldx, 1), 7, NAN, Xd, lead=1)
        Y, sy = A.stack(BATCH, (N, nrhs), (ldy, 1), 5, NAN, Yd, lead=3)
        X.freeze(), Y.freeze()
    K, sk = A.stack(BATCH, (npad, npad), (ldk, 1), 10)
    W, sw = A.stack(BATCH, (npad, npad), (ldw, 1), 14)
    Dinv, sd = A.stack(BATCH, (2 * (npad // 64) * 4096,), (1,), 6)
    alpha, sa = A.stack(BATCH, (npad, nrhs), (nrhs, 1), 3, lead=1)
    info = A.out_i32(BATCH)
    factor = "factor" in entry
    per = isinstance(params, (list, tuple))
    pcs = (KernelParamsC * BATCH)(*[q.to_c(d) for q in params]) if per else params.to_c(d)
    pref = pcs if per else ctypes.byref(pcs)
    size = lib.gpx_fit_factor_batched_workspace_size if factor else lib.gpx_fit_batched_workspace_size
    ws = A.plain_ws(A.ws_size(size, N, nrhs, BATCH))
    args = [pref, BATCH, N, ptr(X), ldx, sx, ptr(Y), ldy, sy, nrhs, ptr(K), ldk, sk, ptr(Dinv), sd]
    if not factor:
        args += [ptr(W), ldw, sw]
    call(engine, entry, *args, ptr(alpha), sa, ptr(info), ptr(ws), ws.numel())
    sync()
    for b, tight in enumerate(tights):
        pb = SimpleNamespace(X=(Xd if shared_x else Xd[b]).cpu().numpy(),
                             op=to_oracle(params[b] if per else params, d))
        check_factor(K.view[b], Dinv.view[b], info.view[b], tight, pb, N, f"{what} problem {b}")
        yb = (Yd[:, b:b + 1] if shared_x else Yd[b]).cpu().numpy()
        check_alpha(alpha.view[b], tight.alpha, O.fit(pb.X, yb, pb.op).alpha, N, f"{what} problem {b}", rtol=1e-6)
        if not factor:
            check_inverse(W.view[b], K.view[b], tight, f"{what} problem {b}")
    if factor:
        assert W.sentinels() == W.view.numel()
    assert all(w.outside_intact() for w in (K, W, Dinv, alpha, info)), f"{what}: a gap was written"
    assert unchanged(X, Y)


def batch_inputs(p):
    Xd = torch.stack([t(p.X), t(p.X[::-1].copy()), t(0.5 * p.X + 0.1)])
    Yd = torch.stack([t(p.Y), t(p.Y[::-1].copy()), t(2.0 * p.Y - 0.3)])
    return Xd, Yd


@pytest.mark.parametrize("form", ["strided", "shared_x"])
@pytest.mark.parametrize("entry", ["gpx_fit_batched_f64", "gpx_fit_factor_batched_f64", "gpx_fit_batched_params_f64"])
@pytest.mark.parametrize("kind,d", CASES[1:])
def test_fit_batched(engine, kind, d, entry, form):
    """batch = 3 with gaps between the problems on every stride_*, and the documented shared form: stride_x = 0,
    stride_y = 1, ldy = batch (the outputs keep their gaps)."""
    p = prob(kind, d)
    inverse = "factor" not in entry
    params = [p.kp, p.kp.replace(outputscale=1.7, const_mean=-0.1), p.kp.replace(noise=3e-4)] \
        if "params" in entry else p.kp
    if form == "strided":
        Xd, Yd = batch_inputs(p)
        tights = engine.fit_batched(Xd, Yd, params, inverse=inverse)
        run_batched_fit(engine, entry, params, p, Xd, Yd, NRHS, False, tights, f"{entry} strided")
    else:
        Xd, Yd = t(p.X), t(p.Y)
        plist = params if isinstance(params, list) else [params] * BATCH
        # (the header: a problem of a batch has the bits of the single fit with its parameters)
        tights = [engine.fit(Xd, Yd[:, b], plist[b], inverse=inverse) for b in range(BATCH)]
        run_batched_fit(engine, entry, params, p, Xd, Yd, 1, True, tights, f"{entry} shared X")


@pytest.mark.parametrize("kind,d", CASES[1:])
def test_trtri_batched(engine, kind, d):
    """gpx_trtri_batched_f64: ldl, stride_l, stride_dinv, ldw, stride_w."""
    p = prob(kind, d)
    Xd, Yd = batch_inputs(p)
    sts = engine.fit_batched(Xd, Yd, p.kp, inverse=False)
    npad = sts[0].npad
    Lb, _, Db, _, _ = sts[0]._batch
    L, sl = A.stack(BATCH, (npad, npad), (npad + 2, 1), 10, NAN, Lb)
    Dinv, sd = A.stack(BATCH, (Db[0].numel(),), (1,), 6, NAN, Db.reshape(BATCH, -1))
    W, sw = A.stack(BATCH, (npad, npad), (npad + 6, 1), 14)
    L.freeze(), Dinv.freeze()
    ws = A.plain_ws(A.ws_size(engine.lib.gpx_trtri_batched_workspace_size, N, BATCH))
    call(engine, "gpx_trtri_batched_f64", BATCH, N, ptr(L), npad + 2, sl, ptr(Dinv), sd, ptr(W), npad + 6, sw, ptr(ws),
         ws.numel())
    sync()
    engine.inverse_batched(sts)
    for b in range(BATCH):
        check_inverse(W.view[b], Lb[b], sts[b], f"problem {b}")
    assert W.outside_intact() and unchanged(L, Dinv)


def test_trtri_128_tile_level(engine):
    """Padded n = 8192 is the smallest size whose inverse runs a level on the 128 x 128 tiles (the hand-placed k loop of
    gpx_trmm_asm.h): the same loose pitches, all of W written (the tiles below the diagonal by the W12 step of the level
    that owns their transposed position) and the bits of the tight run.  Tolerance and row sample of
    tests/test_gpu_parity.py::test_large_fit_inverse_and_factor_rows."""
    n, d = 8100, 8
    X, y = O.synthetic_problem(n, d, 1)
    kp, _ = pair("rbf", d, noise=1e-4)
    st = engine.fit(t(X), t(y), kp)
    npad = st.npad
    L, Dinv, W = A.matrix(npad, npad + 2, NAN, st.L).freeze(), Win(st.Dinv.shape, None, NAN, st.Dinv).freeze(), \
        A.matrix(npad, npad + 6)
    ws = A.plain_ws(A.ws_size(engine.lib.gpx_trtri_workspace_size, n))
    call(engine, "gpx_trtri_f64", n, ptr(L), npad + 2, ptr(Dinv), ptr(W), npad + 6, ptr(ws), ws.numel())
    sync()
    engine.inverse(st)
    assert same_bits(W.view, st.W)
    assert W.sentinels() == 0 and A.lower_zero(W.view) and W.outside_intact() and unchanged(L, Dinv)
    ri = torch.tensor(np.sort(np.random.default_rng(n).choice(n, 16, replace=False)), device=A.DEV)
    prod = W.view[:n, :n].T[ri] @ torch.tril(st.L[:n, :n])
    eye = torch.zeros_like(prod)
    eye[torch.arange(16, device=A.DEV), ri] = 1.0
    assert (prod - eye).abs().max().item() <= 1e-9


@pytest.mark.parametrize("kind,d", CASES)
def test_append(engine, kind, d):
    """gpx_append_f64 200 -> 300 (ldx, ldy, ldl, ldw): the old fit's leading 256 x 256 blocks in sentinel-filled L / W."""
    p = prob(kind, d)
    n0, npad0 = NF, 256
    st = engine.fit(t(p.X[:n0]), t(p.Y[:n0]), p.kp, capacity=N, inverse=True)
    L0, W0, D0 = st.L.clone(), st.W.clone(), st.Dinv.clone()
    tight = engine.append(st, t(p.X), t(p.Y))
    npad, pc = tight.npad, p.kp.to_c(d)
    assert npad == 384 and tight.L.stride(0) == npad
    X, Y = A.rows(t(p.X), d + 3), A.rows(t(p.Y), NRHS + 4, col0=2)
    L, W, Dinv = A.matrix(npad, npad + 2), A.matrix(npad, npad + 6), dinv_win(npad)
    L.view[:npad0, :npad0].copy_(L0)
    W.view[:npad0, :npad0].copy_(W0)
    Dinv.view[:npad0 // 64 * 4096].copy_(D0.reshape(-1)[:npad0 // 64 * 4096])
    alpha, info = A.out_f64(npad, NRHS), A.out_i32()
    ws = A.plain_ws(A.ws_size(engine.lib.gpx_append_workspace_size, n0, N, NRHS))
    call(engine, "gpx_append_f64", ctypes.byref(pc), n0, N, ptr(X), d + 3, ptr(Y), NRHS + 4, NRHS, ptr(L), npad + 2,
         ptr(Dinv), ptr(W), npad + 6, ptr(alpha), ptr(info), ptr(ws), ws.numel())
    sync()
    check_factor(L.view, Dinv.view, info.view, tight, p, N, "append")
    check_inverse(W.view, L.view, tight, "append")
    check_alpha(alpha.view, tight.alpha, O.fit(p.X, p.Y, p.op).alpha, N, "append")
    assert all(w.outside_intact() for w in (L, W, Dinv, alpha, info)) and unchanged(X, Y)


# ---- posterior and the sweeps ----------------------------------------------------------------------------------------
SWEEP_CASES = [(k, d, N) for k, d in CASES] + [("rbf", 3, NF)]


@pytest.mark.parametrize("kind,d,n", SWEEP_CASES)
def test_posterior(engine, kind, d, n):
    """gpx_posterior_f64: ldx, ldw, ldxs, ldmean; n = 200 takes the fused small-n sweep."""
    p, st = prob(kind, d, n), tight_fit(engine, kind, d, n)
    npad, pc = st.npad, p.kp.to_c(d)
    ym, ys = [0.5 * r for r in range(NRHS)], [1.0 + r for r in range(NRHS)]
    mu_t, var_t = engine.posterior(st, t(p.Xs), ym, ys)
    s = loose_state(p, st)
    mean, var = Win((M, NRHS), (NRHS + 1, 1), SENT, lead=1, tail=4), A.out_f64(M)
    ws = A.plain_ws(A.ws_size(engine.lib.gpx_sweep_workspace_size, n, NRHS, M))
    call(engine, "gpx_posterior_f64", ctypes.byref(pc), n, ptr(s.X), d + 3, ptr(s.W), npad + 6, ptr(s.alpha), NRHS,
         ptr(s.Xs), M, d + 5, (ctypes.c_double * NRHS)(*ym), (ctypes.c_double * NRHS)(*ys), ptr(mean), NRHS + 1,
         ptr(var), ptr(ws), ws.numel())
    sync()
    assert same_bits(mean.view, mu_t) and same_bits(var.view, var_t)
    mu_r, var_r = O.posterior(O.fit(p.X, p.Y, p.op), p.Xs)
    mu_r = np.asarray(ym) + np.asarray(ys) * mu_r.reshape(M, NRHS)
    var_r = np.maximum(var_r * ys[0] ** 2, 1e-12)
    check_posterior(mean.view.cpu().numpy(), var.view.cpu().numpy(), mu_r, var_r, O.kernel_diag(p.Xs, p.op) * ys[0] ** 2)
    assert mean.outside_intact() and var.outside_intact() and mean.sentinels() == 0 and var.sentinels() == 0
    assert unchanged(s.X, s.W, s.alpha, s.Xs)


def acq_params(p, acq="logei"):
    ap = AcqParamsC()
    ap.kind, ap.best_f, ap.beta, ap.y_mean, ap.y_scale = ACQ_KINDS[acq], 0.3 + 1.7 * float(p.Y[:, 0].max()), 4.0, 0.3, 1.7
    return ap, dict(best_f=ap.best_f, beta=4.0, y_mean=0.3, y_scale=1.7)


def oracle_scores(p, acq="logei"):
    ost = O.fit(p.X, p.Y[:, 0], p.op)
    ap, _ = acq_params(p, acq)
    mu, var = O.posterior(ost, p.Xs, 0.3, 1.7)
    return O.acquisition(mu, var, ACQ_KINDS[acq], ap.best_f, 4.0), (mu - ap.best_f) / np.sqrt(var)


def check_scores(sg, sref, u):
    keep = u > -10  # (tests/test_gpu_parity.py: logEI where the improvement is not astronomically small)
    assert np.abs(sg[keep] - sref[keep]).max() <= 1e-8 * max(1.0, np.abs(sref[keep]).max())


def with_prune(engine, prune, fn):
    before = engine.get_option("sweep_prune")
    engine.set_option("sweep_prune", prune)
    try:
        out = fn()
        sync()
        return out
    finally:
        engine.set_option("sweep_prune", before)


@pytest.mark.parametrize("prune", [0, 2])
@pytest.mark.parametrize("kind,d,n", SWEEP_CASES)
def test_acquire_argmax(engine, kind, d, n, prune):
    """gpx_acquire_argmax_f64 (ldx, ldw, ldxs) with sweep_prune 0 and 2, without and (the full sweep) with scores_out."""
    p, st = prob(kind, d, n), tight_fit(engine, kind, d, n)
    npad, pc, off = st.npad, p.kp.to_c(d), 7 * 2 ** 20
    ap, kw = acq_params(p)
    s = loose_state(p, st)
    ws = A.plain_ws(A.ws_size(engine.lib.gpx_sweep_workspace_size, n, 1, M))
    sref, u = oracle_scores(p)
    for scores in (None, A.out_f64(M)):
        bv_t, bi_t, *sc_t = with_prune(engine, prune, lambda: engine.acquire(
            st, t(p.Xs), "logei", index_offset=off, return_scores=scores is not None, **kw))
        bv, bi = A.out_f64(1), A.out_i64(1)
        with_prune(engine, prune, lambda: call(
            engine, "gpx_acquire_argmax_f64", ctypes.byref(pc), n, ptr(s.X), d + 3, ptr(s.W), npad + 6, ptr(s.a0),
            ptr(s.Xs), M, d + 5, ctypes.byref(ap), off, ptr(bv), ptr(bi), ptr(scores), ptr(ws), ws.numel()))
        assert same_bits(bv.view, bv_t) and same_bits(bi.view, bi_t)
        assert bv.outside_intact() and bi.outside_intact()
        i = int(bi.view.item()) - off
        check_argmax(i, sref, None, f"{kind} d={d} n={n} prune={prune}")
        assert abs(float(bv.view.item()) - sref[i]) <= 1e-8 * max(1.0, np.abs(sref[u > -10]).max())
        if scores is not None:
            assert same_bits(scores.view, sc_t[0]) and scores.outside_intact() and scores.sentinels() == 0
            check_scores(scores.view.cpu().numpy(), sref, u)
    assert unchanged(s.X, s.W, s.a0, s.Xs)


@pytest.mark.parametrize("prune", [0, 2])
@pytest.mark.parametrize("kind,d,n", SWEEP_CASES)
def test_acquire_topk(engine, kind, d, n, prune):
    """gpx_acquire_topk_f64 (ldx, ldw, ldxs), k = 5."""
    p, st = prob(kind, d, n), tight_fit(engine, kind, d, n)
    npad, pc, k = st.npad, p.kp.to_c(d), 5
    ap, kw = acq_params(p)
    s = loose_state(p, st)
    val_t, idx_t = with_prune(engine, prune, lambda: engine.acquire_topk(st, t(p.Xs), k, "logei", index_offset=11, **kw))
    val, idx = A.out_f64(k), A.out_i64(k)
    ws = A.plain_ws(A.ws_size(engine.lib.gpx_acquire_topk_workspace_size, n, M, k))
    with_prune(engine, prune, lambda: call(
        engine, "gpx_acquire_topk_f64", ctypes.byref(pc), n, ptr(s.X), d + 3, ptr(s.W), npad + 6, ptr(s.a0), ptr(s.Xs), M,
        d + 5, ctypes.byref(ap), 11, k, ptr(val), ptr(idx), ptr(ws), ws.numel()))
    assert same_bits(val.view, val_t) and same_bits(idx.view, idx_t)
    sref, u = oracle_scores(p)
    i = idx.view.cpu().numpy() - 11
    np.testing.assert_array_equal(i, O.topk_desc(sref, k)[1])
    assert np.abs(val.view.cpu().numpy() - sref[i]).max() <= 1e-8 * max(1.0, np.abs(sref[u > -10]).max())
    assert val.outside_intact() and idx.outside_intact() and unchanged(s.X, s.W, s.a0, s.Xs)


@pytest.mark.parametrize("prune", [0, 2])
@pytest.mark.parametrize("kind,d", CASES)
def test_acquire_multi_argmax_and_topk(engine, kind, d, prune):
    """gpx_acquire_argmax_multi_f64 and gpx_acquire_topk_multi_f64, T = 2: ldx, ldxs and a different ldw_host per
    output."""
    p = prob(kind, d)
    kps = [p.kp, p.kp.replace(outputscale=1.5, const_mean=-0.2)]
    sts = engine.fit_outputs(t(p.X), t(p.Y[:, :2]), kps, inverse=True)
    npad, T, k, w, ym, ys = sts[0].npad, 2, 5, [0.5, 1.0], [0.1, -0.2], [1.5, 0.7]
    kw = dict(kind="ucb", beta=4.0, weights=w, y_mean=ym, y_scale=ys, index_offset=3)
    X, Xs = A.rows(t(p.X), d + 3), A.rows(t(p.Xs), d + 5)
    ldw = [npad + 6, npad + 2]
    Ws = [A.matrix(npad, ldw[i], NAN, sts[i].W).freeze() for i in range(T)]
    als = [Win((npad,), None, NAN, sts[i].alpha[:, 0], lead=1).freeze() for i in range(T)]
    pcs = (KernelParamsC * T)(*[q.to_c(d) for q in kps])
    ap = AcqParamsC()
    ap.kind, ap.best_f, ap.beta, ap.y_mean, ap.y_scale = ACQ_KINDS["ucb"], 0.0, 4.0, 0.0, 1.0
    host = [pcs, T, N, ptr(X), d + 3, (ctypes.c_void_p * T)(*[w_.view.data_ptr() for w_ in Ws]), (ctypes.c_int64 * T)(*ldw),
            (ctypes.c_void_p * T)(*[a.view.data_ptr() for a in als]), (ctypes.c_double * T)(*w), (ctypes.c_double * T)(*ym),
            (ctypes.c_double * T)(*ys), ptr(Xs), M, d + 5, ctypes.byref(ap), 3]
    ost = O.fit_outputs(p.X, p.Y[:, :2], [to_oracle(q, d) for q in kps])
    sref = O.acquisition(*O.objective_posterior(ost, p.Xs, w, ym, ys), O.ACQ_UCB, 0.0, 4.0)
    tol = 1e-9 * max(1.0, np.abs(sref).max())
    # argmax, with the scores where the full sweep runs
    scores = A.out_f64(M) if prune == 0 else None
    bv_t, bi_t, *sc_t = with_prune(engine, prune, lambda: engine.acquire_multi(sts, t(p.Xs), return_scores=prune == 0, **kw))
    bv, bi = A.out_f64(1), A.out_i64(1)
    ws = A.plain_ws(A.ws_size(engine.lib.gpx_sweep_multi_workspace_size, N, M))
    with_prune(engine, prune, lambda: call(engine, "gpx_acquire_argmax_multi_f64", *host, ptr(bv), ptr(bi), ptr(scores),
                                           ptr(ws), ws.numel()))
    assert same_bits(bv.view, bv_t) and same_bits(bi.view, bi_t) and bv.outside_intact() and bi.outside_intact()
    check_argmax(int(bi.view.item()) - 3, sref, None, "multi")
    assert abs(float(bv.view.item()) - sref.max()) <= tol
    if scores is not None:
        assert same_bits(scores.view, sc_t[0]) and scores.outside_intact() and scores.sentinels() == 0
        assert np.abs(scores.view.cpu().numpy() - sref).max() <= tol
    # top-k
    val_t, idx_t = with_prune(engine, prune, lambda: engine.acquire_topk_multi(sts, t(p.Xs), k, **kw))
    val, idx = A.out_f64(k), A.out_i64(k)
    ws = A.plain_ws(A.ws_size(engine.lib.gpx_acquire_topk_multi_workspace_size, N, M, k))
    with_prune(engine, prune, lambda: call(engine, "gpx_acquire_topk_multi_f64", *host, k, ptr(val), ptr(idx), ptr(ws),
                                           ws.numel()))
    assert same_bits(val.view, val_t) and same_bits(idx.view, idx_t) and val.outside_intact() and idx.outside_intact()
    i = idx.view.cpu().numpy() - 3
    np.testing.assert_array_equal(i, O.topk_desc(sref, k)[1])
    assert np.abs(val.view.cpu().numpy() - sref[i]).max() <= tol
    assert unchanged(X, Xs, *Ws, *als)


# ---- gradients and the qNEI set-up -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", CASES)
def test_moments_grad(engine, kind, d):
    """gpx_moments_grad_f64: ldx, ldw, ldxs; 4 q-batches of 3."""
    p, st = prob(kind, d), tight_fit(engine, kind, d)
    npad, pc, m = st.npad, p.kp.to_c(d), 4 * Q
    tight = engine.moments_grad(st, t(p.Xq), Q)
    s = loose_state(p, st)
    outs = [A.out_f64(m), A.out_f64(m, d), A.out_f64(m, Q), A.out_f64(m, d, Q)]
    ws = A.plain_ws(A.ws_size(engine.lib.gpx_moments_grad_workspace_size, N, m))
    call(engine, "gpx_moments_grad_f64", ctypes.byref(pc), N, ptr(s.X), d + 3, ptr(s.W), npad + 6, ptr(s.a0), ptr(s.Xq), m,
         Q, d + 5, *[ptr(o) for o in outs], ptr(ws), ws.numel())
    sync()
    for o, a in zip(outs, tight):
        assert same_bits(o.view, a) and o.outside_intact() and o.sentinels() == 0
    ost = O.fit(p.X, p.Y[:, 0], p.op)
    rm, rdm, rc, rdc = O.moments_grad(ost, p.Xq, Q)
    mean, dmean, cov, dcov = (o.view.cpu().numpy() for o in outs)
    assert np.abs(mean - rm).max() <= 1e-9 * np.abs(rm).max()
    assert np.abs(dmean - rdm).max() <= 1e-8 * np.abs(rdm).max()
    assert np.abs(cov - rc).max() <= 1e-9 * p.op.outputscale
    assert np.abs(dcov - rdc).max() <= 1e-8 * np.abs(rdc).max()
    assert unchanged(s.X, s.W, s.a0, s.Xq)


@pytest.mark.parametrize("kind,d", CASES)
def test_joint_moments_and_cross_cov_grad(engine, kind, d):
    """gpx_joint_moments_f64 (ldx, ldw, ldxb, ldsb; mb = 70) and gpx_cross_cov_grad_f64 (ldx, ldsb, ldxb, ldxs; nb = 5,
    with and without dcross)."""
    p, st = prob(kind, d), tight_fit(engine, kind, d)
    npad, pc, lib = st.npad, p.kp.to_c(d), engine.lib
    s = loose_state(p, st)
    ost = O.fit(p.X, p.Y[:, 0], p.op)
    mean_t, cov_t, Sb_t = engine.joint_moments(st, t(p.Xb))
    ldsb = 130  # >= 70 rounded up to 64, even, no multiple of 64
    mean, cov, Sb = A.out_f64(MB), A.out_f64(MB, MB), Win((npad, 128), (ldsb, 1), SENT, tail=2 * ldsb)
    ws = A.plain_ws(A.ws_size(lib.gpx_joint_moments_workspace_size, N, MB))
    call(engine, "gpx_joint_moments_f64", ctypes.byref(pc), N, ptr(s.X), d + 3, ptr(s.W), npad + 6, ptr(s.a0), ptr(s.Xb),
         MB, d + 1, ptr(mean), ptr(cov), ptr(Sb), ldsb, ptr(ws), ws.numel())
    sync()
    assert same_bits(mean.view, mean_t) and same_bits(cov.view, cov_t) and same_bits(Sb.view[:, :MB], Sb_t[:, :MB])
    assert all(o.outside_intact() for o in (mean, cov, Sb))
    assert mean.sentinels() == 0 and cov.sentinels() == 0 and Sb.sentinels(Sb.view[:, :MB]) == 0
    Ks = O.kernel_matrix(p.X, p.Xb, p.op)
    S_ref = np.linalg.solve(ost.L.T, np.linalg.solve(ost.L, Ks))
    mean_r, cov_r = p.op.const_mean + Ks.T @ ost.alpha, O.kernel_matrix(p.Xb, p.Xb, p.op) - Ks.T @ S_ref
    assert np.abs(mean.view.cpu().numpy() - mean_r).max() <= 1e-9 * np.abs(mean_r).max()
    assert np.abs(cov.view.cpu().numpy() - cov_r).max() <= 1e-9 * np.abs(cov_r).max()
    assert unchanged(s.X, s.W, s.a0, s.Xb)
    # cross-covariance to the first nb baseline points, Sb from the engine's call on them
    m, Xb5 = 4 * Q, t(p.Xb[:NB])
    _, _, Sb5 = engine.joint_moments(st, Xb5)
    Sl = Win(Sb5.shape, (Sb5.shape[1] + 2, 1), NAN, Sb5, tail=8).freeze()
    Xb = A.rows(Xb5, d + 1)
    assert A.ws_size(lib.gpx_cross_cov_grad_workspace_size, N, NB, m) == 0  # (no workspace: ws = NULL below)
    S5 = S_ref[:, :NB]
    cross_r = O.kernel_matrix(p.Xq, p.Xb[:NB], p.op) - O.kernel_matrix(p.Xq, p.X, p.op) @ S5
    dcross_r = (O.kernel_grad_first(p.Xq, p.Xb[:NB], p.op).transpose(0, 2, 1)
                - np.einsum("anj,nb->ajb", O.kernel_grad_first(p.Xq, p.X, p.op), S5))
    for grad in (True, False):
        cross_t, dcross_t = engine.cross_cov_grad(st, Sb5, Xb5, t(p.Xq), need_grad=grad)
        cross, dcross = A.out_f64(m, NB), A.out_f64(m, d, NB) if grad else None
        call(engine, "gpx_cross_cov_grad_f64", ctypes.byref(pc), N, ptr(s.X), d + 3, ptr(Sl), Sb5.shape[1] + 2, ptr(Xb), NB,
             d + 1, ptr(s.Xq), m, d + 5, ptr(cross), ptr(dcross), None, 0)
        sync()
        assert same_bits(cross.view, cross_t) and cross.outside_intact() and cross.sentinels() == 0
        assert np.abs(cross.view.cpu().numpy() - cross_r).max() <= 1e-9 * np.abs(cross_r).max()
        if grad:
            assert same_bits(dcross.view, dcross_t) and dcross.outside_intact() and dcross.sentinels() == 0
            assert np.abs(dcross.view.cpu().numpy() - dcross_r).max() <= 1e-9 * np.abs(dcross_r).max()
    assert unchanged(s.X, Sl, Xb, s.Xq)


def check_mll(out, ref, n, d, T=1):
    assert abs(out[_capi.MLL_NLL] - ref["nll"]) <= 1e-10 * (abs(ref["quad"]) + T * (abs(ref["logdet"]) + n))
    got = {"noise": out[_capi.MLL_D_NOISE], "outputscale": out[_capi.MLL_D_OUTPUTSCALE], "const_mean": out[_capi.MLL_D_MEAN]}
    gmax = max([abs(ref[k]) for k in got] + list(np.abs(ref["lengthscale"])))
    for k in got:
        assert abs(got[k] - ref[k]) <= 1e-8 * (1 + gmax), k
    assert np.abs(out[_capi.MLL_D_LENGTHSCALE:][:d] - ref["lengthscale"]).max() <= 1e-8 * (1 + gmax)
    assert np.abs(out[_capi.MLL_D_LINVAR:][:d] - ref["linear_variance"]).max() <= 1e-8 * (1 + gmax)


@pytest.mark.parametrize("kind,d", CASES)
def test_mll_grad(engine, kind, d):
    """gpx_mll_grad_f64: ldx, ldy, ldl, ldw; three outputs sharing the hyperparameters."""
    p, st = prob(kind, d), tight_fit(engine, kind, d)
    npad, pc = st.npad, p.kp.to_c(d)
    tight = engine.mll_grad(st, t(p.Y))
    s = loose_state(p, st)
    out = A.out_f64(_capi.MLL_NOUT)
    ws = A.plain_ws(A.ws_size(engine.lib.gpx_mll_workspace_size, N))
    call(engine, "gpx_mll_grad_f64", ctypes.byref(pc), N, ptr(s.X), d + 3, ptr(s.Y), NRHS + 4, NRHS, ptr(s.L), npad + 2,
         ptr(s.W), npad + 6, ptr(s.alpha), ptr(out), ptr(ws), ws.numel())
    sync()
    assert same_bits(out.view, tight) and out.outside_intact() and out.sentinels() == 0
    check_mll(out.view.cpu().numpy(), O.mll_value_grad(p.X, p.Y, p.op), N, d, NRHS)
    assert unchanged(s.X, s.Y, s.L, s.W, s.alpha)


@pytest.mark.parametrize("kind,d", CASES)
def test_mll_grad_batched(engine, kind, d):
    """gpx_mll_grad_batched_f64 over the outputs of one fit_outputs call: stride_x = 0, stride_y = 1 with ldy = batch
    (the documented form), ldx, ldl / stride_l, ldw / stride_w and stride_alpha with gaps."""
    p = prob(kind, d)
    kps = [p.kp, p.kp.replace(outputscale=1.7, const_mean=-0.1), p.kp.replace(noise=3e-4)]
    sts = engine.fit_outputs(t(p.X), t(p.Y), kps, inverse=True)
    tight = engine.mll_grad_outputs(sts, t(p.Y))
    Lb, Wb, _, Ab, _ = sts[0]._batch
    npad = sts[0].npad
    X, Y = A.rows(t(p.X), d + 3), Win(p.Y.shape, None, NAN, t(p.Y), lead=1).freeze()
    L, sl = A.stack(BATCH, (npad, npad), (npad + 2, 1), 10, NAN, Lb)
    W, sw = A.stack(BATCH, (npad, npad), (npad + 6, 1), 14, NAN, Wb)
    al, sa = A.stack(BATCH, (npad, 1), (1, 1), 3, NAN, Ab, lead=1)
    L.freeze(), W.freeze(), al.freeze()
    out = A.out_f64(BATCH, _capi.MLL_NOUT)
    pcs = (KernelParamsC * BATCH)(*[q.to_c(d) for q in kps])
    ws = A.plain_ws(A.ws_size(engine.lib.gpx_mll_workspace_size, N))
    call(engine, "gpx_mll_grad_batched_f64", pcs, BATCH, N, ptr(X), d + 3, 0, ptr(Y), BATCH, 1, 1, ptr(L), npad + 2, sl,
         ptr(W), npad + 6, sw, ptr(al), sa, ptr(out), ptr(ws), ws.numel())
    sync()
    assert same_bits(out.view, tight) and out.outside_intact() and out.sentinels() == 0
    for b in range(BATCH):
        check_mll(out.view[b].cpu().numpy(), O.mll_value_grad(p.X, p.Y[:, b], to_oracle(kps[b], d)), N, d)
    assert unchanged(X, Y, L, W, al)


# ---- SVGP, farthest point sampling -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", CASES)
def test_svgp_prepare_predict_moments(engine, kind, d):
    """gpx_svgp_prepare_f64 (ldz, stride_z, stride_m, ldc, stride_c), gpx_svgp_predict_f64 (ldz, stride_z, ldxs, ldmean,
    ldvar) and gpx_svgp_moments_grad_f64 (ldz, ldxs); T = 2, M = 200."""
    T, Mi, lib = 2, 200, engine.lib
    Zn, vmean, vchol, kps, ops = svgp_problem(T, Mi, d, seed=T + Mi, kind=kind)
    Xn = np.random.default_rng(9).standard_normal((M, d))
    prep = engine.svgp_prepare(kps, Zn, vmean, vchol, jitter=SR.JITTER)
    Mpad = prep["W"].shape[1]
    pcs = (KernelParamsC * T)(*[q.to_c(d) for q in kps])
    ldz, ldc = d + 3, Mi + 2
    Z, sz = A.stack(T, (Mi, d), (ldz, 1), 7, NAN, t(Zn), lead=1)
    vm, sm = A.stack(T, (Mi,), (1,), 3, NAN, t(vmean), lead=1)
    vc, sc = A.stack(T, (Mi, Mi), (ldc, 1), 5, NAN, t(vchol), lead=1)
    Z.freeze(), vm.freeze(), vc.freeze()
    W, W2, alpha, info = A.out_f64(T, Mpad, Mpad), A.out_f64(T, Mpad, Mpad), A.out_f64(T, Mpad), A.out_i32(T)
    ws = A.plain_ws(A.ws_size(lib.gpx_svgp_prepare_workspace_size, Mi, T))
    call(engine, "gpx_svgp_prepare_f64", pcs, T, Mi, SR.JITTER, ptr(Z), ldz, sz, ptr(vm), sm, ptr(vc), ldc, sc, ptr(W),
         ptr(W2), ptr(alpha), ptr(info), ptr(ws), ws.numel())
    sync()
    for o, a in ((W, prep["W"]), (W2, prep["W2"]), (alpha, prep["alpha"])):
        assert same_bits(o.view, a) and o.outside_intact() and o.sentinels() == 0
    assert not bool(info.view.any()) and info.outside_intact() and unchanged(Z, vm, vc)
    # predict from the loosely prepared state
    mu_t, var_t, score_t = engine.svgp_predict(prep, t(Xn))
    Xs = A.rows(t(Xn), d + 5)
    mean, var, score = Win((M, T), (T + 1, 1), SENT, lead=1, tail=4), Win((M, T), (T + 2, 1), SENT, lead=1, tail=4), \
        A.out_f64(M)
    W.freeze(), W2.freeze(), alpha.freeze()
    ws = A.plain_ws(A.ws_size(lib.gpx_svgp_predict_workspace_size, Mi, M))
    call(engine, "gpx_svgp_predict_f64", pcs, T, Mi, ptr(Z), ldz, sz, ptr(W), ptr(W2), ptr(alpha), ptr(Xs), M, d + 5, 1e-10,
         ptr(mean), T + 1, ptr(var), T + 2, ptr(score), ptr(ws), ws.numel())
    sync()
    mu_r, var_r, score_r = O.svgp_predict(Zn, vmean, vchol, ops, Xn, jitter=SR.JITTER)
    for o, a, r in ((mean, mu_t, mu_r), (var, var_t, var_r), (score, score_t, score_r)):
        assert same_bits(o.view, a) and o.outside_intact() and o.sentinels() == 0
        assert np.abs(o.view.cpu().numpy() - r).max() <= 1e-9 * np.abs(r).max()
    assert unchanged(Z, W, W2, alpha, Xs)
    # q-batch moments of task 1
    task, m = 1, 4 * Q
    Xqn = np.random.default_rng(5).random((m, d))
    tight = engine.svgp_moments_grad(prep, task, t(Xqn), Q)
    Xq = A.rows(t(Xqn), d + 5)
    outs = [A.out_f64(m), A.out_f64(m, d), A.out_f64(m, Q), A.out_f64(m, d, Q)]
    pc = kps[task].to_c(d)
    ws = A.plain_ws(A.ws_size(lib.gpx_svgp_moments_grad_workspace_size, Mi, m))
    call(engine, "gpx_svgp_moments_grad_f64", ctypes.byref(pc), Mi, ptr(Z.view[task]), ldz, ptr(W.view[task]),
         ptr(W2.view[task]), ptr(alpha.view[task]), ptr(Xq), m, Q, d + 5, *[ptr(o) for o in outs], ptr(ws), ws.numel())
    sync()
    for o, a in zip(outs, tight):
        assert same_bits(o.view, a) and o.outside_intact() and o.sentinels() == 0
    rm, rdm, rc, rdc = SR.moments_grad(Zn[task], vmean[task], np.tril(vchol[task]), ops[task], Xqn, Q)
    mean, dmean, cov, dcov = (o.view.cpu().numpy() for o in outs)
    assert np.abs(mean - rm).max() <= 1e-9 * np.abs(rm).max()
    assert np.abs(dmean - rdm).max() <= 1e-8 * np.abs(rdm).max()
    assert np.abs(cov - rc).max() <= 1e-9 * SR.prior_scale(ops[task], Xqn)
    assert np.abs(dcov - rdc).max() <= 1e-8 * np.abs(rdc).max()
    assert unchanged(Z, W, W2, alpha, Xq)


@pytest.mark.parametrize("d", [3, 17])
def test_fps(engine, d):
    """gpx_fps_f64: ldx."""
    Xn = np.random.default_rng(d).random((M, d))
    k, start = 20, 5
    tight = engine.fps(t(Xn), k, start)
    X, idx = A.rows(t(Xn), d + 3), A.out_i64(k)
    call(engine, "gpx_fps_f64", ptr(X), M, d, d + 3, k, start, ptr(idx))
    sync()
    assert same_bits(idx.view, tight) and idx.outside_intact() and X.unchanged()
    np.testing.assert_array_equal(idx.view.cpu().numpy(), O.farthest_point_sampling(Xn, k, start))
